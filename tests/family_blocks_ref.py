"""A float64 restatement of the three family-block ops from their formulas (include/bayeformers_amd_family_blocks.h:
bf_norm_add_rmsnorm, bf_qknorm_rope, bf_geglu).  Inputs are taken as they are (the rounded values of whatever dtype they
have) and every result is float64; tests/test_family_blocks_cpu.py pins the restatement to transformers' own modules run
in float64."""
import math

import torch

from decoder_blocks_ref import rope_ref


def rmsnorm64(x, gamma, eps, weight_offset):
    x = x.double()
    var = (x * x).sum(-1, keepdim=True) / x.shape[-1]
    return x / torch.sqrt(var + float(eps)) * (float(weight_offset) + gamma.double())


def round_once(t, dtype):
    """float64 -> dtype -> float64 with ONE rounding to nearest even.  torch may convert float64 to a 16-bit type through
    float32, which rounds twice: go through float32 rounded to odd instead (truncated towards zero, the last bit set when
    anything was cut off), which the second rounding to a much narrower format cannot double-round."""
    f = t.float()
    if dtype == torch.float32:
        return f.double()
    bits = f.view(torch.int32)  # sign and magnitude: - 1 is one step towards zero
    bits = torch.where(f.double().abs() > t.abs(), bits - 1, bits)
    bits = torch.where(bits.view(torch.float32).double() != t, bits | 1, bits)
    return bits.view(torch.float32).to(dtype).double()


def norm_add_rmsnorm_ref(x, gamma_pre, residual, gamma_out, eps_pre, eps_out, weight_offset, dtype=None):
    """(u, z, y) in float64: u = x normalised under gamma_pre (x itself without one), z = residual + u (u without a
    residual), y = z normalised under gamma_out.  With a `dtype`, u and z are rounded to it where the kernel rounds them
    (after the first norm, after the add), and the statistics of y come from the rounded z."""
    def rnd(t):
        return round_once(t, dtype) if dtype is not None else t

    u = x.double() if gamma_pre is None else rnd(rmsnorm64(x, gamma_pre, eps_pre, weight_offset))
    z = u if residual is None else rnd(residual.double() + u)
    return u, z, rmsnorm64(z, gamma_out, eps_out, weight_offset)


def qknorm_rope_ref(x, cos, sin, gamma, eps, weight_offset):
    """x [B, heads, T, D] -> (y, mag): every head normalised over D under gamma (x itself when gamma is None), unrounded,
    then rope_ref of it — its result and the magnitude of the two terms of the rotation before they were added."""
    n = x.double() if gamma is None else rmsnorm64(x, gamma, eps, weight_offset)
    return rope_ref(n, cos, sin)


def geglu_ref(gate, up):
    """g u / (1 + exp(-2k)), k = sqrt(2/pi) (g + 0.044715 g^3), float64: 0.5 g (1 + tanh k) u without the cancellation
    (exp overflows to inf for 2k below about -709: g / inf = -0)."""
    g = gate.double()
    k = math.sqrt(2.0 / math.pi) * (g + 0.044715 * g * g * g)
    return g / (1.0 + torch.exp(-2.0 * k)) * up.double()
