"""A float64 restatement of the three decoder-block ops from their formulas (include/bayeformers_amd.h: bf_add_rmsnorm,
bf_rope_qk, bf_swiglu).  Inputs are taken as they are (the rounded values of whatever dtype they have) and every result
is float64; tests/test_decoder_blocks_cpu.py pins the restatement to transformers' own modules run in float64."""
import torch


def add_rmsnorm_ref(x, residual, gamma, eps, dtype=None):
    """(z, y): z = x + residual in float64 — rounded to `dtype` when one is given, as the kernel's sum output is, and the
    statistics and y then come from that rounded z — and y = z / sqrt(mean(z^2) + eps) * gamma."""
    z = x.double() if residual is None else x.double() + residual.double()
    if dtype is not None and residual is not None:
        z = z.to(dtype).double()
    var = (z * z).sum(-1, keepdim=True) / z.shape[-1]
    return z, z / torch.sqrt(var + float(eps)) * gamma.double()


def rope_ref(x, cos, sin):
    """x [B, heads, T, D], cos / sin [1 or B, T, D] -> (x cos + rotate_half(x) sin, |x cos| + |rotate_half(x) sin|) in
    float64, rotate_half(x) = [-x2, x1] over the two halves of the last axis.  The second result is the magnitude the two
    terms had before they were added (they can cancel)."""
    x, c, s = x.double(), cos.double()[:, None], sin.double()[:, None]
    half = x.shape[-1] // 2
    rot = torch.cat((-x[..., half:], x[..., :half]), dim=-1)
    return x * c + rot * s, (x * c).abs() + (rot * s).abs()


def swiglu_ref(gate, up):
    """silu(gate) * up with silu(g) = g / (1 + exp(-g)), float64 (exp overflows to inf below about -709: g / inf = -0)."""
    g = gate.double()
    return g / (1.0 + torch.exp(-g)) * up.double()
