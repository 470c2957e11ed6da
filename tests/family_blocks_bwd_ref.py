"""A float64 restatement of the three family-block backward formulas (include/bayeformers_amd_family_blocks_bwd.h:
bf_norm_add_rmsnorm_bwd, bf_qknorm_rope_bwd, bf_geglu_bwd).  Inputs are taken as they are stored (the rounded values of
whatever dtype they have), every result is float64, and beside each gradient whose terms can cancel comes the magnitude
those terms had before they were added, in the style of decoder_blocks_bwd_ref.py.  tests/test_family_blocks_bwd_cpu.py pins
the restatement to torch.autograd.grad through transformers' own code in float64."""
import math

import torch

from decoder_blocks_bwd_ref import rope_bwd_ref

K2C = 2.0 * math.sqrt(2.0 / math.pi)
K2CA = K2C * 0.044715


def _rms_stage(v, w, cot, mag_cot, eps):
    """One RMSNorm's backward over the last axis, y = v r w with r = rsqrt(mean(v^2) + eps), for the cotangent `cot` whose
    own terms had the magnitude `mag_cot` (>= |cot|) -> (dv, mag_dv, terms of dw [.., N], their magnitudes):
        dv = r (w o cot) - v r^3 mean(v o w o cot),   dw = sum cot o v r;
    mag_dv = r |w| mag_cot + |v| r^3 mean(|v w| mag_cot), the map applied to magnitudes; the dw terms' are mag_cot |v| r."""
    r = 1.0 / torch.sqrt((v * v).sum(-1, keepdim=True) / v.shape[-1] + float(eps))
    b = w * cot
    dv = r * b - v * r ** 3 * (v * b).mean(-1, keepdim=True)
    mb = w.abs() * mag_cot
    mag = r * mb + v.abs() * r ** 3 * (v.abs() * mb).mean(-1, keepdim=True)
    return dv, mag, cot * v * r, mag_cot * v.abs() * r


def norm_add_rmsnorm_bwd_ref(x, z, gamma_pre, gamma_out, dy, eps_pre, eps_out, weight_offset, dz_in=None):
    """For u = x r(x) (woff + gp) (x itself without gamma_pre), z = res + u, y = z r(z) (woff + go), from the stored z (and
    x): a dict of float64 tensors.
      stage 2:  dz = r_z a - z r_z^3 mean(z o a) + dz_in with a = (woff + go) o dy (dy None: dz = dz_in), the gradient of
                the residual; dgamma_out = sum_rows dy o z r_z (dy None: 0).
      stage 1:  with gamma_pre, dz (float64) as the cotangent: dx = r_x b - x r_x^3 mean(x o b), b = (woff + gp) o dz,
                dgamma_pre = sum_rows dz o x r_x; without it dx = dz.
    mag_dz = |r a| + |z| r^3 mean|z a| + |dz_in|; mag_dx = stage 1's map applied to mag_dz (the magnitudes through both
    stages); mag_dgamma_out = sum_rows |dy z r_z|; mag_dgamma_pre = sum_rows mag_dz |x| r_x."""
    z = z.double()
    N = z.shape[-1]
    out = {}
    if dy is not None:
        dy = dy.double()
        dz, mag, t, tm = _rms_stage(z, float(weight_offset) + gamma_out.double(), dy, dy.abs(), eps_out)
        out["dgamma_out"], out["mag_dgamma_out"] = t.reshape(-1, N).sum(0), tm.reshape(-1, N).sum(0)
    else:
        dz, mag = torch.zeros_like(z), torch.zeros_like(z)
        out["dgamma_out"] = out["mag_dgamma_out"] = torch.zeros(N, dtype=torch.float64, device=z.device)
    if dz_in is not None:
        dz, mag = dz + dz_in.double(), mag + dz_in.double().abs()
    out["dz"], out["mag_dz"] = dz, mag
    if gamma_pre is None:
        out["dx"], out["mag_dx"] = dz, mag
        return out
    dx, mag_x, t, tm = _rms_stage(x.double(), float(weight_offset) + gamma_pre.double(), dz, mag, eps_pre)
    out["dx"], out["mag_dx"] = dx, mag_x
    out["dgamma_pre"], out["mag_dgamma_pre"] = t.reshape(-1, N).sum(0), tm.reshape(-1, N).sum(0)
    return out


def qknorm_rope_bwd_ref(dout, cos, sin, x=None, gamma=None, eps=0.0, weight_offset=0):
    """The transpose of family_blocks_ref.qknorm_rope_ref for one tensor: dout [B, heads, T, D], cos / sin [1 or B, T, D],
    x the forward's input -> (dx, mag_dx, dgamma, mag_dgamma).  dn = rope_bwd_ref(dout) (written for unequal table halves);
    without a gamma dx = dn and the dgammas are None; with one, the RMSNorm's backward over D with dn as the cotangent,
    dgamma = sum_{b, heads, t} dn o x r, and the magnitudes are the norm's map applied to the rotation's."""
    dn, mag = rope_bwd_ref(dout, cos, sin)
    if gamma is None:
        return dn, mag, None, None
    D = dn.shape[-1]
    dx, mag_x, t, tm = _rms_stage(x.double(), float(weight_offset) + gamma.double(), dn, mag, eps)
    return dx, mag_x, t.reshape(-1, D).sum(0), tm.reshape(-1, D).sum(0)


def geglu_bwd_ref(gate, up, dy):
    """-> (dgate, dup, mag_dgate) for y = g s u, s = sigmoid(2k), 2k = g (2c + 2c 0.044715 g^2), c = sqrt(2 / pi):
        dup = dy g s,   dgate = dy u s (1 + g q (1 - s)),   q = d(2k)/dg = 2c (1 + 3 * 0.044715 g^2);
    mag_dgate = |dy u s| (1 + |g q| (1 - s)), the two terms of dgate before they are added (they cancel for negative
    gates).  1 - s is taken as sigmoid(-2k): no cancellation of its own, and where it (or s) is 0 the product with g q,
    finite in float64 for every gate of a 16- or 32-bit dtype, is 0 too."""
    g, u, dy = gate.double(), up.double(), dy.double()
    a = g * (K2C + K2CA * g * g)
    s, ms = torch.sigmoid(a), torch.sigmoid(-a)
    gq = g * (K2C + 3.0 * K2CA * g * g)
    return dy * u * (s * (1.0 + gq * ms)), dy * (g * s), (dy * u * s).abs() * (1.0 + gq.abs() * ms)
