"""A float64 restatement of the three decoder-block backward formulas (include/bayeformers_amd.h: bf_add_rmsnorm_bwd,
bf_rope_qk_bwd, bf_swiglu_bwd).  Inputs are taken as they are (the rounded values of whatever dtype they have), every
result is float64, and beside each gradient whose terms can cancel comes the magnitude those terms had before they were
added, as rope_ref returns it.  tests/test_decoder_blocks_bwd_cpu.py pins the restatement to torch.autograd.grad through
transformers' own code in float64."""
import torch


def add_rmsnorm_bwd_ref(z, gamma, dy, eps, dz_in=None):
    """For y = z r gamma with r = rsqrt(mean(z^2) + eps) over the last axis -> (dz, dgamma, mag_dz, mag_dgamma):
        dz = r (gamma o dy) - z r^3 mean(z o gamma o dy) + dz_in,      dgamma = sum_rows dy o z r,
    mag_dz = |r gamma dy| + |z| r^3 mean|z gamma dy| + |dz_in| (the row mean is itself a sum that cancels) and
    mag_dgamma = sum_rows |dy z r|."""
    z, g, dy = z.double(), gamma.double(), dy.double()
    r = 1.0 / torch.sqrt((z * z).sum(-1, keepdim=True) / z.shape[-1] + float(eps))
    a = g * dy
    t1 = r * a
    dz = t1 - z * r ** 3 * (z * a).mean(-1, keepdim=True)
    mag = t1.abs() + z.abs() * r ** 3 * (z * a).abs().mean(-1, keepdim=True)
    if dz_in is not None:
        dz = dz + dz_in.double()
        mag = mag + dz_in.double().abs()
    t = (dy * z * r).reshape(-1, z.shape[-1])
    return dz, t.sum(0), mag, t.abs().sum(0)


def rope_bwd_ref(dy, cos, sin):
    """dy [B, heads, T, D], cos / sin [1 or B, T, D] -> (dx, magnitude) of the forward y1 = x1 c1 - x2 s1,
    y2 = x2 c2 + x1 s2 (c1, s1 / c2, s2: the two halves of the tables): dx1 = dy1 c1 + dy2 s2, dx2 = dy2 c2 - dy1 s1."""
    dy, c, s = dy.double(), cos.double()[:, None], sin.double()[:, None]
    h = dy.shape[-1] // 2
    d1, d2, c1, c2, s1, s2 = dy[..., :h], dy[..., h:], c[..., :h], c[..., h:], s[..., :h], s[..., h:]
    dx = torch.cat((d1 * c1 + d2 * s2, d2 * c2 - d1 * s1), -1)
    mag = torch.cat(((d1 * c1).abs() + (d2 * s2).abs(), (d2 * c2).abs() + (d1 * s1).abs()), -1)
    return dx, mag


def swiglu_bwd_ref(gate, up, dy):
    """-> (dgate, dup, mag_dgate) for y = silu(gate) up, s = 1 / (1 + exp(-gate)): dgate = dy up s (1 + gate (1 - s)),
    dup = dy gate s; mag_dgate = |dy up s| (1 + |gate| (1 - s)), the two terms of dgate before they are added (they cancel
    near gate = -1.278).  1 - s is taken as sigmoid(-gate): no cancellation of its own for large gates."""
    g, u, dy = gate.double(), up.double(), dy.double()
    s, ms = torch.sigmoid(g), torch.sigmoid(-g)
    return dy * u * s * (1.0 + g * ms), dy * g * s, (dy * u * s).abs() * (1.0 + g.abs() * ms)
