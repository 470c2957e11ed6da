"""A float64 restatement of the LayerNorm entries from their formulas (include/bayeformers_amd.h: bf_add_layernorm and
its dropout / strided-rows forms, bf_embed_layernorm, bf_add_layernorm_bwd and its dropout / two-gradient forms; the
backward's formulas are the header comment of add_layernorm_bwd_kernel in bayeformers_amd/csrc/bf_norm.hip).  Inputs are
taken as they are (the rounded values of whatever dtype they have) and every result is float64;
tests/test_layernorm_ref_cpu.py pins the restatement to torch's layer_norm, float64 autograd and HF BertEmbeddings run in
float64.

Besides the results every function returns the MAGNITUDES its result had before cancellation, which the bounds of
tests/test_gpu_layernorm.py are made of: a LayerNorm row whose mean is far above its spread, or a sum of gradients that
cancels, is ill conditioned, and an fp32 evaluation may be wrong by its unit roundoff times those magnitudes, not times the
result."""
from types import SimpleNamespace

import torch


def _row_stats(z, eps):
    """(z - mean, 1 / sqrt(biased variance + eps)) over the last axis: the two-pass formula."""
    n = z.shape[-1]
    d = z - z.sum(-1, keepdim=True) / n
    var = (d * d).sum(-1, keepdim=True) / n
    return d, 1.0 / torch.sqrt(var + float(eps))


def _sum_rows(x, residual, keep, keep_scale):
    """(z, |x * keep * keep_scale| or None): z = x * keep * keep_scale + residual.  With dropout the scaled x is rounded to
    fp32 once before the residual is added: that one rounding is relative to the product, not to the sum."""
    z = x.double()
    xs = None
    if keep is not None:
        z = z * keep.double() * float(keep_scale)
        xs = z.abs()
    if residual is not None:
        z = z + residual.double()
    return z, xs


def _row_mean(t):
    return t.sum(-1, keepdim=True) / t.shape[-1]


def add_layernorm_ref(x, residual, gamma, beta, eps, keep=None, keep_scale=1.0):
    """(y, cond): z = x * keep * keep_scale + residual (keep: the 0 / 1 dropout mask, None = no dropout; residual may be
    None), zh = (z - mean) * rstd with the biased variance and eps inside the square root, y = zh * gamma + beta;
    cond = (|z| + mean_row |z|) * rstd * |gamma|, the magnitude y's first term had before z - mean cancelled."""
    z, _ = _sum_rows(x, residual, keep, keep_scale)
    d, rstd = _row_stats(z, eps)
    y = d * rstd * gamma.double() + beta.double()
    return y, (z.abs() + _row_mean(z.abs())) * rstd * gamma.double().abs()


def dropout_product_ref(x, residual, gamma, eps, keep, keep_scale):
    """(|xs| + mean_row |xs|) * rstd * |gamma| with xs = x * keep * keep_scale and rstd of z = xs + residual: what ONE
    rounding of the product xs is relative to, by the time it has reached y directly and through the mean."""
    z, xs = _sum_rows(x, residual, keep, keep_scale)
    _, rstd = _row_stats(z, eps)
    return (xs + _row_mean(xs)) * rstd * gamma.double().abs()


def embed_layernorm_ref(ids, type_ids, pos_ids, word, type, pos, gamma, beta, eps, seq_len):
    """(y, cond) [B, L, N]: y = LayerNorm((word[ids] + type[type_ids or 0]) + pos[pos_ids or position in the sequence]).
    ids [B, L]; type_ids [B, L] or None; pos_ids [1 or B, L] or None; seq_len = L.  cond is add_layernorm_ref's with
    |word| + |type| + |pos| in place of |z|: the kernel adds the three rows in fp32, and the roundings of those two adds are
    relative to the addends.  A row with an id outside its table is NaN in both results."""
    B, L = ids.shape
    assert L == seq_len
    ti = torch.zeros_like(ids) if type_ids is None else type_ids.expand(B, L)
    pi = torch.arange(L, device=ids.device)[None].expand(B, L) if pos_ids is None else pos_ids.expand(B, L)
    bad = ((ids < 0) | (ids >= word.shape[0]) | (ti < 0) | (ti >= type.shape[0]) | (pi < 0) | (pi >= pos.shape[0]))
    wi, ti, pi = (torch.where(bad, torch.zeros_like(ids), i) for i in (ids, ti, pi))
    w, t, p = word.double()[wi], type.double()[ti], pos.double()[pi]
    z = (w + t) + p
    zabs = w.abs() + t.abs() + p.abs()
    d, rstd = _row_stats(z, eps)
    y = d * rstd * gamma.double() + beta.double()
    cond = (zabs + _row_mean(zabs)) * rstd * gamma.double().abs()
    nan = torch.full_like(y, float("nan"))
    return torch.where(bad[..., None], nan, y), torch.where(bad[..., None], nan, cond)


def add_layernorm_bwd_ref(x, residual, gamma, dy, eps, dy2=None, keep=None, keep_scale=1.0):
    """(dz, dx, dgamma, dbeta, m) for out = LayerNorm(x * keep * keep_scale + residual) * gamma + beta and the output
    gradient g = dy + dy2.  With zh = (z - mean) * rstd and a = g * gamma:
        dz = rstd * (a - mean_row(a) - zh * mean_row(a * zh))    the gradient of z, so of the residual
        dx = dz * keep * keep_scale                              (dz itself without dropout)
        dgamma = sum_rows g * zh,   dbeta = sum_rows g
    m holds the magnitudes: zmag = (|z| + mean_row |z|) * rstd (what zh was before z - mean cancelled), xsmag = the same of
    xs = x * keep * keep_scale (None without dropout: what the one rounding of that product is relative to), zh = |zh|,
    a = |a|, a_mean = mean_row |a|, s2 = |mean_row(a * zh)|, azh_mean = mean_row |a * zh|, rstd, g = |g|, gzh_sum =
    sum_rows |g * zh|, g_sum = sum_rows |g|, and scale = keep * keep_scale (None without dropout)."""
    N = x.shape[-1]
    z, xs = _sum_rows(x.reshape(-1, N), None if residual is None else residual.reshape(-1, N),
                      None if keep is None else keep.reshape(-1, N), keep_scale)
    zabs = z.abs()
    d, rstd = _row_stats(z, eps)
    zh = d * rstd
    g = dy.double().reshape(-1, N)
    if dy2 is not None:
        g = g + dy2.double().reshape(-1, N)
    a = g * gamma.double()
    s1, s2 = _row_mean(a), _row_mean(a * zh)
    dz = rstd * (a - s1 - zh * s2)
    scale = None if keep is None else keep.double().reshape(-1, N) * float(keep_scale)
    dx = dz if scale is None else dz * scale
    m = SimpleNamespace(zmag=(zabs + _row_mean(zabs)) * rstd, xsmag=None if xs is None else (xs + _row_mean(xs)) * rstd,
                        zh=zh.abs(), a=a.abs(), a_mean=_row_mean(a.abs()), s2=s2.abs(),
                        azh_mean=_row_mean((a * zh).abs()), rstd=rstd, g=g.abs(), gzh_sum=(g * zh).abs().sum(0),
                        g_sum=g.abs().sum(0), scale=scale)
    return dz, dx, (g * zh).sum(0), g.sum(0), m
