"""tests/attention_ref.py — the float64 restatement the encoder attention kernels are held to — against torch's own softmax,
logsumexp and autograd in float64, on the CPU.  float64 against float64: the bound 1e-12 (relative to max |reference|) is
~4 decimal orders above what a 64-key-deep fp64 contraction of O(1) terms rounds to, and 4 below the fp16 tolerances."""
import math

import numpy as np
import pytest
import torch

from attention_ref import attention_ref
from oracle import bayes_oracle as bo

SEED = 0x5EED
REL = 1e-12


def _inputs(B, H, T, seed, gain=1.0):
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(B, T, H * 64, generator=g).to(torch.bfloat16).view(B, T, H, 64).transpose(1, 2) for _ in range(3))
    go = torch.randn(B, T, H, 64, generator=g).to(torch.bfloat16)
    return q * gain, k, v, go


def _mask(kind, B, T, fill):
    if kind == "none":
        return None
    m = torch.zeros(B, T)
    m[0, T - 37:] = fill          # right tail
    m[B - 1, :T // 2 + 5] = fill  # left head past the middle
    if B > 2:
        m[1, 40:77] = fill        # a hole
    return m


def _rel(a, r):
    return (a - r).abs().max().item() / max(r.abs().max().item(), 1e-300)


def _autograd(q, k, v, mask, scale, keep, inv_keep, go):
    qq, kk, vv = (t.detach().double().clone().requires_grad_(True) for t in (q, k, v))
    s = qq @ kk.transpose(-1, -2) * scale
    if mask is not None:
        s = s + mask.double()[:, None, None, :]
    p = torch.softmax(s, -1)
    if keep is not None:
        p = p * keep.double() * inv_keep
    out = (p @ vv).transpose(1, 2)
    out.backward(go.double())
    lse = torch.logsumexp(s.detach(), -1) / math.log(2.0)
    return out.detach(), lse, qq.grad.transpose(1, 2), kk.grad.transpose(1, 2), vv.grad.transpose(1, 2)


@pytest.mark.parametrize("B,H,T", [(1, 1, 128), (3, 2, 128), (2, 3, 256)])
@pytest.mark.parametrize("mask,fill", [("none", 0.0), ("some", float("-inf")), ("some", -1e4)])
@pytest.mark.parametrize("p", [0.0, 0.25])
def test_restatement_matches_torch_autograd_in_float64(B, H, T, mask, fill, p):
    q, k, v, go = _inputs(B, H, T, seed=B * 100 + T + H, gain=2.0)
    m = _mask(mask, B, T, fill)
    keep = torch.from_numpy(bo.attention_keep_mask(B, H, T, p, SEED, 3, 4)) if p > 0 else None
    inv = float(bo.dropout_keep_scale(p))
    r = attention_ref(q, k, v, m, 0.125, keep=keep, p=p, go=go)
    out, lse, dq, dk, dv = _autograd(q, k, v, m, 0.125, keep, inv, go)
    assert r.out.shape == (B, T, H, 64) and r.lse.shape == (B, H, T) and r.delta.shape == (B, H, T)
    for name, got, want in (("out", r.out, out), ("dq", r.dq, dq), ("dk", r.dk, dk), ("dv", r.dv, dv)):
        assert _rel(got, want) <= REL, (name, _rel(got, want))
    assert (r.lse - lse).abs().max().item() <= REL * lse.abs().max().item()
    assert _rel(r.delta, (go.double() * out).sum(-1).transpose(1, 2)) <= REL
    cs = r.colsum(B)
    assert cs.shape == (3, B, H * 64)
    for t, g in enumerate((dq, dk, dv)):
        flat = g.reshape(B, T, H * 64)  # (the column sums of dk are 0 in exact arithmetic: relative to sum |x|)
        assert (cs[t] - flat.sum(1)).abs().max().item() <= REL * flat.abs().sum(1).max().item()


def test_out_is_softmax_times_v():
    q, k, v, _ = _inputs(2, 2, 128, seed=1)
    r = attention_ref(q, k, v, None, 0.125)
    want = torch.softmax(q.double() @ k.double().transpose(-1, -2) * 0.125, -1) @ v.double()
    assert _rel(r.out, want.transpose(1, 2)) <= REL
    assert r.dq is None and r.delta is None


@pytest.mark.parametrize("p", [0.0, 0.5])
def test_a_fully_masked_sequence_gives_zeros_and_an_infinite_lse(p):
    B, H, T = 3, 2, 128
    q, k, v, go = _inputs(B, H, T, seed=2)
    m = torch.zeros(B, T)
    m[1] = float("-inf")
    m[2, 100:] = float("-inf")
    keep = torch.from_numpy(bo.attention_keep_mask(B, H, T, p, SEED, 1, 1)) if p > 0 else None
    r = attention_ref(q, k, v, m, 0.125, keep=keep, p=p, go=go)
    for t in (r.out, r.lse, r.delta, r.dq, r.dk, r.dv):
        assert not torch.isnan(t).any()
    assert (r.out[1] == 0).all() and (r.dq[1] == 0).all() and (r.dk[1] == 0).all() and (r.dv[1] == 0).all()
    assert (r.delta[1] == 0).all() and (r.lse[1] == float("inf")).all()
    assert torch.isfinite(r.lse[0]).all() and torch.isfinite(r.lse[2]).all()
    assert (r.dk[2, 100:] == 0).all() and (r.dv[2, 100:] == 0).all()  # hidden keys get no gradient
    # the neighbours are what they are without that sequence
    sel = [0, 2]
    r2 = attention_ref(q[sel], k[sel], v[sel], m[sel], 0.125, keep=None if keep is None else keep[sel], p=p, go=go[sel])
    for a, b in ((r.out, r2.out), (r.lse, r2.lse), (r.dq, r2.dq), (r.dk, r2.dk), (r.dv, r2.dv)):
        assert torch.equal(a[sel], b)


@pytest.mark.parametrize("chunk", [128 * 128 * 8, 3 * 256 * 256 * 8, 1 << 20])
def test_chunked_equals_unchunked(chunk):
    """One (sequence, head) at a time, a few heads at a time, a few sequences at a time: the slabs are independent, and a
    batched fp64 matmul computes each [T, T] product on its own — the same bits."""
    B, H, T = 3, 3, 256
    q, k, v, go = _inputs(B, H, T, seed=3)
    m = _mask("some", B, T, float("-inf"))
    keep = torch.from_numpy(bo.attention_keep_mask(B, H, T, 0.1, SEED, 2, 7))
    whole = attention_ref(q, k, v, m, 0.125, keep=keep, p=0.1, go=go, chunk_bytes=None)
    parts = attention_ref(q, k, v, m, 0.125, keep=keep, p=0.1, go=go, chunk_bytes=chunk)
    for name in ("out", "lse", "delta", "dq", "dk", "dv"):
        a, b = getattr(whole, name), getattr(parts, name)
        assert _rel(b, a) <= 1e-14, name


def test_lse_is_in_log2_units():
    q, k, v, _ = _inputs(1, 1, 128, seed=4)
    r = attention_ref(q * 0, k, v, None, 0.125)
    assert (r.lse - 7.0).abs().max().item() <= 1e-12  # 128 equal scores of 0: log2(128)
    assert np.isclose(r.out[0, 0, 0].numpy(), v.double().mean(2)[0, 0].numpy(), rtol=0, atol=1e-14).all()
