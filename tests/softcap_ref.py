"""float64 restatement of causal grouped-query attention with soft-capped logits (Gemma 2):

    z = scale q . k,   s = softcap tanh(z / softcap) (s = z without a softcap),   then + key mask, then the causal /
    window visibility, then the softmax over the keys.

Query i of Tq (index Tk - Tq + i) sees key j iff j <= index and index - j < W.  The gradients are the closed form the
backward kernels implement, ds_z = p (dp - delta) (1 - th^2) with th = tanh(z / softcap), not autograd's (the CPU test
holds the two together).  Shared by tests/test_softcap_cpu.py and tests/test_gpu_softcap_attention.py: no GPU needed."""
import math

import torch

LN2 = math.log(2.0)


def visible(Tq, Tk, W, device):
    """[Tq, Tk] bool; W None: causal only"""
    i = (Tk - Tq + torch.arange(Tq, device=device))[:, None]
    j = torch.arange(Tk, device=device)[None, :]
    seen = j <= i
    return seen if W is None else seen & (i - j < W)


def scores(q64, k64, scale, softcap):
    """(s, th): the capped scores and tanh(z / softcap) (None without a cap); differentiable"""
    z = q64 @ k64.transpose(-1, -2) * scale
    if softcap is None:
        return z, None
    th = torch.tanh(z / softcap)
    return th * softcap, th


def forward(q, k, v, key_mask, scale, W=None, softcap=None):
    """float64 (out [B, H, Tq, D], lse [B, H, Tq] in log2 units, p, th) of q [B, H, Tq, D], k / v [B, Hkv, Tk, D] (any
    floating dtype, cast here; G = H / Hkv query heads share a K/V head); differentiable in q, k, v"""
    H, Tq = q.shape[1], q.shape[2]
    Hkv, Tk = k.shape[1], k.shape[2]
    G = H // Hkv
    q64, k64, v64 = q.double(), k.double().repeat_interleave(G, 1), v.double().repeat_interleave(G, 1)
    s, th = scores(q64, k64, scale, softcap)
    if key_mask is not None:
        s = s + key_mask.double()[:, None, None, :]
    s = s.masked_fill(~visible(Tq, Tk, W, q.device), float("-inf"))
    m = s.amax(-1, keepdim=True)
    ok = torch.isfinite(m)
    m = torch.where(ok, m, torch.zeros_like(m)).detach()
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    p = torch.where(ok, e / torch.where(ok, l, torch.ones_like(l)), torch.zeros_like(e))
    lse = torch.where(ok, (m + torch.log(torch.where(ok, l, torch.ones_like(l)))) / LN2, torch.full_like(m, float("inf")))
    return p @ v64, lse[..., 0], p, th


def reference(q, k, v, key_mask, scale, W=None, softcap=None, go=None):
    """[out [B, Tq, H, D], lse [B, H, Tq] (log2 units, +inf for a row with no visible key)] and, given the output
    gradient go [B, Tq, H, D], + [dq [B, Tq, H, D], dk, dv [B, Tk, Hkv, D]] (summed over each group), all float64."""
    B, H, Tq, D = q.shape
    Hkv, Tk = k.shape[1], k.shape[2]
    G = H // Hkv
    with torch.no_grad():
        out, lse, p, th = forward(q, k, v, key_mask, scale, W, softcap)
        res = [out.transpose(1, 2), lse]
        if go is not None:
            q64, k64, v64 = q.double(), k.double().repeat_interleave(G, 1), v.double().repeat_interleave(G, 1)
            g = go.double().transpose(1, 2)
            dp = g @ v64.transpose(-1, -2)
            ds = p * (dp - (g * out).sum(-1, keepdim=True))
            if th is not None:
                ds = ds * (1.0 - th * th)
            res += [(scale * ds @ k64).transpose(1, 2),
                    (scale * ds.transpose(-1, -2) @ q64).view(B, Hkv, G, Tk, D).sum(2).transpose(1, 2),
                    (p.transpose(-1, -2) @ g).view(B, Hkv, G, Tk, D).sum(2).transpose(1, 2)]
    return res


def autograd_reference(q, k, v, key_mask, scale, W, softcap, go):
    """the same five tensors with the gradients from autograd through `forward`"""
    qr, kr, vr = (t.detach().double().requires_grad_(True) for t in (q, k, v))
    out, lse, _, _ = forward(qr, kr, vr, key_mask, scale, W, softcap)
    out = out.transpose(1, 2)
    out.backward(go.double())
    return [out.detach(), lse.detach(), qr.grad.transpose(1, 2), kr.grad.transpose(1, 2), vr.grad.transpose(1, 2)]
