"""A float64 restatement of the encoder attention's contract (bf_attention_fwd / bf_attention_bwd and their _dropout
siblings, include/bayeformers_amd.h): plain torch, on whatever device the operands live, one slab of sequences and heads at a
time so that the [B, H, T, T] doubles of a large shape never exist at once.

    S  = scale q k^T + mask            P = softmax(S) over ALL keys (a query with no visible key: P = 0)
    P~ = P o keep / (1 - p)            out = P~ v            lse = log2 sum_k exp(S)  (+inf without a visible key)
    delta = sum_d go o out             dS = P o (keep / (1 - p) o (go v^T) - delta)
    dq = scale dS k                    dk = scale dS^T q     dv = P~^T go
"""
import math

import torch

LN2 = math.log(2.0)


class AttentionRef:
    """out [B, T, H, 64], lse [B, H, T] (log2 units) and, given go: delta [B, H, T], dq / dk / dv [B, T, H, 64]; float64."""

    def __init__(self):
        self.out = self.lse = self.delta = self.dq = self.dk = self.dv = None

    def colsum(self, S):
        """[3, S, H*64]: per sample (B / S consecutive sequences each) the sums over sequences and tokens of dq, dk, dv."""
        B, T, H, D = self.dq.shape
        assert B % S == 0
        return torch.stack([g.reshape(S, (B // S) * T, H * D).sum(1) for g in (self.dq, self.dk, self.dv)])


def _slab(q, k, v, mask, scale, keep, inv_keep, go):
    """One [b, h, T, D] slab, everything float64 already (keep: float64 0 / 1 or None)."""
    s = q @ k.transpose(-1, -2) * scale
    if mask is not None:
        s = s + mask[:, None, None, :]
    m = s.amax(-1, keepdim=True)
    valid = torch.isfinite(m)
    m = torch.where(valid, m, torch.zeros_like(m))
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    l1 = torch.where(valid, l, torch.ones_like(l))
    p = torch.where(valid, e / l1, torch.zeros_like(e))
    lse = torch.where(valid, (m + torch.log(l1)) / LN2, torch.full_like(m, float("inf")))[..., 0]
    pd = p if keep is None else p * keep * inv_keep
    out = pd @ v
    if go is None:
        return out, lse, None, None, None, None
    dpd = go @ v.transpose(-1, -2)
    delta = (go * out).sum(-1, keepdim=True)
    ds = p * ((dpd if keep is None else dpd * keep * inv_keep) - delta)
    return out, lse, delta[..., 0], scale * (ds @ k), scale * (ds.transpose(-1, -2) @ q), pd.transpose(-1, -2) @ go


def attention_ref(q, k, v, mask, scale, keep=None, p=0.0, go=None, chunk_bytes=1 << 28):
    """q, k, v: [B, H, T, D] in any strides and dtype; mask: additive [B, T] or None (-inf or finite entries); keep: the
    dropout keep mask [B, H, T, T] (0 / 1) with rate p — the factor 1 / (1 - p) is oracle.bayes_oracle.dropout_keep_scale's,
    the rate rounded to 16 bits as the kernels do; go: the output gradient [B, T, H, D] or None.  chunk_bytes bounds the
    size of one [b, h, T, T] double (None: one slab)."""
    B, H, T, D = q.shape
    inv_keep = 1.0
    if keep is not None:
        from oracle import bayes_oracle as bo

        inv_keep = float(bo.dropout_keep_scale(p))
    per_head = T * T * 8
    if chunk_bytes is None:
        nb, nh = B, H
    else:
        nh = max(1, min(H, chunk_bytes // per_head))
        nb = max(1, min(B, chunk_bytes // (per_head * nh))) if nh == H else 1
    r = AttentionRef()
    dev = q.device
    r.out = torch.empty(B, T, H, D, dtype=torch.float64, device=dev)
    r.lse = torch.empty(B, H, T, dtype=torch.float64, device=dev)
    if go is not None:
        r.delta = torch.empty(B, H, T, dtype=torch.float64, device=dev)
        r.dq, r.dk, r.dv = (torch.empty(B, T, H, D, dtype=torch.float64, device=dev) for _ in range(3))
    for b0 in range(0, B, nb):
        for h0 in range(0, H, nh):
            bs, hs = slice(b0, b0 + nb), slice(h0, h0 + nh)
            res = _slab(q[bs, hs].double(), k[bs, hs].double(), v[bs, hs].double(),
                        None if mask is None else mask[bs].double(), float(scale),
                        None if keep is None else keep[bs, hs].double(), inv_keep,
                        None if go is None else go[bs, :, hs].double().transpose(1, 2))
            r.out[bs, :, hs] = res[0].transpose(1, 2)
            r.lse[bs, hs] = res[1]
            if go is not None:
                r.delta[bs, hs] = res[2]
                for dst, src in zip((r.dq, r.dk, r.dv), res[3:]):
                    dst[bs, :, hs] = src.transpose(1, 2)
    return r
