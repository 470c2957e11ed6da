"""A numpy restatement of bf_probs_truncate's contract (include/bayeformers_amd.h): the kept set by thresholds on the
values, the fixed-point top-p mass, the kept argmax and the rows copied through."""
import math

import numpy as np


def truncate_ref(probs, top_k=None, top_p=None, min_p=None):
    """The expected output of bf_probs_truncate for fp32 rows probs [R, V] (None: the criterion is off)."""
    probs = np.ascontiguousarray(probs, dtype=np.float32)
    out = np.zeros_like(probs)
    V = probs.shape[1]
    for r, p in enumerate(probs):
        if not np.isfinite(p).all() or not (p > 0).any():
            out[r] = p
            continue
        keep = p > 0
        mx = p.max()
        if top_k is not None and 0 < top_k < V:
            keep &= p >= np.sort(p)[::-1][top_k - 1]
        if top_p is not None and float(np.float32(top_p)) < 1.0:
            m, e = math.frexp(float(mx))
            E = e - 1 if m == 0.5 else e
            q = np.floor(np.ldexp(p.astype(np.float64), 40 - E)).astype(np.uint64)
            v = p[keep]
            order = np.argsort(-v, kind="stable")
            cum = np.cumsum(q[keep][order], dtype=np.uint64)
            total = int(cum[-1])
            need = min(max(math.ceil(float(np.float32(top_p)) * float(total)), 1), total)
            keep &= p >= v[order][int(np.searchsorted(cum, np.uint64(need)))]
        if min_p is not None and min_p > 0:
            keep &= p >= np.float32(np.float32(min_p) * mx)
        keep |= p == mx
        out[r] = np.where(keep, p, np.float32(0))
    return out


def softmax_rows(logits):
    x = np.asarray(logits, dtype=np.float64)
    e = np.exp(x - x.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(np.float32)
