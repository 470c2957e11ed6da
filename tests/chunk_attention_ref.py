"""float64 restatement of the cached-chunk attention contract (include/bayeformers_amd_chunk.h), for the tests.

Tq new queries against Tk cached keys, bottom-right aligned at the fill L (kv_len, default Tk): query i has position
p_i = L - Tq + i and sees the keys max(0, p_i - W + 1) .. p_i the additive key mask leaves visible; keys at or past L are
never looked at (they may hold NaN); a query with no visible key gives 0; the soft-cap comes before the mask."""
import torch


def chunk_visible(Tq, Tk, kv_len=None, window=None, device="cpu"):
    """[Tq, Tk] bool: key j is inside query i's causal range (and window), before any key mask."""
    L = Tk if kv_len is None else max(0, min(int(kv_len), Tk))
    p = L - Tq + torch.arange(Tq, device=device)[:, None]
    j = torch.arange(Tk, device=device)[None, :]
    seen = (j <= p) & (j < L)
    if window is not None:
        seen = seen & (j > p - window)
    return seen


def chunk_reference(q, k, v, scale, kv_len=None, key_mask=None, window=None, softcap=None):
    """q [N, H, Tq, D], k / v [N, Hkv, Tk, D] (any float dtype) -> float64 [N, Tq, H, D]."""
    N, H, Tq, D = q.shape
    Hkv, Tk = k.shape[1], k.shape[2]
    L = Tk if kv_len is None else max(0, min(int(kv_len), Tk))
    out = torch.zeros(N, Tq, H, D, dtype=torch.float64, device=q.device)
    if L == 0:
        return out
    kk = k[:, :, :L].double().repeat_interleave(H // Hkv, 1)  # the slots past the fill are not touched
    vv = v[:, :, :L].double().repeat_interleave(H // Hkv, 1)
    s = torch.matmul(q.double(), kk.transpose(-1, -2)) * scale
    if softcap is not None:
        s = softcap * torch.tanh(s / softcap)
    if key_mask is not None:
        s = s + key_mask[:, :L].double()[:, None, None, :]
    seen = chunk_visible(Tq, Tk, L, window, q.device)[:, :L]
    s = s.masked_fill(~seen[None, None], float("-inf"))
    m = s.amax(-1, keepdim=True)
    p = torch.where(torch.isinf(m), torch.zeros_like(s), torch.exp(s - m.clamp(min=-1e300)))
    l = p.sum(-1, keepdim=True)
    return (torch.matmul(p, vv) / torch.where(l > 0, l, torch.ones_like(l))).transpose(1, 2).contiguous()


def dense_reference(q, k, v, scale, allowed, softcap=None):
    """The same function from a dense [N, 1 or H, Tq, Tk] bool mask (True = visible) by a plain masked softmax — what the
    framework's attention computes over _padding_mask_interface's mask; rows with nothing visible give 0."""
    H, Hkv = q.shape[1], k.shape[1]
    kk = k.double().repeat_interleave(H // Hkv, 1)
    vv = v.double().repeat_interleave(H // Hkv, 1)
    s = torch.matmul(q.double(), kk.transpose(-1, -2)) * scale
    if softcap is not None:
        s = softcap * torch.tanh(s / softcap)
    s = s.masked_fill(~allowed, float("-inf"))
    none = ~allowed.any(-1, keepdim=True)
    p = torch.softmax(s.masked_fill(none, 0.0), -1).masked_fill(none, 0.0)
    return torch.matmul(p, vv).transpose(1, 2).contiguous()
