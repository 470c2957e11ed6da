"""The FP8 KV-cache rows of include/bayeformers_amd_kv8.h restated on the CPU on top of tests/fp8_rows_ref.py (the centred
FP8 rows with centre zero): what bf_kv8_append / bf_kv8_dequantize must produce bit for bit, and a float64 reference of the
decode attention with a fill, a window and a soft-cap.  Not a test module."""
import torch

from fp8_rows_ref import dequantize_rows, quantize_rows


def quantize(x: torch.Tensor):
    """x [..., D] bf16 -> (q [..., D] uint8 holding e4m3fn bytes, scale [...] fp32 = 2^e of the row's amax)."""
    assert x.dtype == torch.bfloat16
    D = x.shape[-1]
    rows = x.reshape(-1, D)
    q, scale = quantize_rows(rows[None], torch.zeros_like(rows))
    return q.reshape(x.shape), scale.reshape(x.shape[:-1])


def dequantize(q: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """float(q) * scale as bf16 (exact)."""
    D = q.shape[-1]
    rows = q.reshape(-1, D)
    out = dequantize_rows(rows[None], scale.reshape(1, -1), torch.zeros(rows.shape, dtype=torch.bfloat16, device=q.device))
    return out.reshape(q.shape)


def append(kq, vq, k_scale, v_scale, k, v, pos: int) -> None:
    """bf_kv8_append on CPU tensors, in place: rows k / v [N, Hkv, Tq, D] go to slots pos .. pos + Tq - 1; a slot outside
    [0, capacity) is skipped."""
    cap = kq.shape[2]
    for src, q, s in ((k, kq, k_scale), (v, vq, v_scale)):
        bytes_, scale = quantize(src.contiguous())
        for i in range(src.shape[2]):
            if 0 <= pos + i < cap:
                q[:, :, pos + i] = bytes_[:, :, i]
                s[:, :, pos + i] = scale[:, :, i]


def special_rows(D: int) -> torch.Tensor:
    """[4, D] bf16: all zero; one large entry among zeros; negatives only; magnitudes from amax down to 2^-20 amax."""
    g = torch.Generator().manual_seed(D)
    rows = torch.zeros(4, D)
    rows[1, D // 3] = 28672.0  # 1.75 * 2^14: a 4-bit significand, kept exactly
    rows[2] = -torch.rand(D, generator=g) - 0.25
    rows[3] = 1.5 * 2.0 ** -torch.linspace(0, 20, D) * torch.where(torch.rand(D, generator=g) < 0.5, -1.0, 1.0)
    return rows.to(torch.bfloat16)


def decode_reference(q, k, v, scale, kv_len=None, key_mask=None, window=None, softcap=None):
    """float64: q [N, H, Tq, D], k / v [N, Hkv, Tk, D] of which the first L = kv_len (default Tk) keys are filled; query i sees
    keys L - Tq + i - window + 1 .. L - Tq + i that key_mask [N, Tk] (additive) does not hide; soft-capped logits
    softcap * tanh(scale q.k / softcap).  Returns [N, Tq, H, D]; a query with no visible key gives 0."""
    N, H, Tq, D = q.shape
    Hkv, Tk = k.shape[1], k.shape[2]
    L = Tk if kv_len is None else int(kv_len)
    G = H // Hkv
    kk = k.double().repeat_interleave(G, 1)
    vv = v.double().repeat_interleave(G, 1)
    s = torch.matmul(q.double(), kk.transpose(-1, -2)) * scale
    if softcap is not None:
        s = softcap * torch.tanh(s / softcap)
    if key_mask is not None:
        s = s + key_mask.double()[:, None, None, :]
    i = torch.arange(Tq, device=q.device)[:, None]
    j = torch.arange(Tk, device=q.device)[None, :]
    hidden = j > L - Tq + i
    if window is not None:
        hidden = hidden | (j <= L - Tq + i - window)
    s = s.masked_fill(hidden, float("-inf"))
    m = s.amax(-1, keepdim=True)
    p = torch.where(torch.isinf(m), torch.zeros_like(s), torch.exp(s - m.clamp(min=-1e300)))
    l = p.sum(-1, keepdim=True)
    out = torch.matmul(p, vv) / torch.where(l > 0, l, torch.ones_like(l))
    return out.transpose(1, 2)
