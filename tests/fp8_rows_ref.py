"""The centred FP8 row format of include/bayeformers_amd_fp8.h restated in plain torch on the CPU: what
bf_fp8_rows_quantize / bf_fp8_rows_dequantize must produce bit for bit.  Not a test module."""
import torch

E4M3_MAX = 448.0
EXP_CLAMP = 64


def row_exponent(amax: torch.Tensor) -> torch.Tensor:
    """int32 e per row: the smallest integer with amax * 2^-e <= 448 (amax = m 2^x, m in [0.5, 1): x - 9 if m <= 0.875, else
    x - 8), 0 where amax = 0, clamped to [-64, 64]."""
    m, x = torch.frexp(amax.to(torch.float32))
    e = torch.where(m <= 0.875, x - 9, x - 8)
    e = torch.where(amax == 0, torch.zeros_like(e), e)
    return e.clamp(-EXP_CLAMP, EXP_CLAMP).to(torch.int32)


def quantize_rows(w16: torch.Tensor, center16: torch.Tensor):
    """w16 [S, N, K] bf16, center16 [N, K] bf16 -> (q [S, N, K] uint8 holding e4m3fn bytes, scale [S, N] fp32 = 2^e)."""
    assert w16.dtype == torch.bfloat16 and center16.dtype == torch.bfloat16
    d = w16.float() - center16.float()[None]
    e = row_exponent(d.abs().amax(dim=-1))
    one = torch.ones((), dtype=torch.float32)
    scale = torch.ldexp(one, e)
    arg = (d * torch.ldexp(one, -e)[..., None]).clamp(-E4M3_MAX, E4M3_MAX)  # the product is exact; the clamp acts only at |e| = 64
    assert float(arg.abs().max()) <= E4M3_MAX
    q = arg.to(torch.float8_e4m3fn).view(torch.uint8)
    return q, scale


def dequantize_rows(q: torch.Tensor, scale: torch.Tensor, center16: torch.Tensor) -> torch.Tensor:
    """W^ = bf16_rne(fp32(float(q) * scale + float(center16))): the product is exact, one fp32 and one bf16 rounding."""
    v = q.view(torch.float8_e4m3fn).float() * scale[..., None] + center16.float()[None]
    return v.to(torch.bfloat16)
