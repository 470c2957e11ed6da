"""The row-subset kernels behind the narrow last encoder layer of pooled-head models, each on its own:
bf_gemm_nt_rows (strided rows of x) against float64, bf_attention_fwd_rows bit for bit against the same rows of
bf_attention_fwd, bf_add_layernorm_rows bit for bit against bf_add_layernorm on gathered rows."""
import numpy as np
import pytest
import torch

from bayeformers_amd import _C, ops

pytestmark = pytest.mark.gpu

# tests/test_gpu_kept_weights.py's bound for the same kernel: relative to max |ref|, one rounding of the 16-bit output
# (2^-9 for bf16's 8 significant bits, 2^-12 for fp16's 11) doubled, plus fp32 accumulation noise over K
TOL = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
BAND = 4096
MARK16 = 0x7FC1  # a NaN in bf16 and in fp16


def _gelu64(v):
    return 0.5 * v * (1.0 + torch.erf(v / np.sqrt(2.0)))


class Guarded:
    """n 16-bit elements between two bands of NaN-pattern words."""

    def __init__(self, n, dtype):
        self.n = n
        self.buf = torch.full((n + 2 * BAND,), MARK16, dtype=torch.int16, device="cuda")
        self.t = self.buf[BAND:BAND + n].view(dtype)

    def intact(self):
        return bool((self.buf[:BAND] == MARK16).all()) and bool((self.buf[BAND + self.n:] == MARK16).all())


@pytest.mark.parametrize("act", [0, 1], ids=["plain", "gelu"])
@pytest.mark.parametrize("N", [768, 3072])
@pytest.mark.parametrize("L", [128, 384])
@pytest.mark.parametrize("M", [1, 17, 32, 64])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_strided_rows_gemm_against_float64(dt, M, L, N, act):
    """Rows m * L of a [S, M*L, K] activation (row stride L*K) times W_s^T, + bias, optional GELU, into a banded output."""
    S = 3
    K = 3072 if N == 768 else 768  # the two feed-forward shapes of BERT-base (N 768 / K 3072 splits K)
    g = torch.Generator(device="cuda").manual_seed(M * 7919 + L * 31 + N + act)
    x = torch.randn(S, M * L, K, device="cuda", generator=g).to(dt)
    w = (torch.randn(S, N, K, device="cuda", generator=g) * K ** -0.5).to(dt)
    bias = torch.randn(S, N, device="cuda", generator=g)
    out = Guarded(S * M * N, dt)
    y = ops.gemm_nt_rows(x, w, bias, S, M, N, K, M * L * K, L * K, act, out=out.t.view(S * M, N))
    torch.cuda.synchronize()
    assert out.intact(), "the guard bands around y were written"
    rows = x[:, ::L].double()
    assert rows.shape == (S, M, K)
    ref = torch.einsum("smk,snk->smn", rows, w.double()) + bias[:, None, :].double()
    ref = _gelu64(ref) if act else ref
    err = (y.view(S, M, N).double() - ref).abs().max().item()
    bound = TOL[dt] * ref.abs().max().item() + 1e-5 * np.sqrt(K)
    print(f"[rows gemm {dt} M={M} L={L} N={N} K={K} act={act}] max err {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    # the same rows gathered into a compact tensor, through the same entry at row stride K: the same bits
    y2 = ops.gemm_nt_rows(x[:, ::L].contiguous(), w, bias, S, M, N, K, M * K, K, act)
    assert torch.equal(y2, y)


def test_strided_rows_gemm_counts_as_a_tiled_launch_and_refuses_bad_strides():
    import ctypes

    lib = _C.lib()
    S, M, N, K, L = 2, 32, 768, 768, 128
    x = torch.randn(S, M * L, K, device="cuda").to(torch.bfloat16)
    w = torch.randn(S, N, K, device="cuda").to(torch.bfloat16)
    lib.bf_profile_reset()
    lib.bf_profile_enable(1)
    try:
        ops.gemm_nt_rows(x, w, None, S, M, N, K, M * L * K, L * K)
        torch.cuda.synchronize()
    finally:
        lib.bf_profile_enable(0)
    n, ms, work = ctypes.c_uint64(), ctypes.c_double(), ctypes.c_double()
    _C.check(lib.bf_profile_read(_C.BF_PROF_GEMM, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(work)), "bf_profile_read")
    lib.bf_profile_reset()
    assert n.value == 1 and work.value == 2.0 * S * M * N * K
    with pytest.raises(_C.BayeFormersAMDError):   # a row stride below K
        ops.gemm_nt_rows(x, w, None, S, M, N, K, M * L * K, K - 8)
    with pytest.raises(_C.BayeFormersAMDError):   # a sample stride that does not hold the rows
        ops.gemm_nt_rows(x, w, None, S, M, N, K, K, L * K)


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("T", [128, 256, 384])
@pytest.mark.parametrize("q_rows", [1, 4])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_rows_attention_is_bitwise_the_full_kernels_rows(dt, q_rows, T, masked):
    B, H, D = 6, 12, 64
    g = torch.Generator(device="cuda").manual_seed(T * 13 + q_rows + int(masked))
    q, k, v = (torch.randn(B, T, H * D, device="cuda", generator=g).to(dt).view(B, T, H, D).transpose(1, 2) for _ in range(3))
    mask = mask_off = None
    if masked:
        lens = torch.randint(T // 3, T + 1, (B,), generator=torch.Generator().manual_seed(T)).tolist()
        mask = torch.zeros(B, T, device="cuda")
        for b, n in enumerate(lens):
            mask[b, n:] = float("-inf")
        mask_off = torch.zeros(1, dtype=torch.bool, device="cuda")
    assert ops.attention_supported(q, k, v)
    full = ops.attention_forward(q, k, v, mask, D ** -0.5, mask_off)
    out = Guarded(B * q_rows * H * D, dt)
    rc = _C.lib().bf_attention_fwd_rows(q.data_ptr(), k.data_ptr(), v.data_ptr(), mask.data_ptr() if masked else None,
                                        mask_off.data_ptr() if masked else None, out.t.data_ptr(), ops._TORCH2BF[dt], B, T, H,
                                        D, H * D, q_rows, D ** -0.5, ops._stream_ptr())
    assert rc == 0, _C.lib().bf_last_error()
    torch.cuda.synchronize()
    assert out.intact(), "the guard bands around the compact output were written"
    assert torch.equal(out.t.view(B, q_rows, H, D), full[:, :q_rows])
    assert torch.equal(ops.attention_forward_rows(q, k, v, mask, D ** -0.5, mask_off, q_rows=q_rows), full[:, :q_rows])
    assert torch.isfinite(full[:, :q_rows].float()).all()


def test_rows_attention_refuses_what_it_does_not_take():
    B, T, H, D = 2, 128, 2, 64
    q, k, v = (torch.randn(B, T, H * D, device="cuda").to(torch.bfloat16).view(B, T, H, D).transpose(1, 2) for _ in range(3))
    for bad in (0, 17):
        with pytest.raises(_C.BayeFormersAMDError):
            ops.attention_forward_rows(q, k, v, None, 0.125, q_rows=bad)


@pytest.mark.parametrize("N", [768, 1024, 1536])
@pytest.mark.parametrize("L", [128, 384])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "fp16", "fp32"])
def test_strided_residual_layernorm_is_bitwise_the_compact_kernel(dt, L, N):
    rows = 37
    g = torch.Generator(device="cuda").manual_seed(L + N)
    x = torch.randn(rows, N, device="cuda", generator=g).to(dt)
    res = torch.randn(rows, L, N, device="cuda", generator=g).to(dt)
    gamma, beta = (torch.randn(N, device="cuda", generator=g) for _ in range(2))
    want = ops.add_layernorm(x, res[:, 0].contiguous(), gamma, beta, 1e-12)
    got = ops.add_layernorm_rows(x, res, L * N, gamma, beta, 1e-12)
    assert torch.equal(got, want)
    with pytest.raises(_C.BayeFormersAMDError):
        ops.add_layernorm_rows(x, res, N - 8, gamma, beta, 1e-12)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_strided_rows_gemm_on_the_tiled_kernel_against_float64(dt):
    """K % 32 != 0 is not the streaming kernel's: the generic tiled kernel reads the strided rows."""
    S, M, N, K, L = 3, 37, 200, 72, 5
    g = torch.Generator(device="cuda").manual_seed(K)
    x = torch.randn(S, M * L, K, device="cuda", generator=g).to(dt)
    w = (torch.randn(S, N, K, device="cuda", generator=g) * K ** -0.5).to(dt)
    bias = torch.randn(S, N, device="cuda", generator=g)
    out = Guarded(S * M * N, dt)
    y = ops.gemm_nt_rows(x, w, bias, S, M, N, K, M * L * K, L * K, 0, out=out.t.view(S * M, N))
    torch.cuda.synchronize()
    assert out.intact()
    ref = torch.einsum("smk,snk->smn", x[:, ::L].double(), w.double()) + bias[:, None, :].double()
    err = (y.view(S, M, N).double() - ref).abs().max().item()
    assert err <= TOL[dt] * ref.abs().max().item() + 1e-5 * np.sqrt(K)
    assert torch.equal(y, ops.gemm_nt(x[:, ::L].contiguous(), w, bias, S, M, N, K, M * K, dt).view(S * M, N))


def test_streaming_shape_without_its_workspace_is_an_error():
    """N 768 / K 3072 at S 3 splits K: the launch needs scratch, and without it fails instead of running the tiled kernel."""
    lib = _C.lib()
    S, M, N, K = 3, 32, 768, 3072
    dt = _C.BF_DT_BF16
    assert lib.bf_gemm_nt_rows_workspace_bytes(dt, S, M, N, K) > 0
    assert lib.bf_gemm_nt_rows_workspace_bytes(dt, S, M, N, K + 8) == 0 and lib.bf_gemm_nt_rows_workspace_bytes(dt, S, 65, N, K) == 0
    x = torch.zeros(S, M, K, device="cuda", dtype=torch.bfloat16)
    w = torch.zeros(S, N, K, device="cuda", dtype=torch.bfloat16)
    out = Guarded(S * M * N, torch.bfloat16)
    rc = lib.bf_gemm_nt_rows(x.data_ptr(), dt, M * K, K, w.data_ptr(), dt, None, out.t.data_ptr(), dt, S, M, N, K, 0, None, 0,
                             ops._stream_ptr())
    torch.cuda.synchronize()
    assert rc == 1 and b"workspace" in lib.bf_last_error()
    assert bool((out.buf == MARK16).all())
