"""The two epilogues of the five-slot-ring GEMM (full-tile path and general path) through ops.gemm_nt / ops.gemm_nt_layers.

Small shapes: S = 2 and K = 128 (the ring kernel's minimum) keep every case at a few launches of a fraction of a millisecond.
The shapes M x N cover: tiles that are full in both directions (256 x 256), partial rows (288, 300, 513), full and partial N
tiles in one launch (320), a partial N tile alone with N % 64 != 0 (200) and the scalar tail of N % 8 != 0 (204).  With two
samples the schedule gives each of these columns tiles of 4 or 5 units only (M = 300 and 513 end in a ragged one) and one tile
per workgroup: they exercise the general path and the H = 4 / 5 instantiations of the full-tile path, not the heights the
BERT-base step runs.

Tall shapes (TALL): enough 256-column tiles for more than one round of the persistent kernel — a workgroup's second tile
DMAs into the LDS slot its first epilogue used — and, between them, FULL tiles of every template height 4 ... 8.  That is not
taken on trust: test_tall_shapes_cover_every_tile_height_and_several_rounds reads it off the host schedule (bf_gemm_schedule)
for the device's CU count and fails if a change of the schedule policy takes a height or the second round away.  One of them
is the attention-out launch of the BERT-base step itself (S = 10, M = 4096, N = 768: heights 7 and 8).  They are the smallest
of their kind: a round is one tile of >= 128 x 256 outputs on each of 256 CUs.

Exact cases: operands and bias are integers of magnitude <= 3, so every product and every fp32 partial sum (|sum| <=
128 * 9 + 3) is exact whatever the order of accumulation, and the one rounding is the conversion of the fp32 result to
bf16 / fp16.  The expected output is the float64 product rounded the same way on the CPU (the float64 -> fp32 step is exact
for these integers), and the comparison is bit for bit.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from bayeformers_amd import _C, ops

pytestmark = pytest.mark.gpu

S, K = 2, 128
MS = [256, 288, 300, 513]
NS = [256, 320, 200, 204]
DTYPES = [torch.bfloat16, torch.float16]
NAN_BITS = 0x7FC1   # a quiet NaN with a payload, in bf16 and in fp16
GUARD = 1024        # elements before and after the window
TALL = [(10, 1, 4096, 768), (2, 3, 8192, 512), (2, 3, 4096, 768)]   # (S, L, M, N), see the module docstring


def _ints(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-3, 4, shape, generator=g).double()


def _bits(t):
    return t.contiguous().view(torch.int16)


def _exact_case(M, N, L, with_bias, dtype, S=S):
    """(x, w [L,S,N,K], bias [L,S,N] or None, expected [L,S,M,N] in dtype), operands on the GPU, expected on the CPU"""
    x = _ints((S, M, K), 1000 + M)
    w = _ints((L, S, N, K), 2000 + N + L)
    b = _ints((L, S, N), 3000 + N + L) if with_bias else None
    ref = torch.einsum("smk,lsnk->lsmn", x, w)
    if b is not None:
        ref = ref + b[:, :, None, :]
    expected = ref.float().to(dtype)
    return x.to(dtype).cuda(), w.to(dtype).cuda(), (b.float().cuda() if b is not None else None), expected


@functools.lru_cache(maxsize=None)
def _tall_reference(S, L, M, N):
    """the float64 product + bias of a tall shape, computed once for both dtypes (kept as fp32: exact for these integers)"""
    x = _ints((S, M, K), 1000 + M)
    w = _ints((L, S, N, K), 2000 + N + L)
    b = _ints((L, S, N), 3000 + N + L)
    ref = torch.einsum("smk,lsnk->lsmn", x, w) + b[:, :, None, :]
    return x, w, b, ref.float()


def _window(M, N, dtype, misalign=0, S=S):
    """a [S,M,N] window, 16-byte aligned (+ misalign elements), in a buffer filled with a NaN pattern"""
    buf = torch.empty(2 * GUARD + S * M * N + 8, dtype=torch.int16, device="cuda")
    buf.fill_(NAN_BITS)
    start = GUARD + misalign
    assert (buf.data_ptr() + 2 * GUARD) % 16 == 0
    out = buf[start:start + S * M * N].view(dtype).view(S, M, N)
    return buf, out, start


def _assert_bands(buf, start, n):
    assert bool((buf[:start] == NAN_BITS).all()), "the band before the window was written"
    assert bool((buf[start + n:] == NAN_BITS).all()), "the band after the window was written"


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("M", MS)
def test_exact_integer_products_bit_for_bit(M, N, dtype):
    for L in (1, 3):
        for with_bias in (False, True):
            x, w, b, expected = _exact_case(M, N, L, with_bias, dtype)
            want = _bits(expected.cuda())
            if L == 1:
                buf, out, start = _window(M, N, dtype)
                y = ops.gemm_nt(x, w[0], b[0] if with_bias else None, S, M, N, K, M * K, dtype, out=out)
                y2 = ops.gemm_nt(x, w[0], b[0] if with_bias else None, S, M, N, K, M * K, dtype)
                _assert_bands(buf, start, S * M * N)
                y, y2 = y[None], y2[None]
            else:
                y = ops.gemm_nt_layers(x, w, b, L, S, M, N, K, M * K, dtype)
                y2 = ops.gemm_nt_layers(x, w, b, L, S, M, N, K, M * K, dtype)
            bad = (_bits(y) != want)
            assert not bool(bad.any()), f"L={L} bias={with_bias}: {int(bad.sum())} of {bad.numel()} outputs differ from the fp64 product"
            assert torch.equal(_bits(y), _bits(y2)), f"L={L} bias={with_bias}: two launches differ"


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("M,N", [(256, 256), (513, 320), (300, 204)])
def test_window_two_bytes_off_alignment_takes_the_general_path(M, N, dtype):
    """`out` 2 bytes off a 16-byte boundary: no 16-byte store may be used; same bits, bands untouched"""
    x, w, b, expected = _exact_case(M, N, 1, True, dtype)
    buf, out, start = _window(M, N, dtype, misalign=1)
    assert out.data_ptr() % 16 == 2
    y = ops.gemm_nt(x, w[0], b[0], S, M, N, K, M * K, dtype, out=out)
    assert torch.equal(_bits(y), _bits(expected[0].cuda()))
    _assert_bands(buf, start, S * M * N)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("M", MS)
def test_fused_gelu_against_fp64(M, N, dtype):
    """act = 1 with random operands; the bound is test_gemm_fused_gelu's (tests/test_gpu_linear.py) for 16-bit outputs"""
    g = torch.Generator(device="cuda").manual_seed(7)
    for L in (1, 3):
        w = torch.randn(L, S, N, K, device="cuda", generator=g).to(dtype)
        x = torch.randn(S, M, K, device="cuda", generator=g).to(dtype)
        bias = torch.randn(L, S, N, device="cuda", generator=g)
        pre = torch.einsum("smk,lsnk->lsmn", x.double(), w.double()) + bias[:, :, None, :].double()
        ref = torch.nn.functional.gelu(pre)
        if L == 1:
            buf, out, start = _window(M, N, dtype)
            y = ops.gemm_nt(x, w[0], bias[0], S, M, N, K, M * K, dtype, act=1, out=out)[None]
            y2 = ops.gemm_nt(x, w[0], bias[0], S, M, N, K, M * K, dtype, act=1)[None]
            _assert_bands(buf, start, S * M * N)
        else:
            y = ops.gemm_nt_layers(x, w, bias, L, S, M, N, K, M * K, dtype, act=1)
            y2 = ops.gemm_nt_layers(x, w, bias, L, S, M, N, K, M * K, dtype, act=1)
        err = (y.double() - ref).abs().max().item()
        bound = 2.0 ** -8 * ref.abs().max().item() + 1e-5 * np.sqrt(K)
        assert err <= bound, f"L={L}: max |y - gelu(fp64)| = {err:.3e} > {bound:.3e}"
        assert torch.equal(_bits(y), _bits(y2)), f"L={L}: two launches differ"


def _schedule(S, L, M, N, n_cu):
    """the host-built tile schedule of a launch as (rounds, [(height in units, first row, n tile)] of its tiles)"""
    lib = _C.lib()
    r, g = ctypes.c_int(), ctypes.c_int()
    n = lib.bf_gemm_schedule(S, L, M, N, n_cu, None, 0, ctypes.byref(r), ctypes.byref(g))
    out = np.zeros(n, dtype=np.int32)
    assert lib.bf_gemm_schedule(S, L, M, N, n_cu, out.ctypes.data, n, ctypes.byref(r), ctypes.byref(g)) == n
    t = out.reshape(-1, 4)
    t = t[(t[:, 2] >> 24) > 0]
    return r.value, [(int(z) >> 24, int(m0), int(z) & 0xFFFFFF) for _, _, z, m0 in t]


def test_tall_shapes_cover_every_tile_height_and_several_rounds():
    """what the tall cases below are there for, read off the schedule the kernel will walk on this device"""
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    full_heights = set()
    for S_, L, M, N in TALL:
        rounds, tiles = _schedule(S_, L, M, N, n_cu)
        assert rounds > 1, f"{(S_, L, M, N)}: one round only, no workgroup runs a second tile"
        full = {h for h, m0, tn in tiles if h >= 4 and m0 + 32 * h <= M and (tn + 1) * 256 <= N}
        print(f"{(S_, L, M, N)}: {rounds} rounds, {len(tiles)} tiles, full-tile heights {sorted(full)}")
        full_heights |= full
    assert full_heights >= {4, 5, 6, 7, 8}, f"full tiles of heights {sorted(full_heights)} only"


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("S_,L,M,N", TALL)
def test_tall_exact_integer_products_bit_for_bit(S_, L, M, N, dtype):
    """full tiles of heights 4 ... 8 and second tiles of a workgroup: bit for bit, twice, under guard bands where `out=` exists"""
    x64, w64, b64, ref = _tall_reference(S_, L, M, N)
    x, w, b = x64.to(dtype).cuda(), w64.to(dtype).cuda(), b64.float().cuda()
    want = _bits(ref.to(dtype).cuda())
    if L == 1:
        buf, out, start = _window(M, N, dtype, S=S_)
        y = ops.gemm_nt(x, w[0], b[0], S_, M, N, K, M * K, dtype, out=out)[None]
        y2 = ops.gemm_nt(x, w[0], b[0], S_, M, N, K, M * K, dtype)[None]
        _assert_bands(buf, start, S_ * M * N)
    else:
        y = ops.gemm_nt_layers(x, w, b, L, S_, M, N, K, M * K, dtype)
        y2 = ops.gemm_nt_layers(x, w, b, L, S_, M, N, K, M * K, dtype)
    bad = (_bits(y) != want)
    assert not bool(bad.any()), f"{int(bad.sum())} of {bad.numel()} outputs differ from the fp64 product"
    assert torch.equal(_bits(y), _bits(y2)), "two launches differ"


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("S_,L,M,N", TALL)
def test_tall_fused_gelu_against_fp64(S_, L, M, N, dtype):
    """act = 1 on the tall shapes, random operands, test_gemm_fused_gelu's bound; two launches equal"""
    g = torch.Generator(device="cuda").manual_seed(11)
    w = torch.randn(L, S_, N, K, device="cuda", generator=g).to(dtype)
    x = torch.randn(S_, M, K, device="cuda", generator=g).to(dtype)
    bias = torch.randn(L, S_, N, device="cuda", generator=g)
    ref = torch.nn.functional.gelu(torch.einsum("smk,lsnk->lsmn", x.double(), w.double()) + bias[:, :, None, :].double())
    if L == 1:
        buf, out, start = _window(M, N, dtype, S=S_)
        y = ops.gemm_nt(x, w[0], bias[0], S_, M, N, K, M * K, dtype, act=1, out=out)[None]
        y2 = ops.gemm_nt(x, w[0], bias[0], S_, M, N, K, M * K, dtype, act=1)[None]
        _assert_bands(buf, start, S_ * M * N)
    else:
        y = ops.gemm_nt_layers(x, w, bias, L, S_, M, N, K, M * K, dtype, act=1)
        y2 = ops.gemm_nt_layers(x, w, bias, L, S_, M, N, K, M * K, dtype, act=1)
    err = (y.double() - ref).abs().max().item()
    bound = 2.0 ** -8 * ref.abs().max().item() + 1e-5 * np.sqrt(K)
    assert err <= bound, f"max |y - gelu(fp64)| = {err:.3e} > {bound:.3e}"
    assert torch.equal(_bits(y), _bits(y2)), "two launches differ"
