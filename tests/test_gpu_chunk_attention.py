"""bf_attention_chunk_gqa / bf_attention_chunk_gqa_kv8 (csrc/bf_attention_chunk.hip) against the float64 restatement of
tests/chunk_attention_ref.py: offsets that are aligned to no tile, query tails, fills below the capacity read from the
device, windows, the soft-cap, padding masks, HF's strided projections; keys past the fill are never read; the FP8 form
is bitwise the 16-bit form on the dequantised cache; launches are deterministic and capturable.

The error bound is TOL of tests/test_gpu_decode_attention.py (bf16 9.1e-3, fp16 1.2e-3) on that file's inputs (standard
normal q, k, v), asserted per element as |out - ref| <= TOL * max(1, |ref|): the plain absolute error wherever |ref| <= 1,
scaled with the output's own ulp above that.  A row with few visible keys (the first rows of a first chunk, a short window)
is nearly a row of v, so outputs here reach |ref| of 3.6 - 4.5, where the correctly rounded reference itself is up to half
an ulp off (7.8e-3 at 2 <= |ref| < 4, 1.6e-2 from 4 on, in bf16): no 16-bit output can hold 9.1e-3 absolute there.
Measured on the MI355X over the cases below: the asserted figure at most 6.6e-3 in bf16 and 8.1e-4 in fp16; the plain
max |out - ref| 8.7e-3 .. 1.07e-2 in bf16 and 1.1e-3 .. 1.8e-3 in fp16, where the correctly rounded reference alone
is 7.8e-3 .. 8.6e-3 and 9.8e-4 .. 1.8e-3 off.  The test prints that floor beside the measured figures, and test_a_chunk_rounds_as_its_rows_of_the_whole_sequence_forward
holds bf_attention_fwd_gqa to the same bound on the same rows, where the two kernels agree bit for bit.

Only valid arguments reach the device: every kv_len below lies in [Tq, Tk]."""
import pytest
import torch

from chunk_attention_ref import chunk_reference
from test_gpu_decode_attention import TOL

pytestmark = pytest.mark.gpu

TQS = [17, 128, 129, 200]   # below a tile, a tile, a tile and a row, two tiles with a tail
OFFS = [0, 5, 127, 130]     # the first chunk; an unaligned diagonal; just below and just above a tile
WINDOWS = [None, 40, 150]   # below and above a key tile
CAPS = [None, 30.0]
SPARE = 37                  # capacity slots past the fill in the kv_len cases


def _qkv(N, H, Hkv, Tq, Tk, D, dtype, gen, static):
    """q as HF's transposed projection; k / v as HF's transposed projections too, or (static) a contiguous cache."""
    q = torch.randn(N, Tq, H, D, generator=gen, device="cuda").to(dtype).transpose(1, 2)
    if static:
        k = torch.randn(N, Hkv, Tk, D, generator=gen, device="cuda").to(dtype)
        v = torch.randn(N, Hkv, Tk, D, generator=gen, device="cuda").to(dtype)
    else:
        k = torch.randn(N, Tk, Hkv, D, generator=gen, device="cuda").to(dtype).transpose(1, 2)
        v = torch.randn(N, Tk, Hkv, D, generator=gen, device="cuda").to(dtype).transpose(1, 2)
    return q, k, v


def _padding(N, Tk, L, off):
    """Left padding: row 0 hides its first keys, the last row everything up to the fill — its chunk sees nothing."""
    m = torch.zeros(N, Tk, device="cuda")
    m[0, : off // 2 + 3] = float("-inf")
    m[N - 1, :L] = float("-inf")
    return m


def _err(out, ref):
    """(max over the elements of |out - ref| / max(1, |ref|), max |out - ref|): the first is what TOL bounds."""
    d = (out.double() - ref).abs()
    return (d / ref.abs().clamp(min=1.0)).max().item(), d.max().item()


def _floor(ref, dtype):
    """max |round(ref) - ref|: the error of the correctly rounded reference, which no kernel's output can beat."""
    return (ref.to(dtype).double() - ref).abs().max().item()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("D", [64, 128, 256])
@pytest.mark.parametrize("H,Hkv", [(4, 1), (4, 4)])
def test_chunk_matches_float64(dtype, D, H, Hkv):
    from bayeformers_amd import ops

    gen = torch.Generator(device="cuda").manual_seed(100 * H + 10 * Hkv + D)
    N, scale = 2, D ** -0.5
    calls, worst, worst_abs, floor, top = dict(ops.CHUNK_CALLS), 0.0, 0.0, 0.0, 0.0
    for Tq in TQS:
        for off in OFFS:
            L = off + Tq
            for static in (False, True):
                Tk = L + SPARE if static else L
                q, k, v = _qkv(N, H, Hkv, Tq, Tk, D, dtype, gen, static)
                kv_len = torch.tensor([L], device="cuda") if static else None
                assert ops.attention_chunk_supported(q, k, v)
                for padded in (False, True):
                    m = _padding(N, Tk, L, off) if padded else None
                    for W in WINDOWS:
                        for cap in CAPS:
                            out = ops.attention_forward_chunk(q, k, v, kv_len, m, scale, window=W, softcap=cap)
                            ref = chunk_reference(q, k, v, scale, kv_len=L, key_mask=m, window=W, softcap=cap)
                            assert out.shape == (N, Tq, H, D) and out.is_contiguous() and out.dtype == dtype
                            assert torch.isfinite(out).all()
                            if padded:
                                assert torch.equal(out[N - 1], torch.zeros_like(out[N - 1]))  # no visible key: exactly 0
                            rel, ab = _err(out, ref)
                            worst, worst_abs = max(worst, rel), max(worst_abs, ab)
                            floor, top = max(floor, _floor(ref, dtype)), max(top, ref.abs().max().item())
                            assert rel < TOL[dtype], (Tq, off, static, padded, W, cap, rel, ab)
    print(f"chunk {dtype} D={D} H={H} Hkv={Hkv}: max |err| / max(1, |ref|) = {worst:.3e} (bound {TOL[dtype]:.1e}), "
          f"max |err| = {worst_abs:.3e}, of the correctly rounded reference {floor:.3e}, max |ref| = {top:.2f}")
    assert ops.CHUNK_CALLS["fwd"] - calls["fwd"] == len(TQS) * len(OFFS) * 2 * 2 * len(WINDOWS) * len(CAPS)


def _fp8_cache(k, v):
    """k / v [N, Hkv, Tk, D] bf16 quantised by bf_kv8_append into a fresh cache of their size."""
    from bayeformers_amd import ops

    N, Hkv, Tk, D = k.shape
    kq, vq = (torch.zeros(N, Hkv, Tk, D, dtype=torch.uint8, device="cuda") for _ in range(2))
    ks, vs = (torch.zeros(N, Hkv, Tk, device="cuda") for _ in range(2))
    ops.kv8_append(k, v, kq, vq, ks, vs, torch.zeros(1, dtype=torch.long, device="cuda"))
    return kq, vq, ks, vs


@pytest.mark.parametrize("D", [64, 128, 256])
@pytest.mark.parametrize("H,Hkv", [(4, 1), (4, 2)])
def test_kv8_chunk_is_bitwise_the_16_bit_form_on_the_dequantised_cache(D, H, Hkv):
    from bayeformers_amd import ops

    gen = torch.Generator(device="cuda").manual_seed(D + H)
    N, scale = 2, D ** -0.5
    calls = dict(ops.CHUNK_CALLS)
    n = 0
    for Tq, off in ((17, 5), (129, 127), (200, 130), (128, 0)):
        L = off + Tq
        Tk = L + SPARE
        q, k, v = _qkv(N, H, Hkv, Tq, Tk, D, torch.bfloat16, gen, True)
        kq, vq, ks, vs = _fp8_cache(k, v)
        assert ops.attention_chunk_kv8_supported(q, kq, vq)
        kd, vd = ops.kv8_dequantize(kq, ks), ops.kv8_dequantize(vq, vs)
        kv_len = torch.tensor([L], device="cuda")
        m = _padding(N, Tk, L, off)
        for mask, W, cap in ((None, None, None), (m, 40, None), (m, 150, 30.0), (None, None, 30.0)):
            a = ops.attention_forward_chunk_kv8(q, kq, vq, ks, vs, kv_len, mask, scale, window=W, softcap=cap)
            b = ops.attention_forward_chunk(q, kd, vd, kv_len, mask, scale, window=W, softcap=cap)
            assert torch.equal(a, b), (Tq, off, W, cap)
            ref = chunk_reference(q, kd, vd, scale, kv_len=L, key_mask=mask, window=W, softcap=cap)
            assert _err(a, ref)[0] < TOL[torch.bfloat16]
            n += 1
    assert ops.CHUNK_CALLS["kv8"] - calls["kv8"] == n and ops.CHUNK_CALLS["fwd"] - calls["fwd"] == n


@pytest.mark.parametrize("D", [64, 256])
def test_keys_past_the_fill_are_never_read(D):
    from bayeformers_amd import ops

    gen = torch.Generator(device="cuda").manual_seed(3 * D)
    N, H, Hkv, Tq, off, scale = 2, 4, 2, 129, 127, D ** -0.5
    L = off + Tq
    q, k, v = _qkv(N, H, Hkv, Tq, L + SPARE, D, torch.bfloat16, gen, True)
    kq, vq, ks, vs = _fp8_cache(k, v)
    kv_len = torch.tensor([L], device="cuda")
    for W, cap in ((None, None), (150, 30.0)):
        exact = ops.attention_forward_chunk(q, k[:, :, :L], v[:, :, :L], None, None, scale, window=W, softcap=cap)  # Tk = L
        exact8 = ops.attention_forward_chunk_kv8(q, kq[:, :, :L], vq[:, :, :L], ks[:, :, :L].contiguous(),
                                                 vs[:, :, :L].contiguous(), None, None, scale, window=W, softcap=cap)
        kn, vn = k.clone(), v.clone()
        kn[:, :, L:] = float("nan")
        vn[:, :, L:] = float("nan")
        ksn, vsn = ks.clone(), vs.clone()
        ksn[:, :, L:] = float("nan")
        vsn[:, :, L:] = float("nan")
        out = ops.attention_forward_chunk(q, kn, vn, kv_len, None, scale, window=W, softcap=cap)
        out8 = ops.attention_forward_chunk_kv8(q, kq, vq, ksn, vsn, kv_len, None, scale, window=W, softcap=cap)
        assert torch.isfinite(out).all() and torch.equal(out, exact)
        assert torch.isfinite(out8).all() and torch.equal(out8, exact8)


def test_two_launches_are_bitwise_equal_and_a_captured_one_follows_the_fill():
    from bayeformers_amd import ops

    gen = torch.Generator(device="cuda").manual_seed(11)
    N, H, Hkv, Tq, D, Tk, scale = 2, 4, 2, 200, 128, 600, 128 ** -0.5
    q, k, v = _qkv(N, H, Hkv, Tq, Tk, D, torch.bfloat16, gen, True)
    m = _padding(N, Tk, 0, 6)
    kv_len = torch.tensor([330], device="cuda")
    a = ops.attention_forward_chunk(q, k, v, kv_len, m, scale, window=150)
    b = ops.attention_forward_chunk(q, k, v, kv_len, m, scale, window=150)
    assert torch.equal(a, b)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.attention_forward_chunk(q, k, v, kv_len, m, scale, window=150)
    for L in (330, 200, 600, 457):
        kv_len.fill_(L)  # in place: the captured launch reads it on the device
        graph.replay()
        eager = ops.attention_forward_chunk(q, k, v, kv_len, m, scale, window=150)
        assert torch.equal(out, eager), L
        ref = chunk_reference(q, k, v, scale, kv_len=L, key_mask=m, window=150)
        assert _err(out, ref)[0] < TOL[torch.bfloat16], L


@pytest.mark.parametrize("D", [64, 128, 256])
@pytest.mark.parametrize("W,cap", [(48, None), (100, 30.0), (None, None)])
def test_a_chunk_rounds_as_its_rows_of_the_whole_sequence_forward(D, W, cap):
    """key_origin lays the key tiles on the sequence's tile grid: a span's rows are BITWISE the same rows of
    bf_attention_fwd_gqa over the whole sequence — from the whole cache (origin 0), and from a cache that kept the last
    W - 1 keys before the span (origin = the keys dropped), at origins that are multiples of no tile; and origin changes
    nothing beyond rounding (fp64 reference)."""
    from bayeformers_amd import ops

    gen = torch.Generator(device="cuda").manual_seed(D + (W or 0))
    N, H, Hkv, T, scale = 2, 4, 2, 300, D ** -0.5
    q, k, v = _qkv(N, H, Hkv, T, T, D, torch.bfloat16, gen, False)
    m = torch.zeros(N, T, device="cuda")
    m[1, :20] = float("-inf")  # left padding
    whole = ops.attention_forward_gqa(q, k, v, m, scale, True, window=W, softcap=cap)
    whole_ref = chunk_reference(q, k, v, scale, key_mask=m, window=W, softcap=cap)  # (Tq = Tk: the cache-free sequence)
    rel, ab = _err(whole, whole_ref)
    print(f"bf_attention_fwd_gqa D={D} W={W} cap={cap}: max |err| / max(1, |ref|) = {rel:.3e}, max |err| = {ab:.3e}, "
          f"of the correctly rounded reference {_floor(whole_ref, torch.bfloat16):.3e}")
    assert rel < TOL[torch.bfloat16]  # the existing forward, held to the bound the chunk kernel is held to
    for a, b in ((64, 128), (128, 150), (150, 279), (279, 300), (0, 17)):
        rows = whole[:, a:b]
        full = ops.attention_forward_chunk(q[:, :, a:b], k[:, :, :b], v[:, :, :b], None, m[:, :b].contiguous(), scale,
                                           window=W, softcap=cap)
        assert torch.equal(full, rows), (a, b, "origin 0")
        assert _err(full, whole_ref[:, a:b]) == _err(rows, whole_ref[:, a:b])  # ... and so the same error figures
        if W is None:  # (nothing is dropped without a window)
            continue
        origin = max(a - W + 1, 0)  # what a sliding-window cache kept before the span: its last W - 1 keys
        ref = chunk_reference(q[:, :, a:b], k[:, :, :b], v[:, :, :b], scale, key_mask=m[:, :b], window=W, softcap=cap)
        km = m[:, origin:b].contiguous()
        cut = ops.attention_forward_chunk(q[:, :, a:b], k[:, :, origin:b], v[:, :, origin:b], None, km, scale, window=W,
                                          softcap=cap, key_origin=origin)
        assert torch.equal(cut, rows), (a, b, origin)
        assert _err(cut, ref)[0] < TOL[torch.bfloat16], (a, b, origin)
        unaligned = ops.attention_forward_chunk(q[:, :, a:b], k[:, :, origin:b], v[:, :, origin:b], None, km, scale,
                                                window=W, softcap=cap)
        assert _err(unaligned, ref)[0] < TOL[torch.bfloat16]  # (without the origin: right, rounded another way)
