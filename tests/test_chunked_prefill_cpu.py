"""Host side of sample_generate(prefill_chunk=...) (no GPU): the header and symbol table of the cached-chunk attention
entries, their refusals before any launch, the routing of a cached chunk with the switch off and on, the span helper, the
argument checks, and the float64 reference (tests/chunk_attention_ref.py) against a dense-mask softmax."""
import ctypes
import os
import re

import pytest
import torch

import bayeformers_amd as bf
from bayeformers_amd import _C, graphs, ops, sampling
from bayeformers_amd.sampling import _prefill_spans, sample_generate
from chunk_attention_ref import chunk_reference, chunk_visible, dense_reference
from kv8_ref import quantize
from test_kept_fp8_cpu import _c_type_class, _ctypes_class, _small_llama

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"bf_attention_chunk_gqa", "bf_attention_chunk_gqa_kv8"}
PTR = 4096  # an aligned non-NULL address: every call below is refused on its arguments, nothing is launched


@pytest.fixture(autouse=True)
def _switches_off_again():
    yield
    bf.chunked_attention(False)
    bf.softcap_attention(False)


# ---------------------------------------------------------------------------------------------------- header, bindings
def test_chunk_header_prototypes_match_the_ctypes_signatures():
    header = open(os.path.join(ROOT, "include", "bayeformers_amd_chunk.h")).read()
    assert '#include "bayeformers_amd.h"' in header
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    header = re.sub(r"^\s*#.*$", "", header, flags=re.M)
    parsed = {}
    for ret, name, params in re.findall(r"([A-Za-z_][A-Za-z0-9_ \t\n\*]*?)\b(bf_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", header):
        assert name not in parsed, name
        parsed[name] = (_c_type_class(ret), [_c_type_class(a.strip()) for a in params.split(",")])
    assert set(parsed) == set(_C.CHUNK_SYMBOLS) == ENTRIES
    for name, (res, args) in _C.CHUNK_SYMBOLS.items():
        c_res, c_args = parsed[name]
        assert _ctypes_class(res) == c_res and len(args) == len(c_args), name
        for i, (a, c) in enumerate(zip(args, c_args)):
            assert _ctypes_class(a) == c, (name, i, a, c)


def test_chunk_symbols_are_a_table_of_their_own():
    others = [_C.SYMBOLS, _C.SOFTCAP_SYMBOLS, _C.FAMILY_BLOCK_SYMBOLS, _C.FAMILY_BLOCK_BWD_SYMBOLS, _C.PACKED_SYMBOLS,
              _C.FP8_SYMBOLS, _C.KV8_SYMBOLS]
    for table in others:
        assert not set(_C.CHUNK_SYMBOLS) & set(table)
    assert len(_C.SYMBOLS) == 90 and _C.ABI_VERSION == 6
    main = open(os.path.join(ROOT, "include", "bayeformers_amd.h")).read()
    assert not any(name in main for name in ENTRIES)  # (the main header is as it was)


def test_chunk_symbols_resolve_in_the_built_library():
    lib = _C.lib()
    for name, (res, args) in _C.CHUNK_SYMBOLS.items():
        fn = getattr(lib, name)
        assert fn.restype is res and fn.argtypes == args
    assert lib.bf_version() == _C.ABI_VERSION


def test_a_library_without_the_chunk_entries_asks_for_a_rebuild(monkeypatch):
    class Old:
        def __getattr__(self, name):
            if name in _C.CHUNK_SYMBOLS:
                raise AttributeError(name)
            return getattr(real, name)

    real = ctypes.CDLL(_C.LIB_PATH)
    monkeypatch.setattr(_C, "_lib", None)
    monkeypatch.setattr(ctypes, "CDLL", lambda path: Old())
    with pytest.raises(_C.BayeFormersAMDError,
                       match=r"lacks bf_attention_chunk_gqa \(the cached-chunk attention entries\): rebuild"):
        _C.lib()


# ---------------------------------------------------------------------------------------------------- host refusals
def _shape(N=2, Tq=17, Tk=64, H=4, Hkv=2, D=64, q_stride=None, k_stride=None):
    s = _C.bf_attn_decode_t(N, Tq, Tk, H, Hkv, D)
    s.q_stride[:] = q_stride or [H * Tq * D, Tq * D, D]
    s.k_stride[:] = k_stride or [Hkv * Tk * D, Tk * D, D]
    s.v_stride[:] = [Hkv * Tk * D, Tk * D, D]
    return s


def _chunk(shape, q=PTR, k=PTR, out=PTR, mask=None, kv_len=None, dtype=_C.BF_DT_BF16, window=0, softcap=0.0, origin=0):
    lib = _C.lib()
    rc = lib.bf_attention_chunk_gqa(q, k, PTR, mask, None, kv_len, out, dtype, ctypes.byref(shape) if shape else None,
                                    window, origin, softcap, 0.125, None)
    return rc, lib.bf_last_error()


def _chunk8(shape, q=PTR, kq=PTR, ks=PTR, vs=PTR, kv_len=None, dtype=_C.BF_DT_BF16, window=0, softcap=0.0, origin=0):
    lib = _C.lib()
    rc = lib.bf_attention_chunk_gqa_kv8(q, kq, PTR, ks, vs, None, None, kv_len, PTR, dtype, ctypes.byref(shape), window,
                                        origin, softcap, 0.125, None)
    return rc, lib.bf_last_error()


@pytest.mark.parametrize("call,what", [(_chunk, b"bf_attention_chunk_gqa:"), (_chunk8, b"bf_attention_chunk_gqa_kv8:")],
                         ids=["16-bit", "kv8"])
def test_the_entries_refuse_before_any_launch(call, what):
    for kw, word in ((dict(D=96), b"head size 96"), (dict(H=4, Hkv=3), b"do not divide"), (dict(Tq=0), b"Tq=0"),
                     (dict(Tq=65, Tk=64), b"fewer than Tq=65"), (dict(N=70000), b"exceeds the grid"),
                     (dict(H=70000, Hkv=2), b"exceeds the grid"), (dict(N=0), b"must be positive"),
                     (dict(q_stride=[4 * 17 * 64, 17 * 64, 68]), b"multiples of 8")):
        rc, msg = call(_shape(**kw))
        assert rc == 1 and msg.startswith(what) and word in msg, (kw, msg)
    rc, msg = call(_shape(), window=-1)
    assert rc == 1 and b"window=-1" in msg
    rc, msg = call(_shape(), origin=-1)
    assert rc == 1 and b"key_origin=-1" in msg
    for cap in (-1.0, float("inf"), float("nan")):
        rc, msg = call(_shape(), softcap=cap)
        assert rc == 1 and b"softcap" in msg
    rc, msg = call(_shape(), softcap=1e-40)  # scaling / softcap overflows fp32
    assert rc == 1 and b"not finite" in msg
    rc, msg = call(_shape(), q=None)
    assert rc == 1 and b"NULL" in msg
    rc, msg = call(_shape(), q=PTR + 8)
    assert rc == 1 and b"16-byte aligned" in msg
    rc, msg = call(_shape(), kv_len=PTR + 4)
    assert rc == 1 and b"kv_len" in msg
    rc, msg = call(_shape(), dtype=_C.BF_DT_F32)
    assert rc == 1 and b"bf16" in msg


def test_the_entries_refuse_what_is_their_own():
    rc, msg = _chunk(None)
    assert rc == 1 and b"shape is NULL" in msg
    rc, msg = _chunk(_shape(), k=None)
    assert rc == 1 and b"NULL" in msg
    rc, msg = _chunk(_shape(), out=PTR + 2)
    assert rc == 1 and b"16-byte aligned" in msg
    rc, msg = _chunk(_shape(), mask=PTR + 2)
    assert rc == 1 and b"mask" in msg
    rc, msg = _chunk(_shape(k_stride=[2 * 64 * 64, 64 * 64 + 4, 64]))
    assert rc == 1 and b"multiples of 8" in msg
    assert _chunk(_shape(), dtype=_C.BF_DT_F16, q=None)[1].endswith(b"NULL argument")  # (fp16 is taken: refused on the pointer)
    rc, msg = _chunk8(_shape(), dtype=_C.BF_DT_F16)
    assert rc == 1 and b"bfloat16" in msg
    for kw in (dict(ks=None), dict(vs=None)):
        rc, msg = _chunk8(_shape(), **kw)
        assert rc == 1 and b"NULL scale" in msg
    rc, msg = _chunk8(_shape(), ks=PTR + 2)
    assert rc == 1 and b"4-byte aligned" in msg
    rc, msg = _chunk8(_shape(k_stride=[2 * 64 * 64 + 8, 64 * 64, 64]))  # fine for bf16 elements, not for bytes
    assert rc == 1 and b"multiples of 16" in msg


def test_the_ops_wrappers_check_their_arguments_on_the_host():
    calls = dict(ops.CHUNK_CALLS)
    q = torch.zeros(2, 4, 17, 64, dtype=torch.bfloat16)
    k = torch.zeros(2, 2, 40, 64, dtype=torch.bfloat16)
    kq = torch.zeros(2, 2, 40, 64, dtype=torch.uint8)
    sc = torch.zeros(2, 2, 40)
    for call in (lambda: ops.attention_forward_chunk(q, k, k, None, None, 0.125),
                 lambda: ops.attention_forward_chunk_kv8(q, kq, kq, sc, sc, None, None, 0.125)):
        with pytest.raises(_C.BayeFormersAMDError, match="ROCm|device"):
            call()
    assert not ops.attention_chunk_supported(q, k, k) and not ops.attention_chunk_kv8_supported(q, kq, kq)  # (not on the device)
    assert ops.attention_chunk_supported(q, k, k, check_device=False)
    assert ops.attention_chunk_supported(q.half(), k.half(), k.half(), check_device=False)
    assert ops.attention_chunk_supported(q[:, :, :1], k, k, check_device=False)  # any Tq >= 1: the routing picks the chunks
    assert not ops.attention_chunk_supported(q, k[:, :, :16], k[:, :, :16], check_device=False)  # Tq > Tk
    assert not ops.attention_chunk_supported(q.float(), k.float(), k.float(), check_device=False)
    assert not ops.attention_chunk_supported(q, k[:, :1].expand(2, 3, 40, 64), k[:, :1].expand(2, 3, 40, 64), check_device=False)
    assert ops.attention_chunk_kv8_supported(q, kq, kq, check_device=False)
    assert not ops.attention_chunk_kv8_supported(q.half(), kq, kq, check_device=False)
    assert not ops.attention_chunk_kv8_supported(q, k, k, check_device=False)
    k24 = torch.zeros(2, 2, 40, 72, dtype=torch.uint8)[..., :64]  # a token stride of 72 bytes
    assert not ops.attention_chunk_kv8_supported(q, k24, k24, check_device=False)
    assert set(ops.CHUNK_CALLS) == {"fwd", "kv8"} and ops.CHUNK_CALLS == calls  # (a refused call counts nothing)
    assert set(ops.KV8_CALLS) == {"append", "decode", "dequantize"} and set(ops.DECODE_CALLS) == {"fwd", "len", "window", "len_window"}


# ---------------------------------------------------------------------------------------------------- routing
@pytest.fixture
def launches(monkeypatch):
    """Pretend the chunk, decode and prefill entries apply to CPU tensors and record what each call was given."""
    seen = []
    for name in ("attention_chunk_supported", "attention_chunk_kv8_supported", "attention_decode_supported",
                 "attention_decode_kv8_supported"):
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda q, k, v, check_device=True, real=real: real(q, k, v, False))

    def zeros(q):
        return torch.zeros(q.shape[0], q.shape[2], q.shape[1], q.shape[3], dtype=q.dtype)

    def chunk(q, k, v, kv_len, key_mask, scaling, mask_off=None, window=None, softcap=None, key_origin=0):
        assert k.dtype == q.dtype
        seen.append(("chunk", kv_len is not None, window, softcap, None if key_mask is None else tuple(key_mask.shape))
                    + ((key_origin,) if key_origin else ()))
        return zeros(q)

    def chunk8(q, kq, vq, k_scale, v_scale, kv_len, key_mask, scaling, mask_off=None, window=None, softcap=None, key_origin=0):
        assert kq.dtype == torch.uint8 and k_scale is kq._bf_kv8_scale and v_scale is vq._bf_kv8_scale
        seen.append(("chunk_kv8", kv_len is not None, window, softcap, None if key_mask is None else tuple(key_mask.shape))
                    + ((key_origin,) if key_origin else ()))
        return zeros(q)

    def decode(name):
        def run(q, *a, **kw):
            seen.append((name,))
            return zeros(q)
        return run

    def deq(q, scale, out=None):
        seen.append(("dequantize",))
        return torch.zeros(q.shape, dtype=torch.bfloat16)

    import transformers.integrations.sdpa_attention as sa

    real_sdpa = sa.sdpa_attention_forward

    def sdpa(module, q, k, v, *a, **kw):
        assert k.dtype == q.dtype
        seen.append(("sdpa",))
        kw.pop("s_aux", None), kw.pop("softcap", None)
        return real_sdpa(module, q, k, v, *a, **kw)

    eager = bf._softcap_eager
    monkeypatch.setattr(bf, "_softcap_eager", lambda *a, **kw: seen.append(("softcap_eager",)) or eager(*a, **kw))
    monkeypatch.setattr(ops, "attention_forward_chunk", chunk)
    monkeypatch.setattr(ops, "attention_forward_chunk_kv8", chunk8)
    for name in ("attention_forward_decode", "attention_forward_decode_len", "attention_forward_decode_kv8"):
        monkeypatch.setattr(ops, name, decode(name))
    monkeypatch.setattr(ops, "kv8_dequantize", deq)
    monkeypatch.setattr(sa, "sdpa_attention_forward", sdpa)
    return seen


def _module():
    mod = torch.nn.Module()
    mod.is_causal = True
    mod.num_key_value_groups = 2
    return mod.eval()


def _call(Tq=17, Tk=40, fixed=False, W=None, pad=False, fp8=False, grad=False):
    """(q, k, v, mask) of a cached chunk: Tq new queries whose cache holds Tk keys after them (fixed: a capacity of Tk + 9)."""
    from transformers.masking_utils import causal_mask_function, sliding_window_causal_mask_function

    g = torch.Generator().manual_seed(0)
    cap = Tk + 9 if fixed else Tk
    q = torch.randn(2, 4, Tq, 64, generator=g).to(torch.bfloat16).requires_grad_(grad)
    k = torch.randn(2, 2, cap, 64, generator=g).to(torch.bfloat16)
    v = torch.randn(2, 2, cap, 64, generator=g).to(torch.bfloat16)
    if fp8:
        (k, ks), (v, vs) = quantize(k), quantize(v)
        k._bf_kv8_scale, v._bf_kv8_scale = ks, vs
    am = None
    if pad:
        am = torch.ones(2, cap, dtype=torch.long)
        am[1, :3] = 0
    fn = causal_mask_function if W is None else sliding_window_causal_mask_function(W)
    off = torch.tensor(Tk - Tq) if fixed else Tk - Tq
    mask = bf._padding_mask_interface(2, q_length=Tq, kv_length=cap, q_offset=off, mask_function=fn, attention_mask=am,
                                      allow_is_causal_skip=False, device="cpu")
    assert getattr(mask, "_bf_decode", False) and (getattr(mask, "_bf_kv_len", None) is not None) == fixed
    assert getattr(mask, "_bf_window", None) == W
    return q, k, v, mask


def _run(launches, *args, **kw):
    del launches[:]
    with torch.no_grad():
        out, _ = bf._attention_interface(_module(), *args, **kw)
    return list(launches), out


def test_the_switch_is_off_by_default_follows_the_environment_and_is_baked(monkeypatch):
    assert not bf.chunked_attention_enabled()
    model = _small_llama()
    off = graphs.baked_state(model)
    bf.chunked_attention()
    assert bf.chunked_attention_enabled() and graphs.baked_state(model) != off
    assert not graphs.still_valid(model, off)
    bf.chunked_attention(False)
    assert graphs.baked_state(model) == off and graphs.still_valid(model, off)
    monkeypatch.setenv("BF_CHUNKED_ATTENTION", "1")
    assert bf.chunked_attention_enabled()


def test_with_the_switch_off_a_cached_chunk_goes_where_it_went(launches):
    for fixed in (False, True):
        for W in (None, 12):
            kw = {} if W is None else dict(sliding_window=W)
            seen, out = _run(launches, *_call(fixed=fixed, W=W, pad=True), **kw)
            assert seen == [("sdpa",)] and out.shape == (2, 17, 4, 64)
            seen, _ = _run(launches, *_call(fixed=fixed, W=W), softcap=30.0, **kw)  # no cap kernels: SDPA, as ever
            assert seen == [("sdpa",)]
        seen, _ = _run(launches, *_call(fixed=True, fp8=True))
        assert seen == [("dequantize",), ("dequantize",), ("sdpa",)]
    bf.softcap_attention()
    seen, _ = _run(launches, *_call(Tq=40, Tk=100), softcap=30.0)
    assert seen == [("softcap_eager",)]
    seen, _ = _run(launches, *_call(fixed=True, fp8=True), softcap=30.0)
    assert seen == [("dequantize",), ("dequantize",), ("softcap_eager",)]


def test_with_the_switch_on_a_cached_chunk_goes_to_the_chunk_entries(launches):
    bf.chunked_attention()
    for fixed in (False, True):
        for W in (None, 12):
            for pad in (False, True):
                kw = {} if W is None else dict(sliding_window=W)
                keys = (2, 49 if fixed else 40) if pad else None
                seen, out = _run(launches, *_call(fixed=fixed, W=W, pad=pad), **kw)
                assert seen == [("chunk", fixed, W, None, keys)], (fixed, W, pad, seen)
                assert out.shape == (2, 17, 4, 64)
                if fixed:
                    seen, _ = _run(launches, *_call(fixed=True, W=W, pad=pad, fp8=True), **kw)
                    assert seen == [("chunk_kv8", True, W, None, keys)]  # (and no dequantise)
    # the first chunk into a static cache: its fill equals the chunk
    seen, _ = _run(launches, *_call(Tq=17, Tk=17, fixed=True))
    assert seen == [("chunk", True, None, None, None)]
    # a sliding-window cache that kept its last 11 keys of 40: the entry learns where its key 0 lies in the sequence
    from transformers.masking_utils import sliding_window_causal_mask_function

    q, k, v, _ = _call(Tq=17, Tk=28)
    am = torch.ones(2, 57, dtype=torch.long)
    am[1, :3] = 0
    mask = bf._padding_mask_interface(2, q_length=17, kv_length=28, q_offset=40, kv_offset=29, attention_mask=am,
                                      mask_function=sliding_window_causal_mask_function(12), device="cpu")
    assert mask._bf_decode and mask._bf_window == 12 and mask._bf_key_origin == 29
    seen, _ = _run(launches, q, k, v, mask, sliding_window=12)
    assert seen == [("chunk", False, 12, None, (2, 28), 29)]
    bf.softcap_attention()
    seen, _ = _run(launches, q, k, v, mask, sliding_window=12, softcap=30.0)
    assert seen == [("chunk", False, 12, 30.0, (2, 28), 29)]
    bf.softcap_attention(False)
    # a cap: only with the soft-cap kernels on
    seen, _ = _run(launches, *_call(W=12), softcap=30.0, sliding_window=12)
    assert seen == [("sdpa",)]
    seen, _ = _run(launches, *_call(fixed=True, fp8=True), softcap=30.0)
    assert seen == [("dequantize",), ("dequantize",), ("sdpa",)]
    bf.softcap_attention()
    seen, _ = _run(launches, *_call(W=12, pad=True), softcap=30.0, sliding_window=12)
    assert seen == [("chunk", False, 12, 30.0, (2, 40))]
    seen, _ = _run(launches, *_call(fixed=True, fp8=True), softcap=30.0)
    assert seen == [("chunk_kv8", True, None, 30.0, None)]


def test_what_the_chunk_entries_do_not_take_keeps_its_route(launches):
    bf.chunked_attention()
    # 16 queries and fewer are decode steps
    assert _run(launches, *_call(Tq=16))[0] == [("attention_forward_decode",)]
    assert _run(launches, *_call(Tq=16, fixed=True))[0] == [("attention_forward_decode_len",)]
    assert _run(launches, *_call(Tq=16, fixed=True, fp8=True))[0] == [("attention_forward_decode_kv8",)]
    # a gradient
    q, k, v, mask = _call(grad=True)
    del launches[:]
    bf._attention_interface(_module(), q, k, v, mask)
    assert list(launches) == [("sdpa",)]
    q, k, v, mask = _call(fixed=True, fp8=True, grad=True)
    del launches[:]
    bf._attention_interface(_module(), q, k, v, mask)
    assert list(launches) == [("dequantize",), ("dequantize",), ("sdpa",)]
    # dropout, attention sinks, a window the module disagrees with
    assert _run(launches, *_call(), dropout=0.1)[0] == [("sdpa",)]
    assert _run(launches, *_call(), s_aux=torch.zeros(4))[0] == [("sdpa",)]
    assert _run(launches, *_call(W=12), sliding_window=13)[0] == [("sdpa",)]
    assert _run(launches, *_call(fixed=True, fp8=True), s_aux=torch.zeros(4))[0] == [("dequantize",), ("dequantize",), ("sdpa",)]
    assert _run(launches, *_call(fixed=True, fp8=True, W=12), sliding_window=13)[0] == [("dequantize",), ("dequantize",), ("sdpa",)]
    # a mask _padding_mask_interface did not build, and no mask at all
    q, k, v, _ = _call()
    other = torch.ones(2, 1, 17, 40, dtype=torch.bool).tril(23)
    assert _run(launches, q, k, v, other, is_causal=True)[0] == [("sdpa",)]
    assert _run(launches, q, k, v, None)[0] == [("sdpa",)]
    # a key mask of another shape
    q, k, v, mask = _call(pad=True)
    mask._bf_key_mask = mask._bf_key_mask[:, :39]
    assert _run(launches, q, k, v, mask)[0] == [("sdpa",)]
    # under the soft-cap kernels the fallback stays the capped chain
    bf.softcap_attention()
    assert _run(launches, *_call(), softcap=30.0, dropout=0.1)[0] == [("softcap_eager",)]


def test_the_chunk_rule_sends_the_measured_loss_to_sdpa(launches, monkeypatch):
    for D in (64, 128):
        assert all(ops.chunk_kernel_wins(16, 4, Tq, L, D, W) for Tq in (17, 512, 2048) for L in (4096, 16384, 10 ** 6)
                   for W in (None, 1024))
    assert ops.chunk_kernel_wins(16, 4, 512, 4096, 256) and ops.chunk_kernel_wins(16, 4, 2048, 8191, 256)
    assert not ops.chunk_kernel_wins(16, 4, 512, 8192, 256) and not ops.chunk_kernel_wins(16, 4, 2048, 16384, 256)
    assert ops.chunk_kernel_wins(16, 4, 512, 16384, 256, window=1024)
    assert not ops.chunk_kernel_wins(16, 4, 512, 16384, 256, window=16384)  # (a window that hides nothing)
    # the 16-bit route asks it; the soft-cap and FP8 routes do not
    bf.chunked_attention()
    monkeypatch.setattr(ops, "chunk_kernel_wins", lambda *a, **k: launches.append(("rule",)) or False)
    assert _run(launches, *_call())[0] == [("rule",), ("sdpa",)]
    assert _run(launches, *_call(fixed=True, fp8=True))[0] == [("chunk_kv8", True, None, None, None)]
    bf.softcap_attention()
    assert _run(launches, *_call(), softcap=30.0)[0] == [("chunk", False, None, 30.0, None)]


# ---------------------------------------------------------------------------------------------------- sample_generate
def test_prefill_spans():
    assert _prefill_spans(150, 64) == [(0, 64), (64, 128), (128, 150)]
    assert _prefill_spans(128, 64) == [(0, 64), (64, 128)]
    assert _prefill_spans(65, 64) == [(0, 64), (64, 65)]
    assert _prefill_spans(17, 17) == [(0, 17)] and _prefill_spans(5, 64) == [(0, 5)]
    for T0, C in ((1000, 17), (4099, 512), (33, 32)):
        spans = _prefill_spans(T0, C)
        assert spans[0][0] == 0 and spans[-1][1] == T0 and all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
        assert all(b - a == C for a, b in spans[:-1]) and 0 < spans[-1][1] - spans[-1][0] <= C
    for bad in ((0, 64), (10, 0)):
        with pytest.raises(ValueError):
            _prefill_spans(*bad)


def test_sample_generate_prefill_chunk_argument_checks():
    model = _small_llama()
    bf.manual_seed(1, next_sample=3)
    ids = torch.zeros(1, 40, dtype=torch.long)
    with torch.no_grad():
        for bad in (16, 0, -64, True, 64.0, "64"):
            with pytest.raises(ValueError, match="prefill_chunk"):
                sample_generate(model, ids, samples=2, max_new_tokens=2, prefill_chunk=bad)
        with pytest.raises(RuntimeError, match="fuse_attention"):  # a chunk below T0 on a model that is not routed
            sample_generate(model, ids, samples=2, max_new_tokens=2, prefill_chunk=17)
        with pytest.raises(RuntimeError, match="fuse_attention"):
            sample_generate(model, ids, samples=2, max_new_tokens=2, prefill_chunk=17, static_cache=True)
    from bayeformers_amd import random as bfr

    assert bfr.STATE.next_sample == 3 and not bf.chunked_attention_enabled()
    assert sampling._checked_prefill_chunk(model, None, 40) is None
    assert sampling._checked_prefill_chunk(model, 40, 40) is None and sampling._checked_prefill_chunk(model, 4096, 40) is None
    assert bf.fuse_attention(model)
    assert sampling._checked_prefill_chunk(model, 17, 40) == 17


def test_the_chunked_prefill_feeds_the_spans_and_restores_the_switch():
    class Out:
        pass

    class Fake:
        """What _chunked_prefill needs of a bnn.Model: a forward that takes logits_to_keep, and the log-probs."""
        model = None

        def __init__(self, fail_at=None):
            self.calls, self.fail_at = [], fail_at

        def forward(self, input_ids=None, attention_mask=None, position_ids=None, past_key_values=None, use_cache=None,
                    logits_to_keep=0):
            raise AssertionError

        def __call__(self, **kw):
            assert bf.chunked_attention_enabled()
            if self.fail_at == len(self.calls):
                raise KeyError("boom")
            self.calls.append(kw)
            return Out()

        def log_prob_samples(self):
            return torch.full((2, 2), float(len(self.calls)))

    ids = torch.arange(300).reshape(2, 150)
    pos = ids + 1
    mask = torch.ones(2, 150, dtype=torch.long)
    fake, cache = Fake(), object()
    out, lp = sampling._chunked_prefill(fake, ids, pos, lambda b: mask[:, :b], cache, _prefill_spans(150, 64))
    assert isinstance(out, Out) and torch.equal(lp, torch.ones(2, 2))  # (read after the first span)
    assert not bf.chunked_attention_enabled()
    assert [tuple(c["input_ids"].shape) for c in fake.calls] == [(2, 64), (2, 64), (2, 22)]
    for c, (a, b) in zip(fake.calls, ((0, 64), (64, 128), (128, 150))):
        assert torch.equal(c["input_ids"], ids[:, a:b]) and torch.equal(c["position_ids"], pos[:, a:b])
        assert c["attention_mask"].shape == (2, b) and c["past_key_values"] is cache and c["use_cache"] is True
        assert c["logits_to_keep"] == 1
    fake = Fake()
    sampling._chunked_prefill(fake, ids, None, lambda b: None, cache, _prefill_spans(150, 100))
    assert all(c["position_ids"] is None and c["attention_mask"] is None for c in fake.calls) and len(fake.calls) == 2
    # an exception in a span restores the switch, whichever way it stood
    for before in (False, True):
        bf.chunked_attention(before)
        with pytest.raises(KeyError):
            sampling._chunked_prefill(Fake(fail_at=1), ids, pos, lambda b: mask[:, :b], cache, _prefill_spans(150, 64))
        assert bf._CHUNKED_ATTENTION[0] is before
    bf.chunked_attention(False)

    class NoKeep(Fake):
        def forward(self, input_ids=None, attention_mask=None, position_ids=None, past_key_values=None, use_cache=None):
            raise AssertionError

    fake = NoKeep()
    sampling._chunked_prefill(fake, ids, pos, lambda b: mask[:, :b], cache, _prefill_spans(150, 64))
    assert all("logits_to_keep" not in c for c in fake.calls)


# ---------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("Tq,Tk,L", [(17, 40, 40), (17, 49, 40), (33, 33, 33), (5, 20, 11), (130, 300, 257)])
@pytest.mark.parametrize("W,cap", [(None, None), (7, None), (150, 2.0)])
def test_the_reference_is_a_dense_mask_softmax(Tq, Tk, L, W, cap):
    g = torch.Generator().manual_seed(Tq + Tk)
    q, k, v = torch.randn(2, 4, Tq, 16, generator=g), torch.randn(2, 2, Tk, 16, generator=g), torch.randn(2, 2, Tk, 16, generator=g)
    key_mask = torch.zeros(2, Tk)
    key_mask[0, :3] = float("-inf")
    key_mask[1, :L] = float("-inf")  # a row that sees nothing
    i, j = torch.arange(Tq)[:, None], torch.arange(Tk)[None, :]
    allowed = (j <= L - Tq + i) & (j < L)
    if W is not None:
        allowed = allowed & (j > L - Tq + i - W)
    assert torch.equal(chunk_visible(Tq, Tk, L, W), allowed)
    allowed = allowed[None, None] & (key_mask == 0)[:, None, None, :]
    poisoned_k, poisoned_v = k.clone(), v.clone()
    poisoned_k[:, :, L:], poisoned_v[:, :, L:] = float("nan"), float("nan")  # the slots past the fill are not looked at
    out = chunk_reference(q, poisoned_k, poisoned_v, 0.25, L, key_mask, W, cap)
    ref = dense_reference(q, k, v, 0.25, allowed, cap)
    assert out.shape == (2, Tq, 4, 16) and out.dtype == torch.float64 and torch.isfinite(out).all()
    assert torch.allclose(out, ref, atol=1e-13, rtol=0)
    assert torch.equal(out[1], torch.zeros_like(out[1]))
    if L == Tk and W is None and cap is None:  # the decode kernels' contract is this one at a full cache
        from kv8_ref import decode_reference

        assert torch.allclose(out, decode_reference(q, k, v, 0.25, key_mask=key_mask), atol=1e-13, rtol=0)


def test_the_reference_at_a_negative_position_and_an_empty_cache():
    q, k = torch.ones(1, 1, 4, 8), torch.ones(1, 1, 6, 8)
    assert torch.equal(chunk_reference(q, k, k, 1.0, kv_len=0), torch.zeros(1, 4, 1, 8, dtype=torch.float64))
    out = chunk_reference(q, k, 2 * k, 1.0, kv_len=2)  # positions -2 .. 1: the first two queries see nothing
    assert torch.equal(out[0, :2], torch.zeros(2, 1, 8, dtype=torch.float64)) and torch.equal(out[0, 2:], torch.full((2, 1, 8), 2.0, dtype=torch.float64))
