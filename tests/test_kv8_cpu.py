"""Host side of sample_generate(kv_cache="fp8") (no GPU): the header and symbol table of the FP8 KV-cache entries, their
argument checks, the memory figure, the cache builder, the dispatch, and the torch restatement of the format
(tests/kv8_ref.py) on itself."""
import ctypes
import os
import re

import pytest
import torch

import bayeformers_amd as bf
from bayeformers_amd import _C, ops
from bayeformers_amd import sampling
from bayeformers_amd.kv_cache import Fp8StaticLayer
from bayeformers_amd.plan import kv_cache_bytes
from bayeformers_amd.sampling import _static_cache, sample_generate
from kv8_ref import decode_reference, dequantize, quantize, special_rows
from test_kept_fp8_cpu import _c_type_class, _ctypes_class, _small_llama

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"bf_kv8_append", "bf_kv8_dequantize", "bf_attention_decode_gqa_kv8"}
PTR = 4096  # an aligned non-NULL address: every call below is refused on its arguments, nothing is launched


# ---------------------------------------------------------------------------------------------------- header, bindings
def test_kv8_header_prototypes_match_the_ctypes_signatures():
    header = open(os.path.join(ROOT, "include", "bayeformers_amd_kv8.h")).read()
    assert '#include "bayeformers_amd_kv8.h"' in open(os.path.join(ROOT, "include", "bayeformers_amd.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    header = re.sub(r"^\s*#.*$", "", header, flags=re.M)
    parsed = {}
    for ret, name, params in re.findall(r"([A-Za-z_][A-Za-z0-9_ \t\n\*]*?)\b(bf_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", header):
        assert name not in parsed, name
        parsed[name] = (_c_type_class(ret), [_c_type_class(a.strip()) for a in params.split(",")])
    assert set(parsed) == set(_C.KV8_SYMBOLS) == ENTRIES
    for name, (res, args) in _C.KV8_SYMBOLS.items():
        c_res, c_args = parsed[name]
        assert _ctypes_class(res) == c_res and len(args) == len(c_args), name
        for i, (a, c) in enumerate(zip(args, c_args)):
            assert _ctypes_class(a) == c, (name, i, a, c)


def test_kv8_symbols_are_a_table_of_their_own():
    others = [_C.SYMBOLS, _C.SOFTCAP_SYMBOLS, _C.FAMILY_BLOCK_SYMBOLS, _C.FAMILY_BLOCK_BWD_SYMBOLS, _C.PACKED_SYMBOLS,
              _C.FP8_SYMBOLS]
    for table in others:
        assert not set(_C.KV8_SYMBOLS) & set(table)
    assert len(_C.SYMBOLS) == 90


def test_kv8_symbols_resolve_in_the_built_library():
    lib = _C.lib()
    for name, (res, args) in _C.KV8_SYMBOLS.items():
        fn = getattr(lib, name)
        assert fn.restype is res and fn.argtypes == args
    assert lib.bf_version() == _C.ABI_VERSION == 6


def test_a_library_without_the_kv8_entries_asks_for_a_rebuild(monkeypatch):
    class Old:
        def __getattr__(self, name):
            if name in _C.KV8_SYMBOLS:
                raise AttributeError(name)
            return getattr(real, name)

    real = ctypes.CDLL(_C.LIB_PATH)
    monkeypatch.setattr(_C, "_lib", None)
    monkeypatch.setattr(ctypes, "CDLL", lambda path: Old())
    with pytest.raises(_C.BayeFormersAMDError, match=r"lacks bf_kv8_append \(the FP8 KV-cache entries\): rebuild"):
        _C.lib()


def _shape(N=2, Tq=1, Tk=64, H=4, Hkv=2, D=64, k_stride=None):
    s = _C.bf_attn_decode_t(N, Tq, Tk, H, Hkv, D)
    s.q_stride[:] = [H * Tq * D, Tq * D, D]
    s.k_stride[:] = k_stride or [Hkv * Tk * D, Tk * D, D]
    s.v_stride[:] = [Hkv * Tk * D, Tk * D, D]
    return s


def _decode(shape, q=PTR, kq=PTR, ks=PTR, vs=PTR, ws=None, dtype=_C.BF_DT_BF16, window=0, softcap=0.0):
    lib = _C.lib()
    rc = lib.bf_attention_decode_gqa_kv8(q, kq, PTR, ks, vs, None, None, None, PTR, ws, dtype, ctypes.byref(shape), window,
                                         softcap, 0.125, None)
    return rc, lib.bf_last_error()


def test_kv8_decode_refuses_before_any_launch():
    for dtype in (_C.BF_DT_F16, _C.BF_DT_F32):
        rc, msg = _decode(_shape(), dtype=dtype)
        assert rc == 1 and b"bf16" in msg and b"bfloat16" in msg
    rc, msg = _decode(_shape(D=96))
    assert rc == 1 and b"head size 96" in msg
    for kw in (dict(ks=None), dict(vs=None)):
        rc, msg = _decode(_shape(), **kw)
        assert rc == 1 and b"NULL scale" in msg
    rc, msg = _decode(_shape(), kq=PTR + 8)
    assert rc == 1 and b"16-byte aligned" in msg
    rc, msg = _decode(_shape(), ks=PTR + 2)
    assert rc == 1 and b"4-byte aligned" in msg
    rc, msg = _decode(_shape(Tq=17))
    assert rc == 1 and b"Tq=17" in msg
    rc, msg = _decode(_shape(k_stride=[2 * 64 * 64 + 8, 64 * 64, 64]))  # fine for bf16 elements, not for bytes
    assert rc == 1 and b"multiples of 16" in msg
    rc, msg = _decode(_shape(), window=-1)
    assert rc == 1 and b"window=-1" in msg
    rc, msg = _decode(_shape(), softcap=-1.0)
    assert rc == 1 and b"softcap" in msg
    # a shape whose keys are split needs the workspace bf_attention_decode_workspace_bytes counts
    split = _shape(N=1, Tq=1, Tk=4096, H=4, Hkv=2, D=64)
    need = _C.lib().bf_attention_decode_workspace_bytes(ctypes.byref(split))
    assert need > 0
    rc, msg = _decode(split)
    assert rc == 1 and b"workspace" in msg and str(need).encode() in msg
    assert _C.lib().bf_attention_decode_workspace_bytes(ctypes.byref(_shape())) == 0


def test_kv8_append_and_dequantize_refuse_before_any_launch():
    lib = _C.lib()
    st = (ctypes.c_int64 * 3)(2 * 64, 64, 2 * 64)

    def app(k=PTR, dtype=_C.BF_DT_BF16, kq=PTR, ks=PTR, pos=PTR, D=64, strides=st, Tq=1):
        rc = lib.bf_kv8_append(k, PTR, dtype, strides, st, kq, PTR, ks, PTR, pos, 1, 2, Tq, D, 8, None)
        return rc, lib.bf_last_error()

    rc, msg = app(dtype=_C.BF_DT_F16)
    assert rc == 1 and b"bfloat16" in msg
    rc, msg = app(D=96)
    assert rc == 1 and b"head size 96" in msg
    rc, msg = app(ks=None)
    assert rc == 1 and b"NULL scale" in msg
    rc, msg = app(kq=PTR + 8)
    assert rc == 1 and b"16-byte aligned" in msg
    rc, msg = app(k=PTR + 2)
    assert rc == 1 and b"16-byte aligned" in msg
    rc, msg = app(pos=None)
    assert rc == 1 and b"pos" in msg
    rc, msg = app(Tq=0)
    assert rc == 1 and b"Tq=0" in msg
    rc, msg = app(strides=(ctypes.c_int64 * 3)(2 * 64, 64, 2 * 64 + 4))
    assert rc == 1 and b"multiples of 8" in msg

    def deq(q=PTR, scale=PTR, out=PTR, dtype=_C.BF_DT_BF16, rows=4, D=64):
        rc = lib.bf_kv8_dequantize(q, scale, out, dtype, rows, D, None)
        return rc, lib.bf_last_error()

    rc, msg = deq(dtype=_C.BF_DT_F16)
    assert rc == 1 and b"bfloat16" in msg
    rc, msg = deq(D=24)
    assert rc == 1 and b"D=24" in msg
    rc, msg = deq(scale=None)
    assert rc == 1 and b"NULL scale" in msg
    rc, msg = deq(out=PTR + 8)
    assert rc == 1 and b"16-byte aligned" in msg


def test_the_ops_wrappers_check_their_arguments_on_the_host():
    q = torch.zeros(2, 4, 1, 64, dtype=torch.bfloat16)
    kq = torch.zeros(2, 2, 8, 64, dtype=torch.uint8)
    sc = torch.zeros(2, 2, 8)
    for call in (lambda: ops.kv8_append(q[:, :2], q[:, :2], kq, kq, sc, sc, torch.zeros(1, dtype=torch.long)),
                 lambda: ops.kv8_dequantize(kq, sc),
                 lambda: ops.attention_forward_decode_kv8(q, kq, kq, sc, sc, None, None, 0.125)):
        with pytest.raises(_C.BayeFormersAMDError, match="ROCm|device"):
            call()
    assert not ops.attention_decode_kv8_supported(q, kq, kq)  # (not on the device)
    assert ops.attention_decode_kv8_supported(q, kq, kq, check_device=False)
    assert not ops.attention_decode_kv8_supported(q.half(), kq, kq, check_device=False)
    assert not ops.attention_decode_kv8_supported(q, kq.to(torch.bfloat16), kq.to(torch.bfloat16), check_device=False)
    k24 = torch.zeros(2, 2, 8, 72, dtype=torch.uint8)[..., :64]  # a token stride of 72 bytes
    assert not ops.attention_decode_kv8_supported(q, k24, k24, check_device=False)
    assert set(ops.KV8_CALLS) == {"append", "decode", "dequantize"}
    assert set(ops.DECODE_CALLS) == {"fwd", "len", "window", "len_window"}
    assert set(ops.SOFTCAP_CALLS) == {"fwd", "bwd", "decode", "decode_len"}


# ---------------------------------------------------------------------------------------------------- the reference on itself
@pytest.mark.parametrize("D", [64, 128, 256])
def test_dequantised_rows_are_exact_in_bf16_and_within_the_format_bound(D):
    g = torch.Generator().manual_seed(D)
    x = torch.cat([torch.randn(1000, D, generator=g), 30.0 * torch.randn(50, D, generator=g),
                   1e-3 * torch.randn(50, D, generator=g)]).to(torch.bfloat16)
    q, scale = quantize(x)
    assert q.dtype == torch.uint8 and q.shape == x.shape and scale.shape == x.shape[:-1] and scale.dtype == torch.float32
    exact = q.view(torch.float8_e4m3fn).float() * scale[:, None]  # fp32: a 4-bit significand times a power of two
    assert torch.equal(exact.to(torch.bfloat16).float(), exact)  # ... which bf16 holds unchanged
    assert torch.equal(dequantize(q, scale).float(), exact)
    amax = x.float().abs().amax(-1)
    assert bool((scale <= amax / 224).all()) and bool((amax / scale <= 448).all())
    err = (exact.double() - x.double()).abs()
    big = x.double().abs() >= 2.0 ** -6 * scale.double()[:, None]
    bound = torch.where(big, 2.0 ** -4 * x.double().abs(), 2.0 ** -10 * scale.double()[:, None].expand_as(err))
    assert bool((err <= bound).all()), float((err - bound).max())


@pytest.mark.parametrize("D", [64, 256])
def test_special_rows(D):
    x = special_rows(D)
    q, scale = quantize(x)
    assert bool((q[0] == 0).all()) and scale[0] == 1.0  # an all-zero row: scale 1, bytes 0
    one = D // 3  # a single large entry: the top binade, every other byte 0
    assert q[1, one] != 0 and int((q[1] != 0).sum()) == 1 and dequantize(q, scale)[1, one] == x[1, one]
    assert 224 < float(x[1, one]) / float(scale[1]) <= 448
    assert bool((q[2] >= 0x80).all())  # negatives keep their sign bit
    back = dequantize(q, scale).float()
    assert bool((back[2] < 0).all())
    # magnitudes down to 2^-20 amax: below half a subnormal step (2^-10 scale) they round to (signed) zero
    tiny = x[3].float().abs() < 2.0 ** -10 * scale[3]
    assert bool(tiny.any()) and bool((back[3][tiny] == 0).all()) and bool((back[3][~tiny & (x[3].float().abs() > 2.0 ** -9 * scale[3])] != 0).all())
    err = (back.double() - x.double()).abs()
    assert bool((err <= torch.maximum(2.0 ** -4 * x.double().abs(), 2.0 ** -10 * scale.double()[:, None])).all())


def test_the_decode_reference_is_the_plain_one_without_options_and_zero_on_a_hidden_row():
    g = torch.Generator().manual_seed(2)
    q, k, v = torch.randn(2, 4, 3, 16, generator=g), torch.randn(2, 2, 20, 16, generator=g), torch.randn(2, 2, 20, 16, generator=g)
    full = decode_reference(q, k, v, 0.25)
    assert torch.allclose(full, decode_reference(q, k, v, 0.25, kv_len=20, window=100), atol=0, rtol=0)
    short = decode_reference(q, k, v, 0.25, kv_len=11, window=4, softcap=2.0)
    assert torch.allclose(short, decode_reference(q, k[:, :, 5:11], v[:, :, 5:11], 0.25, window=4, softcap=2.0), atol=1e-14)
    mask = torch.zeros(2, 20)
    mask[1] = float("-inf")
    assert torch.equal(decode_reference(q, k, v, 0.25, key_mask=mask)[1], torch.zeros(3, 4, 16, dtype=torch.float64))


# ---------------------------------------------------------------------------------------------------- the memory figure
def test_kv_cache_bytes_hand_count_llama():
    model = _small_llama()  # 2 layers, 2 K/V heads, head size 64 / 4 = 16
    L, Hkv, D = 2, 2, 16
    for S, B, cap in ((1, 1, 7), (3, 2, 64), (10, 8, 4096)):
        rows = L * S * B * Hkv * cap  # K rows; as many V rows
        assert kv_cache_bytes(model, S, B, cap) == kv_cache_bytes(model, S, B, cap, torch.bfloat16, fp8=False) == rows * 4 * D
        assert kv_cache_bytes(model, S, B, cap, torch.float32) == rows * 8 * D
        assert kv_cache_bytes(model, S, B, cap, fp8=True) == rows * (2 * D + 8)
        assert kv_cache_bytes(model, S, B, cap, fp8=True) / kv_cache_bytes(model, S, B, cap) == (2 * D + 8) / (4 * D)
    assert bf.kv_cache_bytes is kv_cache_bytes and "kv_cache_bytes" in bf.__all__
    for dt in (torch.float16, torch.float32):
        with pytest.raises(ValueError, match="bfloat16"):
            kv_cache_bytes(model, 2, 2, 8, dt, fp8=True)
    with pytest.raises(ValueError, match="capacity"):
        kv_cache_bytes(model, 2, 2, 0)


def test_kv_cache_bytes_at_the_llama_8b_layout():
    class Cfg:
        num_hidden_layers, num_attention_heads, num_key_value_heads, hidden_size, head_dim = 32, 32, 8, 4096, 128

    class M:
        config = Cfg()

    assert kv_cache_bytes(M(), 1, 1, 1) == 128 * 1024  # 128 KiB per token and sample
    assert kv_cache_bytes(M(), 10, 8, 4096, fp8=True) / kv_cache_bytes(M(), 10, 8, 4096) == 264 / 512


# ---------------------------------------------------------------------------------------------------- sample_generate
def test_sample_generate_kv_cache_argument_checks():
    model = _small_llama()
    bf.manual_seed(1, next_sample=3)
    ids = torch.zeros(1, 4, dtype=torch.long)
    with torch.no_grad():
        for bad in ("int4", True, "FP8", 8):
            with pytest.raises(ValueError, match="kv_cache"):
                sample_generate(model, ids, samples=2, max_new_tokens=2, kv_cache=bad)
        for name in ("fp32", "fp16"):
            bf.set_compute_dtype(name)
            try:
                with pytest.raises(ValueError, match="bfloat16"):
                    sample_generate(model, ids, samples=2, max_new_tokens=2, kv_cache="fp8")
            finally:
                bf.set_compute_dtype("bf16")
        with pytest.raises(RuntimeError, match="fuse_attention"):  # implies static_cache: the model is not routed
            sample_generate(model, ids, samples=2, max_new_tokens=2, kv_cache="fp8")
        with pytest.raises(ValueError, match="single process"):
            sample_generate(model, ids, samples=2, max_new_tokens=2, kv_cache="fp8", group=object())
        with pytest.raises(NotImplementedError, match="S-sharded"):
            sample_generate(model, ids, samples=2, max_new_tokens=2, group=object())
    from bayeformers_amd import random as bfr

    assert bfr.STATE.next_sample == 3


def _mistral(window=4):
    from transformers import AutoConfig, AutoModelForCausalLM

    cfg = AutoConfig.for_model("mistral", hidden_size=64, num_attention_heads=4, num_key_value_heads=2, head_dim=16,
                               num_hidden_layers=2, intermediate_size=128, vocab_size=100, max_position_embeddings=64,
                               tie_word_embeddings=False, sliding_window=window)
    torch.manual_seed(0)
    return bf.to_bayesian(AutoModelForCausalLM.from_config(cfg).eval(), delta=0.05, freeze=True).eval()


@pytest.mark.parametrize("build", [_small_llama, _mistral], ids=["llama", "mistral"])
def test_static_cache_builds_fp8_layers_on_request(build):
    from transformers.cache_utils import StaticLayer

    model = build()
    with pytest.raises(RuntimeError, match="fuse_attention"):
        _static_cache(model, 64, kv_cache="fp8")
    assert bf.fuse_attention(model)
    cache = _static_cache(model, 64, kv_cache="fp8")
    assert len(cache.layers) == 2
    for layer in cache.layers:
        assert type(layer) is Fp8StaticLayer and isinstance(layer, StaticLayer)
        assert layer.max_cache_len == 64 and layer.get_mask_sizes(1) == (64, 0) and not layer.is_sliding
        assert layer.store_bytes() == 0 and layer.get_seq_length() == 0
    for plain in (_static_cache(model, 64), _static_cache(model, 64, kv_cache=None)):
        assert [type(layer) for layer in plain.layers] == [StaticLayer, StaticLayer]
    with pytest.raises(ValueError, match="kv_cache"):
        _static_cache(model, 64, kv_cache="int4")
    assert sampling._STATIC_LAYER_HOOK is None


def test_the_fp8_layer_refuses_other_dtypes():
    layer = Fp8StaticLayer(max_cache_len=8)
    for dt in (torch.float16, torch.float32):
        x = torch.zeros(1, 2, 1, 64, dtype=dt)
        with pytest.raises(ValueError, match="bfloat16"):
            layer.update(x, x)


# ---------------------------------------------------------------------------------------------------- dispatch
@pytest.fixture
def launches(monkeypatch):
    """Pretend the kv8 entries apply to CPU tensors and record what each call was given."""
    seen = []
    real = ops.attention_decode_kv8_supported
    monkeypatch.setattr(ops, "attention_decode_kv8_supported", lambda q, k, v, check_device=True: real(q, k, v, False))
    monkeypatch.setattr(ops, "decode_kernel_wins", lambda *a, **k: seen.append(("decode_kernel_wins",)) or False)

    def kv8(q, kq, vq, k_scale, v_scale, kv_len, key_mask, scaling, mask_off=None, workspace=None, window=None, softcap=None):
        assert kq.dtype == torch.uint8 and vq.dtype == torch.uint8 and kv_len is not None
        assert k_scale is kq._bf_kv8_scale and v_scale is vq._bf_kv8_scale
        seen.append(("kv8", window, softcap, None if key_mask is None else tuple(key_mask.shape)))
        return torch.zeros(q.shape[0], q.shape[2], q.shape[1], q.shape[3], dtype=q.dtype)

    def deq(q, scale, out=None):
        assert q.dtype == torch.uint8
        seen.append(("dequantize",))
        return dequantize(q, scale)

    import transformers.integrations.sdpa_attention as sa

    real_sdpa = sa.sdpa_attention_forward

    def sdpa(module, q, k, v, *a, **kw):
        assert k.dtype == q.dtype and v.dtype == q.dtype  # never the uint8 rows
        seen.append(("sdpa",))
        kw.pop("s_aux", None), kw.pop("softcap", None)
        return real_sdpa(module, q, k, v, *a, **kw)

    eager = bf._softcap_eager
    monkeypatch.setattr(bf, "_softcap_eager", lambda m, q, k, v, *a, **kw: (
        seen.append(("softcap_eager", str(k.dtype))) or eager(m, q, k, v, *a, **kw)))
    monkeypatch.setattr(ops, "attention_forward_decode_kv8", kv8)
    monkeypatch.setattr(ops, "kv8_dequantize", deq)
    monkeypatch.setattr(sa, "sdpa_attention_forward", sdpa)
    yield seen
    bf.softcap_attention(False)


def _fp8_call(Tq=1, cap=40, fill=7, W=None, pad=False, D=64):
    from transformers.masking_utils import causal_mask_function, sliding_window_causal_mask_function

    g = torch.Generator().manual_seed(0)
    q = torch.randn(2, 4, Tq, D, generator=g).to(torch.bfloat16)
    kq, ks = quantize(torch.randn(2, 2, cap, D, generator=g).to(torch.bfloat16))
    vq, vs = quantize(torch.randn(2, 2, cap, D, generator=g).to(torch.bfloat16))
    kq._bf_kv8_scale, vq._bf_kv8_scale = ks, vs
    am = None
    if pad:
        am = torch.ones(2, cap, dtype=torch.long)
        am[1, :3] = 0
    fn = causal_mask_function if W is None else sliding_window_causal_mask_function(W)
    mask = bf._padding_mask_interface(2, q_length=Tq, kv_length=cap, q_offset=torch.tensor(fill), mask_function=fn,
                                      attention_mask=am, allow_is_causal_skip=False)
    assert mask._bf_kv_len is not None and getattr(mask, "_bf_window", None) == W
    return q, kq, vq, mask


def _module():
    mod = torch.nn.Module()
    mod.is_causal = True
    mod.num_key_value_groups = 2
    return mod.eval()


def _kernel_calls(seen):
    return [e for e in seen if e[0] != "decode_kernel_wins"]


def test_an_fp8_cache_step_goes_to_the_kv8_decode_with_the_window_and_the_cap(launches):
    d0, s0, k0 = dict(ops.DECODE_CALLS), dict(ops.SOFTCAP_CALLS), dict(ops.KV8_CALLS)
    with torch.no_grad():
        for Tq in (1, 16):
            for W, pad in ((None, False), (None, True), (12, False), (12, True)):
                del launches[:]
                q, kq, vq, mask = _fp8_call(Tq=Tq, W=W, pad=pad, fill=7 if Tq == 1 else 16)
                kw = {} if W is None else dict(sliding_window=W)
                out, _ = bf._attention_interface(_module(), q, kq, vq, mask, **kw)
                assert launches == [("kv8", W, None, (2, 40) if pad else None)], (Tq, W, pad, launches)  # (no rule was asked)
                assert out.shape == (2, Tq, 4, 64)
        # the soft-cap: taken with the switch on; with it off the call dequantises and goes where bf16 tensors go (SDPA)
        q, kq, vq, mask = _fp8_call(W=12)
        del launches[:]
        bf._attention_interface(_module(), q, kq, vq, mask, softcap=30.0, sliding_window=12)
        assert _kernel_calls(launches) == [("dequantize",), ("dequantize",), ("sdpa",)]
        bf.softcap_attention()
        del launches[:]
        bf._attention_interface(_module(), q, kq, vq, mask, softcap=30.0, sliding_window=12)
        assert launches == [("kv8", 12, 30.0, None)]
    assert ops.DECODE_CALLS == d0 and ops.SOFTCAP_CALLS == s0 and ops.KV8_CALLS == k0  # (the fakes count nothing)


def test_what_the_kv8_decode_does_not_take_dequantises_first(launches):
    d0, s0 = dict(ops.DECODE_CALLS), dict(ops.SOFTCAP_CALLS)
    with torch.no_grad():
        q, kq, vq, mask = _fp8_call(Tq=17, fill=17)  # a 17-query chunk
        bf._attention_interface(_module(), q, kq, vq, mask)
        assert _kernel_calls(launches) == [("dequantize",), ("dequantize",), ("sdpa",)]
        del launches[:]
        q, kq, vq, mask = _fp8_call()
        bf._attention_interface(_module(), q, kq, vq, mask, dropout=0.1)
        assert _kernel_calls(launches) == [("dequantize",), ("dequantize",), ("sdpa",)]
        del launches[:]
        bf._attention_interface(_module(), q, kq, vq, mask, s_aux=torch.zeros(4))
        assert _kernel_calls(launches) == [("dequantize",), ("dequantize",), ("sdpa",)]
        del launches[:]
        q, kq, vq, mask = _fp8_call(W=12)
        bf._attention_interface(_module(), q, kq, vq, mask, sliding_window=13)  # the module disagrees with the mask
        assert _kernel_calls(launches) == [("dequantize",), ("dequantize",), ("sdpa",)]
        del launches[:]
        bf.softcap_attention()
        q, kq, vq, mask = _fp8_call(Tq=17, fill=17)  # with a cap the fallback is the capped chain, on bf16 tensors
        bf._attention_interface(_module(), q, kq, vq, mask, softcap=30.0)
        assert _kernel_calls(launches) == [("dequantize",), ("dequantize",), ("softcap_eager", "torch.bfloat16")]
        del launches[:]
        q, kq, vq, _ = _fp8_call()
        bf._attention_interface(_module(), q, kq, vq, None)  # no fixed-capacity mask at all
        assert _kernel_calls(launches)[:2] == [("dequantize",), ("dequantize",)] and "kv8" not in [e[0] for e in launches]
    assert ops.DECODE_CALLS == d0 and ops.SOFTCAP_CALLS == s0


def test_a_gradient_keeps_an_fp8_cache_call_off_the_kernel(launches):
    q, kq, vq, mask = _fp8_call()
    bf._attention_interface(_module(), q.requires_grad_(), kq, vq, mask)
    assert _kernel_calls(launches) == [("dequantize",), ("dequantize",), ("sdpa",)]
