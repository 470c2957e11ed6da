"""Host side of sample_generate(sliding_cache="ring") (no GPU): the slot rule, the memory figure, the header and symbol
table of the ring-buffer KV-cache entries, what they refuse before any launch, sample_generate's refusals, the layers
_static_cache builds and the dispatch guard of a ring-marked key."""
import ctypes
import os
import re

import pytest
import torch

import bayeformers_amd as bf
from bayeformers_amd import _C, ops, sampling
from bayeformers_amd.kv_cache import Fp8RingStaticLayer, RingStaticLayer
from bayeformers_amd.plan import kv_cache_bytes
from bayeformers_amd.sampling import _static_cache, sample_generate
from ring_cache_ref import live_keys, placement, visible_span, written_rows
from test_kept_fp8_cpu import _c_type_class, _ctypes_class, _small_llama

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"bf_kv_ring_append", "bf_kv8_ring_append", "bf_attention_decode_gqa_ring", "bf_attention_decode_gqa_ring_kv8"}
PTR = 4096  # an aligned non-NULL address: every call below is refused on its arguments, nothing is launched


# ---------------------------------------------------------------------------------------------------- the rule
def test_ring_slots_is_the_window_plus_the_most_queries_less_one():
    assert ops.DECODE_MAX_QUERIES == 16
    assert ops.ring_slots(20, 119) == 35 and ops.ring_slots(4096, 32768) == 4111 and ops.ring_slots(1, 17) == 16
    assert ops.ring_slots(7, 40) == 22 and ops.ring_slots(129, 1000) == 144 and ops.ring_slots(1000, 4100) == 1015
    # C >= capacity: the layer stays a plain one
    assert ops.ring_slots(20, 35) is None and ops.ring_slots(20, 34) is None and ops.ring_slots(20, 36) == 35
    assert ops.ring_slots(4096, 4096) is None and ops.ring_slots(None, 100) is None
    for bad in ((0, 10), (-3, 10), (4, 0)):
        with pytest.raises(ValueError, match="ring_slots"):
            ops.ring_slots(*bad)


@pytest.mark.parametrize("C", [1, 7, 22, 35])
def test_the_placement_reference(C):
    for fill in (0, 1, C - 3, C, 2 * C + 1):
        if fill < 0:
            continue
        for T in (1, 5, 16, C, C + 9, 3 * C + 2):
            slots = placement(fill, T, C)
            rows = written_rows(T, C)
            # the last min(T, C) rows, each in a slot of its own: what one launch writes without writing a slot twice
            assert sorted(slots.values()) == rows and len(slots) == min(T, C)
            assert all(slot == (fill + i) % C for slot, i in slots.items())
            # afterwards the ring holds the last C sequence indices
            held = live_keys(fill + T, C)
            for slot, i in slots.items():
                assert held[fill + i] == slot


def test_a_step_never_reads_a_key_it_overwrote():
    for W in (1, 7, 20, 129):
        C = ops.ring_slots(W, 10 ** 6)
        for Tq in (1, 5, 16):
            for L in (Tq, W, W + 1, C, C + 1, 3 * C + 5):
                if L < Tq:
                    continue
                lo, hi = visible_span(L, Tq, W)
                held = live_keys(L, C)
                assert hi - lo <= C and all(j in held for j in range(lo, hi))


# ---------------------------------------------------------------------------------------------------- the memory figure
def _config(kind, **kw):
    from transformers import AutoConfig

    class M:
        config = AutoConfig.for_model(kind, hidden_size=64, num_attention_heads=4, num_key_value_heads=2, head_dim=16,
                                      num_hidden_layers=2, intermediate_size=128, vocab_size=100,
                                      max_position_embeddings=64, tie_word_embeddings=False, **kw)
    return M()


CONFIGS = {
    "mistral": (dict(sliding_window=4), [True, True]),
    "qwen2": (dict(sliding_window=4, use_sliding_window=True, max_window_layers=1,
                   layer_types=["full_attention", "sliding_attention"]), [False, True]),
    "gemma2": (dict(sliding_window=4, layer_types=["sliding_attention", "full_attention"]), [True, False]),
    "llama": (dict(), [False, False]),
}


@pytest.mark.parametrize("kind", list(CONFIGS))
def test_kv_cache_bytes_ring_hand_count(kind):
    kw, sliding = CONFIGS[kind]
    model = _config(kind, **kw)
    Hkv, D, C = 2, 16, 4 + 15
    assert sampling._sliding_windows(model.config, 64) == [4 if s else None for s in sliding]
    for S, B, cap in ((1, 1, 7), (3, 2, 64), (10, 8, 4096), (2, 2, C), (2, 2, C + 1)):
        slots = sum(min(cap, C) if s else cap for s in sliding)
        assert kv_cache_bytes(model, S, B, cap, ring=True) == slots * S * B * Hkv * 4 * D
        assert kv_cache_bytes(model, S, B, cap, torch.float32, ring=True) == slots * S * B * Hkv * 8 * D
        assert kv_cache_bytes(model, S, B, cap, fp8=True, ring=True) == slots * S * B * Hkv * (2 * D + 8)
        plain = kv_cache_bytes(model, S, B, cap)
        assert plain == kv_cache_bytes(model, S, B, cap, ring=False) == 2 * cap * S * B * Hkv * 4 * D
        if not any(sliding) or cap <= C:
            assert kv_cache_bytes(model, S, B, cap, ring=True) == plain
        else:
            assert kv_cache_bytes(model, S, B, cap, ring=True) < plain


def test_kv_cache_bytes_ring_at_a_mistral_7b_layout():
    from transformers import AutoConfig

    class M:
        config = AutoConfig.for_model("mistral", hidden_size=4096, num_attention_heads=32, num_key_value_heads=8,
                                      num_hidden_layers=32, sliding_window=4096)

    full, ring = kv_cache_bytes(M(), 1, 1, 32768), kv_cache_bytes(M(), 1, 1, 32768, ring=True)
    assert full == 32 * 32768 * 8 * 4 * 128 and ring == 32 * 4111 * 8 * 4 * 128  # 7.97x


# ---------------------------------------------------------------------------------------------------- header, bindings
def test_ring_header_prototypes_match_the_ctypes_signatures():
    header = open(os.path.join(ROOT, "include", "bayeformers_amd_ring.h")).read()
    assert '#include "bayeformers_amd_ring.h"' in open(os.path.join(ROOT, "include", "bayeformers_amd.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    header = re.sub(r"^\s*#.*$", "", header, flags=re.M)
    parsed = {}
    for ret, name, params in re.findall(r"([A-Za-z_][A-Za-z0-9_ \t\n\*]*?)\b(bf_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", header):
        assert name not in parsed, name
        parsed[name] = (_c_type_class(ret), [_c_type_class(a.strip()) for a in params.split(",")])
    assert set(parsed) == set(_C.RING_SYMBOLS) == ENTRIES
    for name, (res, args) in _C.RING_SYMBOLS.items():
        c_res, c_args = parsed[name]
        assert _ctypes_class(res) == c_res and len(args) == len(c_args), name
        for i, (a, c) in enumerate(zip(args, c_args)):
            assert _ctypes_class(a) == c, (name, i, a, c)


def test_ring_symbols_are_a_table_of_their_own_and_resolve():
    others = [_C.SYMBOLS, _C.SOFTCAP_SYMBOLS, _C.FAMILY_BLOCK_SYMBOLS, _C.FAMILY_BLOCK_BWD_SYMBOLS, _C.PACKED_SYMBOLS,
              _C.FP8_SYMBOLS, _C.KV8_SYMBOLS, _C.CHUNK_SYMBOLS, _C.ENCODER_ANY_SYMBOLS, _C.LORA_SYMBOLS]
    for table in others:
        assert not set(_C.RING_SYMBOLS) & set(table)
    lib = _C.lib()
    for name, (res, args) in _C.RING_SYMBOLS.items():
        fn = getattr(lib, name)
        assert fn.restype is res and fn.argtypes == args
    assert "bf_kv_ring.hip" in __import__("bayeformers_amd.build", fromlist=["SOURCES"]).SOURCES


def _shape(N=2, Tq=1, Tk=64, H=4, Hkv=2, D=64, kv_bytes=False):
    s = _C.bf_attn_decode_t(N, Tq, Tk, H, Hkv, D)
    s.q_stride[:] = [Tq * H * D, D, H * D]
    s.k_stride[:] = s.v_stride[:] = [Hkv * 22 * D, 22 * D, D]
    return s


def _refused(rc):
    assert rc == 1
    return _C.lib().bf_last_error().decode()


def test_ring_decode_refuses_before_any_launch():
    lib = _C.lib()

    def dec(shape=None, kv_len=PTR, ring=22, window=7, softcap=0.0, dtype=_C.BF_DT_BF16, kv8=False):
        shape = shape if shape is not None else _shape()
        if kv8:
            return lib.bf_attention_decode_gqa_ring_kv8(PTR, PTR, PTR, PTR, PTR, None, None, kv_len, PTR, None, dtype,
                                                        ctypes.byref(shape), ring, window, softcap, 0.125, None)
        return lib.bf_attention_decode_gqa_ring(PTR, PTR, PTR, None, None, kv_len, PTR, None, dtype, ctypes.byref(shape),
                                                ring, window, softcap, 0.125, None)

    for kv8 in (False, True):
        assert "kv_len" in _refused(dec(kv_len=None, kv8=kv8))  # the fill is required
        assert "kv_len" in _refused(dec(kv_len=PTR + 4, kv8=kv8))
        assert "window=0" in _refused(dec(window=0, kv8=kv8))
        assert "ring_slots=0" in _refused(dec(ring=0, kv8=kv8))
        assert "softcap" in _refused(dec(softcap=-1.0, kv8=kv8))
        assert "need 23 ring slots" in _refused(dec(window=23, ring=22, kv8=kv8))
        # window + Tq - 1 <= ring_slots: 7 + 16 - 1 = 22 passes the ring check (and fails on nothing it launches: NULL q)
        assert "need 23 ring slots" in _refused(dec(shape=_shape(Tq=16), window=8, kv8=kv8))
        assert "Tq=17" in _refused(dec(shape=_shape(Tq=17), window=1, ring=40, kv8=kv8))
    assert "bf16" in _refused(dec(dtype=_C.BF_DT_F16, kv8=True))
    assert "dtype" in _refused(dec(dtype=_C.BF_DT_F32))


def test_ring_appends_refuse_before_any_launch():
    lib = _C.lib()
    st = (ctypes.c_int64 * 3)(2 * 64, 64, 2 * 64)

    def app(k=PTR, dtype=_C.BF_DT_BF16, kc=PTR, pos=PTR, D=64, strides=st, T=1, ring=22, kv8=False, ks=PTR):
        if kv8:
            return lib.bf_kv8_ring_append(k, PTR, dtype, strides, strides, kc, PTR, ks, PTR, pos, 2, 2, T, D, ring, None)
        return lib.bf_kv_ring_append(k, PTR, dtype, strides, strides, kc, PTR, pos, 2, 2, T, D, ring, None)

    for kv8 in (False, True):
        assert "NULL" in _refused(app(k=None, kv8=kv8))
        assert "NULL" in _refused(app(kc=None, kv8=kv8))
        assert "pos" in _refused(app(pos=None, kv8=kv8))
        assert "pos" in _refused(app(pos=PTR + 4, kv8=kv8))
        assert "head size 48" in _refused(app(D=48, kv8=kv8))
        assert "T=0" in _refused(app(T=0, kv8=kv8))
        assert "ring_slots=0" in _refused(app(ring=0, kv8=kv8))
        assert "aligned" in _refused(app(k=PTR + 8, kv8=kv8))
        assert "strides" in _refused(app(strides=(ctypes.c_int64 * 3)(2 * 64, 64, 60), kv8=kv8))
    assert "dtype" in _refused(app(dtype=_C.BF_DT_F32))
    assert "bf16" in _refused(app(dtype=_C.BF_DT_F16, kv8=True))
    assert "scale" in _refused(app(kv8=True, ks=None))


def test_the_ops_wrappers_check_their_arguments_on_the_host():
    k = torch.zeros(2, 2, 1, 64, dtype=torch.bfloat16)
    kc = torch.zeros(2, 2, 22, 64, dtype=torch.bfloat16)
    pos = torch.zeros(1, dtype=torch.int64)
    with pytest.raises(_C.BayeFormersAMDError, match="ROCm|device"):
        ops.kv_ring_append(k, k, kc, kc, pos)
    with pytest.raises(_C.BayeFormersAMDError, match="ROCm|device"):
        ops.attention_forward_decode_ring(k, kc, kc, pos, None, 0.125, None, None, 7, 22, 40)
    assert set(ops.RING_CALLS) == {"append", "kv8_append", "decode", "kv8_decode"}


# ---------------------------------------------------------------------------------------------------- sample_generate
def _mistral(window=4):
    from transformers import AutoModelForCausalLM

    cfg = _config("mistral", sliding_window=window).config
    torch.manual_seed(0)
    return bf.to_bayesian(AutoModelForCausalLM.from_config(cfg).eval(), delta=0.05, freeze=True).eval()


def test_sample_generate_sliding_cache_refusals():
    ids = torch.zeros(1, 4, dtype=torch.long)
    llama, mistral = _small_llama(), _mistral()
    with torch.no_grad():
        for bad in ("roll", True, "RING", 4):
            with pytest.raises(ValueError, match="sliding_cache"):
                sample_generate(mistral, ids, samples=2, max_new_tokens=2, sliding_cache=bad)
        with pytest.raises(ValueError, match="prefill_chunk"):
            sample_generate(mistral, torch.zeros(1, 40, dtype=torch.long), samples=2, max_new_tokens=2,
                            sliding_cache="ring", prefill_chunk=17)
        with pytest.raises(RuntimeError, match="fuse_attention"):  # implies static_cache: the model is not routed
            sample_generate(mistral, ids, samples=2, max_new_tokens=2, sliding_cache="ring")
        assert bf.fuse_attention(llama) and bf.fuse_attention(mistral)
        with pytest.raises(ValueError, match="would change nothing"):  # no sliding layers
            sample_generate(llama, torch.zeros(1, 40, dtype=torch.long), samples=2, max_new_tokens=2, sliding_cache="ring")
        with pytest.raises(ValueError, match="would change nothing"):  # every C = 19 >= capacity = 5
            sample_generate(mistral, ids, samples=2, max_new_tokens=2, sliding_cache="ring")
        with pytest.raises(ValueError, match="would change nothing"):  # capacity 19 = C exactly
            sample_generate(mistral, torch.zeros(1, 18, dtype=torch.long), samples=2, max_new_tokens=2, sliding_cache="ring")


def test_static_cache_builds_ring_layers_for_the_sliding_layers_alone():
    from transformers import AutoModelForCausalLM
    from transformers.cache_utils import StaticLayer

    from bayeformers_amd.kv_cache import Fp8StaticLayer

    kw, sliding = CONFIGS["qwen2"]
    torch.manual_seed(0)
    model = bf.to_bayesian(AutoModelForCausalLM.from_config(_config("qwen2", **kw).config).eval(), delta=0.05,
                           freeze=True).eval()
    assert bf.fuse_attention(model)
    for fp8, ring_cls, full_cls in ((None, RingStaticLayer, StaticLayer), ("fp8", Fp8RingStaticLayer, Fp8StaticLayer)):
        cache = _static_cache(model, 64, kv_cache=fp8, sliding_cache="ring")
        assert [type(layer) for layer in cache.layers] == [full_cls, ring_cls]
        ring = cache.layers[1]
        assert isinstance(ring, StaticLayer) and ring.ring_slots == 19 and ring.max_cache_len == 64
        assert ring.get_mask_sizes(1) == (64, 0) and not ring.is_sliding and ring.store_bytes() == 0
        assert ring.get_seq_length() == 0
    plain = _static_cache(model, 64)
    assert [type(layer) for layer in plain.layers] == [StaticLayer, StaticLayer]
    with pytest.raises(ValueError, match="sliding_cache"):
        _static_cache(model, 64, sliding_cache="roll")
    with pytest.raises(ValueError, match="ring_slots"):
        RingStaticLayer(max_cache_len=19, ring_slots=19)
    for cls, bad in ((RingStaticLayer, torch.float32), (Fp8RingStaticLayer, torch.float16)):
        x = torch.zeros(1, 2, 1, 64, dtype=bad)
        with pytest.raises(ValueError, match="bfloat16"):
            cls(max_cache_len=64, ring_slots=19).update(x, x)


# ---------------------------------------------------------------------------------------------------- dispatch
def _ring_call(Tq=1, window=7, slots=22, capacity=40, fp8=False, marks=True):
    q = torch.zeros(2, 4, Tq, 64, dtype=torch.bfloat16)
    k, v = (torch.zeros(2, 2, slots, 64, dtype=torch.uint8 if fp8 else torch.bfloat16) for _ in range(2))
    k._bf_ring = v._bf_ring = (slots, capacity)
    if fp8:
        k._bf_kv8_scale, v._bf_kv8_scale = (torch.ones(2, 2, slots) for _ in range(2))
    mask = torch.ones(2, 1, Tq, capacity, dtype=torch.bool)
    if marks:
        mask._bf_kv_len, mask._bf_window, mask._bf_key_mask, mask._bf_mask_off = torch.tensor([9]), window, None, None
    return q, k, v, mask


def test_what_the_ring_entries_do_not_take_raises_and_never_reaches_the_framework(monkeypatch):
    from transformers.integrations import sdpa_attention

    def never(*a, **k):
        raise AssertionError("the framework's attention was given a ring-buffer cache")

    monkeypatch.setattr(sdpa_attention, "sdpa_attention_forward", never)
    monkeypatch.setattr(ops, "kv8_dequantize", never)
    monkeypatch.setattr(ops, "decode_kernel_wins", never)
    ai = bf._attention_interface
    for fp8 in (False, True):
        q, k, v, mask = _ring_call(Tq=17, fp8=fp8)
        with pytest.raises(RuntimeError, match="ring-buffer cache.*17 queries"):
            ai(None, q, k, v, mask)
        q, k, v, mask = _ring_call(fp8=fp8)
        with pytest.raises(RuntimeError, match="dropout"):
            ai(None, q, k, v, mask, dropout=0.1)
        with pytest.raises(RuntimeError, match="s_aux"):
            ai(None, q, k, v, mask, s_aux=torch.zeros(4))
        with pytest.raises(RuntimeError, match="softcap_attention"):
            ai(None, q, k, v, mask, softcap=30.0)
        with pytest.raises(RuntimeError, match="sliding_window=9"):
            ai(None, q, k, v, mask, sliding_window=9)
        with pytest.raises(RuntimeError, match="gradient"):
            with torch.enable_grad():
                ai(None, q.float().requires_grad_(True), k, v, mask)
        for m in (None, _ring_call(fp8=fp8, marks=False)[3]):
            with pytest.raises(RuntimeError, match="not the sliding-window mask"):
                ai(None, q, k, v, m)
        q, k, v, mask = _ring_call(Tq=5, window=20, fp8=fp8)
        with pytest.raises(RuntimeError, match="needs 24 slots"):
            ai(None, q, k, v, mask)
        q, k, v, mask = _ring_call(fp8=fp8)
        mask._bf_key_mask = torch.zeros(2, 22)  # over the slots, not the capacity
        with pytest.raises(RuntimeError, match="key mask"):
            ai(None, q, k, v, mask)
        v._bf_ring = None
        with pytest.raises(RuntimeError, match="same ring"):
            ai(None, q, k, v, _ring_call(fp8=fp8)[3])


def test_a_ring_step_goes_to_the_ring_decode_with_the_window_the_cap_and_the_capacity(monkeypatch):
    seen = []
    monkeypatch.setattr(ops, "attention_decode_supported", lambda q, k, v, check_device=True: True)
    monkeypatch.setattr(ops, "attention_decode_kv8_supported", lambda q, k, v, check_device=True: True)
    monkeypatch.setattr(ops, "decode_kernel_wins", lambda *a, **k: seen.append("wins") or False)

    def ring(q, k, v, kv_len, key_mask, scaling, mask_off=None, workspace=None, window=None, ring_slots=None,
             capacity=None, softcap=None):
        seen.append(("ring", int(kv_len), key_mask, window, ring_slots, capacity, softcap, scaling))
        return torch.zeros(q.shape[0], q.shape[2], q.shape[1], q.shape[3], dtype=q.dtype)

    def ring8(q, kq, vq, ks, vs, kv_len, key_mask, scaling, mask_off=None, workspace=None, window=None, ring_slots=None,
              capacity=None, softcap=None):
        seen.append(("ring8", int(kv_len), key_mask, window, ring_slots, capacity, softcap, scaling))
        return torch.zeros(q.shape[0], q.shape[2], q.shape[1], q.shape[3], dtype=q.dtype)

    monkeypatch.setattr(ops, "attention_forward_decode_ring", ring)
    monkeypatch.setattr(ops, "attention_forward_decode_ring_kv8", ring8)
    for fp8, tag in ((False, "ring"), (True, "ring8")):
        q, k, v, mask = _ring_call(Tq=16, fp8=fp8)  # 7 + 16 - 1 = 22 slots: the most a step carries
        key_mask = mask._bf_key_mask = torch.zeros(2, 40)
        out, _ = bf._attention_interface(None, q, k, v, mask, scaling=0.5, sliding_window=7)
        assert out.shape == (2, 16, 4, 64)
        assert seen.pop() == (tag, 9, key_mask, 7, 22, 40, None, 0.5)
        bf.softcap_attention()
        try:
            bf._attention_interface(None, q, k, v, mask, softcap=30.0)
        finally:
            bf.softcap_attention(False)
        assert seen.pop() == (tag, 9, key_mask, 7, 22, 40, 30.0, 64 ** -0.5)
    assert not seen  # decode_kernel_wins was not consulted
