"""Host side of sliding-window attention (no GPU): the four window entries of the C ABI and their refusals, the sliding
masks _padding_mask_interface builds, the routing of _attention_interface and the static caches of sample_generate."""
import ctypes
import re

import pytest
import torch

transformers = pytest.importorskip("transformers")
from transformers.masking_utils import (and_masks, causal_mask_function, or_masks, sdpa_mask,  # noqa: E402
                                        sliding_window_causal_mask_function, sliding_window_overlay)

import bayeformers_amd as bf  # noqa: E402
from bayeformers_amd import _C, ops  # noqa: E402

WINDOW_ENTRIES = ("bf_attention_fwd_gqa_window", "bf_attention_bwd_gqa_window", "bf_attention_decode_gqa_window",
                  "bf_attention_decode_gqa_len_window")


def test_window_symbols_are_declared_exported_and_bound():
    import os

    header = open(os.path.join(os.path.dirname(bf.__file__), os.pardir, "include", "bayeformers_amd.h")).read()
    declared = set(re.findall(r"\b(bf_[a-z0-9_]+)\s*\(", header))
    lib = _C.lib()
    for name in WINDOW_ENTRIES:
        assert name in declared and name in _C.SYMBOLS
        assert getattr(lib, name).restype is ctypes.c_int
        plain = _C.SYMBOLS[name[:-len("_window")]][1]
        # the plain entry's arguments with an int32 window just before scaling
        assert _C.SYMBOLS[name][1] == plain[:-2] + [ctypes.c_int] + plain[-2:]
    assert _C.ABI_VERSION == 6 and ctypes.sizeof(_C.bf_attn_gqa_t) == 96


def _gqa(causal=1, B=1, T=256, H=4, Hkv=2, D=64):
    s = _C.bf_attn_gqa_t(B, T, H, Hkv, D, causal)
    for name in ("q_stride", "k_stride", "v_stride"):
        getattr(s, name)[:] = [T * H * D, D, H * D]
    return s


def _dec(N=1, Tq=1, Tk=64, H=4, Hkv=2, D=64):
    s = _C.bf_attn_decode_t(N, Tq, Tk, H, Hkv, D)
    for name in ("q_stride", "k_stride", "v_stride"):
        getattr(s, name)[:] = [H * Tk * D, Tk * D, D]
    return s


def _call(name, shape, window, kv_len=16):
    lib = _C.lib()
    f = getattr(lib, name)
    if name == "bf_attention_fwd_gqa_window":
        return f(16, 16, 16, None, None, 16, 16, _C.BF_DT_BF16, ctypes.byref(shape), window, 0.125, None)
    if name == "bf_attention_bwd_gqa_window":
        return f(16, 16, 16, None, None, 16, 16, 16, 16, 16, 16, 16, _C.BF_DT_BF16, ctypes.byref(shape), window, 0.125,
                 None)
    if name == "bf_attention_decode_gqa_window":
        return f(16, 16, 16, None, None, 16, 16, _C.BF_DT_BF16, ctypes.byref(shape), window, 0.125, None)
    return f(16, 16, 16, None, None, kv_len, 16, 16, _C.BF_DT_BF16, ctypes.byref(shape), window, 0.125, None)


@pytest.mark.parametrize("name", WINDOW_ENTRIES)
@pytest.mark.parametrize("window", [0, -1, -(2 ** 31)])
def test_window_entries_refuse_a_window_below_one(name, window):
    shape = _gqa() if "gqa_window" in name and "decode" not in name else _dec()
    assert _call(name, shape, window) != 0
    assert b"window" in _C.lib().bf_last_error()


@pytest.mark.parametrize("name", ["bf_attention_fwd_gqa_window", "bf_attention_bwd_gqa_window"])
def test_prefill_window_entries_refuse_non_causal_shapes(name):
    assert _call(name, _gqa(causal=0), 8) != 0
    assert b"causal" in _C.lib().bf_last_error()


@pytest.mark.parametrize("name", ["bf_attention_fwd_gqa_window", "bf_attention_bwd_gqa_window"])
@pytest.mark.parametrize("kw", [dict(T=100), dict(D=96), dict(H=6, Hkv=4), dict(causal=2)])
def test_prefill_window_entries_refuse_unsupported_shapes(name, kw):
    assert _call(name, _gqa(**kw), 8) != 0 and _C.lib().bf_last_error()


@pytest.mark.parametrize("name", ["bf_attention_decode_gqa_window", "bf_attention_decode_gqa_len_window"])
@pytest.mark.parametrize("kw", [dict(D=96), dict(Tq=17, Tk=100), dict(H=6, Hkv=4), dict(Tq=4, Tk=2)])
def test_decode_window_entries_refuse_unsupported_shapes(name, kw):
    assert _call(name, _dec(**kw), 8) != 0 and _C.lib().bf_last_error()


@pytest.mark.parametrize("kv_len", [None, 12])
def test_decode_len_window_needs_an_aligned_length(kv_len):
    assert _call("bf_attention_decode_gqa_len_window", _dec(), 8, kv_len=kv_len) != 0
    assert b"kv_len" in _C.lib().bf_last_error()


# ---------------------------------------------------------------------------------------------------- masks
def _padding(B, n, kind):
    if kind is None:
        return None
    m = torch.ones(B, n, dtype=torch.long)
    if kind == "left":
        m[1, :min(5, n - 1)] = 0
        m[2, :n // 2] = 0
    else:
        m[1, n - min(4, n - 1):] = 0
    return m


def _check(got, ref, W, key_mask_src):
    if ref is None:  # the window hides nothing and nothing is padded: module.is_causal routes the call
        assert got is None
        return
    assert got is not None and got.dtype == torch.bool and torch.equal(got, ref)
    assert got._bf_window == W and not hasattr(got, "_bf_causal")
    if key_mask_src is None:
        assert got._bf_key_mask is None
    else:
        assert torch.equal(got._bf_key_mask, torch.where(key_mask_src.bool(), 0.0, float("-inf")))
        assert got._bf_key_mask.dtype == torch.float32 and got._bf_mask_off.shape == (1,)


WINDOWS = [1, 5, 48, 127, 128, 300]


@pytest.mark.parametrize("W", WINDOWS)
@pytest.mark.parametrize("T", [16, 128, 256])
@pytest.mark.parametrize("pad", [None, "left", "right"])
def test_cache_free_sliding_mask_is_sdpa_mask(W, T, pad):
    B, fn = 3, sliding_window_causal_mask_function(W)
    m = _padding(B, T, pad)
    kw = dict(q_length=T, kv_length=T, mask_function=fn, attention_mask=m, local_size=W)
    got = bf._padding_mask_interface(B, **kw)
    ref = sdpa_mask(batch_size=B, **kw)
    if ref is None and m is not None:  # an all-visible padding mask: sdpa_mask checks it on the host, we do not
        ref = sdpa_mask(batch_size=B, allow_is_causal_skip=False, **kw)
    _check(got, ref, W, m)
    if T > W:
        assert got is not None  # the window hides keys: a mask even without padding


@pytest.mark.parametrize("W", WINDOWS)
@pytest.mark.parametrize("q_length", [1, 2, 7, 16])
@pytest.mark.parametrize("seen", [3, 47, 128, 400])
@pytest.mark.parametrize("pad", [None, "left"])
def test_dynamic_sliding_layer_step_mask_is_sdpa_mask(W, q_length, seen, pad):
    # what a DynamicSlidingWindowLayer reports after `seen` tokens (kv_offset > 0 once the window is full)
    layer = transformers.cache_utils.DynamicSlidingWindowLayer(sliding_window=W)
    layer.cumulative_length = seen
    kv_length, kv_offset = layer.get_mask_sizes(q_length)
    B, fn = 3, sliding_window_causal_mask_function(W)
    m = _padding(B, seen + q_length, pad)
    kw = dict(q_length=q_length, kv_length=kv_length, q_offset=seen, kv_offset=kv_offset, mask_function=fn,
              attention_mask=m, local_size=W)
    got = bf._padding_mask_interface(B, **kw)
    ref = sdpa_mask(batch_size=B, **kw)
    if ref is None and m is not None:
        ref = sdpa_mask(batch_size=B, allow_is_causal_skip=False, **kw)
    _check(got, ref, W, None if m is None else m[:, kv_offset:kv_offset + kv_length])
    if got is not None and q_length < kv_length:
        assert got._bf_decode is True


@pytest.mark.parametrize("W", WINDOWS)
@pytest.mark.parametrize("q_length", [1, 3])
@pytest.mark.parametrize("fill", [0, 9, 200])
@pytest.mark.parametrize("pad", [None, "left"])
def test_fixed_capacity_sliding_mask_is_sdpa_mask(W, q_length, fill, pad):
    B, cap, fn = 2, 240, sliding_window_causal_mask_function(W)
    m = _padding(3, cap, pad)
    m = m[1:] if m is not None else None
    got = bf._padding_mask_interface(B, q_length=q_length, kv_length=cap, q_offset=torch.tensor(fill),
                                     mask_function=fn, attention_mask=m, local_size=W, allow_is_causal_skip=False)
    ref = sdpa_mask(batch_size=B, q_length=q_length, kv_length=cap, q_offset=fill, mask_function=fn, attention_mask=m,
                    local_size=W, allow_is_causal_skip=False)
    _check(got, ref, W, m)
    assert got._bf_decode is True and got._bf_kv_len.tolist() == [fill + q_length]


@pytest.mark.parametrize("fn", [
    and_masks(sliding_window_overlay(8), causal_mask_function, lambda b, h, q, k: k >= 0),  # a third overlay
    and_masks(causal_mask_function, sliding_window_overlay(8)),                           # another order
    or_masks(sliding_window_causal_mask_function(8), lambda b, h, q, k: k < 2),             # or_mask_function
    and_masks(sliding_window_causal_mask_function(8), lambda b, h, q, k: k >= 0),           # packed sequences
])
def test_other_sliding_compositions_go_to_sdpa_mask(fn):
    m = _padding(3, 32, "left")
    kw = dict(q_length=32, kv_length=32, mask_function=fn, attention_mask=m)
    got = bf._padding_mask_interface(3, **kw)
    assert not hasattr(got, "_bf_window") and torch.equal(got, sdpa_mask(batch_size=3, **kw))


def test_vmap_and_a_disagreeing_local_size_go_to_sdpa_mask():
    fn, m = sliding_window_causal_mask_function(8), _padding(3, 32, "left")
    for extra in (dict(use_vmap=True), dict(local_size=9)):
        kw = dict(q_length=32, kv_length=32, mask_function=fn, attention_mask=m, **extra)
        got = bf._padding_mask_interface(3, **kw)
        assert not hasattr(got, "_bf_window") and torch.equal(got, sdpa_mask(batch_size=3, **kw))
    # an offset pair that is not bottom-right aligned
    kw = dict(q_length=4, kv_length=20, q_offset=30, kv_offset=3, mask_function=fn, attention_mask=None)
    got = bf._padding_mask_interface(3, **kw)
    assert not hasattr(got, "_bf_window") and torch.equal(got, sdpa_mask(batch_size=3, **kw))


# ---------------------------------------------------------------------------------------------------- routing
@pytest.fixture
def launches(monkeypatch):
    """Pretend the kernels apply to CPU tensors and record which entry each call takes, with its window."""
    seen = []
    monkeypatch.setattr(ops, "attention_supported", lambda *a, **k: True)
    monkeypatch.setattr(ops, "attention_decode_supported", lambda *a, **k: True)

    def fwd(q, k, v, key_mask, scaling, causal=True, mask_off=None, want_lse=False, window=None):
        seen.append(("gqa", window))
        return torch.zeros(q.shape[0], q.shape[2], q.shape[1], q.shape[3], dtype=q.dtype)

    def dec(q, k, v, key_mask, scaling, mask_off=None, workspace=None, window=None):
        seen.append(("decode", window))
        return torch.zeros(q.shape[0], q.shape[2], q.shape[1], q.shape[3], dtype=q.dtype)

    import transformers.integrations.sdpa_attention as sa

    real_sdpa = sa.sdpa_attention_forward

    def sdpa(*a, **k):
        seen.append(("sdpa", None))
        k.pop("s_aux", None), k.pop("softcap", None)  # (what the framework's function does with them is not at issue)
        return real_sdpa(*a, **k)

    monkeypatch.setattr(ops, "attention_forward_gqa", fwd)
    monkeypatch.setattr(ops, "attention_forward_decode", dec)
    monkeypatch.setattr(sa, "sdpa_attention_forward", sdpa)
    return seen


def _decoder(kind, **kw):
    from transformers import AutoConfig, AutoModelForCausalLM

    base = dict(hidden_size=64, num_attention_heads=2, num_key_value_heads=1, num_hidden_layers=2, intermediate_size=128,
                vocab_size=64, max_position_embeddings=512, attn_implementation="sdpa", head_dim=32)
    base.update(kw)
    cfg = AutoConfig.for_model(kind, **base)
    torch.manual_seed(0)
    model = AutoModelForCausalLM.from_config(cfg).eval()
    assert bf.fuse_attention(model)
    return model


def test_mistral_sliding_layers_route_to_the_window_entries(launches):
    model = _decoder("mistral", sliding_window=48)
    with torch.no_grad():
        out = model(torch.zeros(1, 128, dtype=torch.long), use_cache=True)
        assert launches == [("gqa", 48)] * 2
        del launches[:]
        model(torch.zeros(1, 1, dtype=torch.long), past_key_values=out.past_key_values, use_cache=True)
    assert launches == [("decode", 48)] * 2


def test_qwen2_mixed_layers_route_full_and_sliding_apart(launches):
    model = _decoder("qwen2", sliding_window=48, use_sliding_window=True, max_window_layers=1,
                     layer_types=["full_attention", "sliding_attention"])
    with torch.no_grad():
        model(torch.zeros(1, 128, dtype=torch.long))
    assert launches == [("gqa", None), ("gqa", 48)]


def _sliding_mask(T=128, W=48):
    return bf._padding_mask_interface(1, q_length=T, kv_length=T, mask_function=sliding_window_causal_mask_function(W),
                                      local_size=W)


@pytest.mark.parametrize("kw", [dict(s_aux=torch.zeros(2)), dict(softcap=30.0), dict(sliding_window=64),
                                dict(sliding_window=None)])
def test_sinks_softcap_and_a_disagreeing_window_go_to_sdpa(launches, kw):
    q, mask = torch.zeros(1, 2, 128, 32), _sliding_mask()
    mod = torch.nn.Module()
    mod.is_causal = True
    bf._attention_interface(mod, q, q[:, :1], q[:, :1], mask, **kw)
    assert launches == [("sdpa", None)]
    bf._attention_interface(mod, q, q[:, :1], q[:, :1], mask, sliding_window=48)
    assert launches[-1] == ("gqa", 48)


# ---------------------------------------------------------------------------------------------------- static caches
def _bayesian(kind, **kw):
    return bf.to_bayesian(_decoder(kind, **kw), delta=0.05, freeze=True).eval()


@pytest.mark.parametrize("kind,kw", [
    ("mistral", dict(sliding_window=48)),
    ("qwen2", dict(sliding_window=48, use_sliding_window=True, max_window_layers=1,
                   layer_types=["full_attention", "sliding_attention"])),
    ("qwen3", dict(sliding_window=48, use_sliding_window=True, max_window_layers=0,
                   layer_types=["sliding_attention", "sliding_attention"])),
])
def test_static_cache_of_an_allowed_family_is_all_static_layers(kind, kw):
    from transformers.cache_utils import StaticLayer

    from bayeformers_amd.sampling import _static_cache

    model = _bayesian(kind, **kw)
    assert bf.fuse_attention(model)
    cache = _static_cache(model, 200)
    assert len(cache.layers) == 2
    assert all(type(layer) is StaticLayer and layer.max_cache_len == 200 for layer in cache.layers)
    assert not any(cache.is_sliding)


def test_static_cache_still_refuses_a_llama_with_sliding_layer_types():
    from bayeformers_amd.sampling import _static_cache

    model = _bayesian("llama", layer_types=["sliding_attention", "full_attention"], sliding_window=8)
    assert bf.fuse_attention(model)
    with pytest.raises(ValueError, match="sliding"):
        _static_cache(model, 64)
