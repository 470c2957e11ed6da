"""Host side of packed-sequence attention (no GPU): band_bounds, the packed masks _padding_mask_interface builds, the
routing of _attention_interface, the two band entries of the C ABI with their refusals, and the switch."""
import ctypes
import os
import re

import pytest
import torch

transformers = pytest.importorskip("transformers")
from transformers.masking_utils import (and_masks, causal_mask_function, find_packed_sequence_indices,  # noqa: E402
                                        packed_sequence_mask_function, sdpa_mask, sliding_window_causal_mask_function)

import bayeformers_amd as bf  # noqa: E402
from bayeformers_amd import _C, graphs, ops  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------- band_bounds
def _ids(T, bounds):
    """Document indices of a row of T tokens whose documents start at 0 and at each of `bounds`."""
    ids = torch.zeros(T, dtype=torch.long)
    for s in bounds:
        ids[s:] += 1
    return ids


T0 = 300
LAYOUTS = {
    "one": [[]],
    "ones": [list(range(1, T0))],
    "edges": [[1, 127, 128, 129, T0 - 1]],
    "mixed": [[], list(range(1, T0)), [1, 127, 128, 129, T0 - 1], [128], [T0 - 1]],
}


def _brute(ids, W):
    B, T = ids.shape
    seen = torch.zeros(B, T, T, dtype=torch.bool)
    for b in range(B):
        for i in range(T):
            for j in range(i + 1):
                seen[b, i, j] = bool(ids[b, i] == ids[b, j]) and (W is None or i - j < W)
    return seen


BRUTE = {}


def _brute_cached(name, W):
    if (name, W) not in BRUTE:
        BRUTE[(name, W)] = _brute(torch.stack([_ids(T0, b) for b in LAYOUTS[name]]), W)
    return BRUTE[(name, W)]


@pytest.mark.parametrize("W", [None, 1, 5, T0, T0 + 7])
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_band_bounds_against_a_brute_force_loop(name, W):
    ids = torch.stack([_ids(T0, b) for b in LAYOUTS[name]])
    lo, hi = ops.band_bounds(ids, W)
    assert lo.dtype == torch.int32 and hi.dtype == torch.int32 and lo.shape == ids.shape == hi.shape
    assert lo.device == ids.device and hi.device == ids.device
    pos = torch.arange(T0)
    assert bool((lo >= 0).all() and (lo <= pos).all() and (hi >= pos).all() and (hi < T0).all())
    assert bool((lo[:, 1:] >= lo[:, :-1]).all() and (hi[:, 1:] >= hi[:, :-1]).all())  # monotone
    seen = _brute_cached(name, W)
    from_lo = (pos[None, None, :] >= lo[:, :, None]) & (pos[None, None, :] <= pos[None, :, None])
    from_hi = (pos[None, :, None] <= hi[:, None, :]) & (pos[None, None, :] <= pos[None, :, None])
    assert torch.equal(from_lo, seen) and torch.equal(from_hi, seen)  # consistent: both rebuild the same mask


def test_band_bounds_refuses_a_window_below_one():
    with pytest.raises(ValueError, match="window"):
        ops.band_bounds(torch.zeros(1, 4, dtype=torch.long), 0)


# ---------------------------------------------------------------------------------------------------- masks
def _packed_ids(B=3, T=32):
    pos = torch.stack([torch.cat([torch.arange(10), torch.arange(3), torch.arange(T - 13)]),
                       torch.cat([torch.arange(1), torch.arange(T - 1)]),
                       torch.arange(T)])[:B]
    return find_packed_sequence_indices(pos)


def _no_markers(m):
    return not any(hasattr(m, a) for a in ("_bf_window", "_bf_causal", "_bf_decode"))


@pytest.mark.parametrize("W", [None, 1, 5, 8, 64])
def test_packed_masks_are_sdpa_mask_and_carry_the_band(W):
    ids = _packed_ids()
    B, T = ids.shape
    inner = causal_mask_function if W is None else sliding_window_causal_mask_function(W)
    fn = and_masks(inner, packed_sequence_mask_function(ids))
    kw = dict(q_length=T, kv_length=T, mask_function=fn, attention_mask=None, allow_is_causal_skip=False)
    if W is not None:
        kw["local_size"] = W
    got = bf._padding_mask_interface(B, **kw)
    ref = sdpa_mask(batch_size=B, **kw)
    assert got.dtype == torch.bool and got.shape == (B, 1, T, T) and torch.equal(got, ref)
    lo, hi = got._bf_band
    want = ops.band_bounds(ids, W)
    assert torch.equal(lo, want[0]) and torch.equal(hi, want[1]) and got._bf_band_window == W
    assert _no_markers(got)
    pos = torch.arange(T)
    assert torch.equal((pos[None, None, :] >= lo[:, :, None]) & (pos[None, None, :] <= pos[None, :, None]), ref[:, 0])


def _near_misses():
    ids = _packed_ids()
    B, T = ids.shape
    packed = packed_sequence_mask_function(ids)
    base = dict(q_length=T, kv_length=T, attention_mask=None, allow_is_causal_skip=False)
    yield "lambda", dict(base, mask_function=and_masks(causal_mask_function, lambda b, h, q, k: ids[b, q] == ids[b, k]))
    yield "three", dict(base, mask_function=and_masks(causal_mask_function, packed, lambda b, h, q, k: k >= 0))
    yield "swapped", dict(base, mask_function=and_masks(packed, causal_mask_function))
    yield "padding", dict(base, mask_function=and_masks(causal_mask_function, packed),
                          attention_mask=torch.ones(B, T, dtype=torch.long))
    yield "offset", dict(base, mask_function=and_masks(causal_mask_function, packed), q_length=T - 4, q_offset=4)
    yield "ids_shape", dict(base, mask_function=and_masks(causal_mask_function, packed_sequence_mask_function(
        torch.cat([ids, ids[:, -1:]], dim=1))))
    yield "vmap", dict(base, mask_function=and_masks(causal_mask_function, packed), use_vmap=True)
    yield "local_size", dict(base, mask_function=and_masks(sliding_window_causal_mask_function(8), packed), local_size=9)
    yield "local_size_no_window", dict(base, mask_function=and_masks(causal_mask_function, packed), local_size=9)


@pytest.mark.parametrize("name", ["lambda", "three", "swapped", "padding", "offset", "ids_shape", "vmap", "local_size",
                                  "local_size_no_window"])
def test_near_misses_go_to_sdpa_mask(name):
    ids = _packed_ids()
    exact = bf._padding_mask_interface(3, q_length=32, kv_length=32, attention_mask=None, allow_is_causal_skip=False,
                                       mask_function=and_masks(causal_mask_function, packed_sequence_mask_function(ids)))
    assert hasattr(exact, "_bf_band")  # the control: the composition itself is recognised
    kw = dict(_near_misses())[name]
    got = bf._padding_mask_interface(3, **kw)
    assert not hasattr(got, "_bf_band") and _no_markers(got)
    assert torch.equal(got, sdpa_mask(batch_size=3, **kw))


# ---------------------------------------------------------------------------------------------------- routing
@pytest.fixture
def launches(monkeypatch):
    """Pretend the kernels apply to CPU tensors and record which entry each call takes."""
    seen = []
    monkeypatch.setattr(ops, "attention_supported", lambda *a, **k: True)

    def out_of(q):
        return torch.zeros(q.shape[0], q.shape[2], q.shape[1], q.shape[3], dtype=q.dtype)

    def band_fwd(q, k, v, lo, scaling, want_lse=False):
        seen.append(("band", lo))
        out = out_of(q)
        return (out, torch.zeros(q.shape[0], q.shape[1], q.shape[2])) if want_lse else out

    def band_bwd(q, k, v, lo, hi, out, grad_out, lse, scaling):
        seen.append(("band_bwd", hi))
        return torch.zeros_like(out), out_of(k), out_of(v)

    def plain_fwd(q, k, v, key_mask, scaling, causal=True, mask_off=None, want_lse=False, window=None):
        seen.append(("gqa", window))
        return out_of(q)

    import transformers.integrations.sdpa_attention as sa

    real_sdpa = sa.sdpa_attention_forward

    def sdpa(*a, **k):
        seen.append(("sdpa", a[4]))
        k.pop("s_aux", None), k.pop("softcap", None)
        return real_sdpa(*a, **k)

    def eager(module, query, key, value, attention_mask, dropout, scaling, softcap):
        seen.append(("eager", attention_mask))
        return out_of(query)

    monkeypatch.setattr(ops, "attention_forward_gqa_band", band_fwd)
    monkeypatch.setattr(ops, "attention_backward_gqa_band", band_bwd)
    monkeypatch.setattr(ops, "attention_forward_gqa", plain_fwd)
    monkeypatch.setattr(sa, "sdpa_attention_forward", sdpa)
    monkeypatch.setattr(bf, "_softcap_eager", eager)
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


DOCS = (100, 28, 128)


def _packed_inputs():
    T = sum(DOCS)
    pos = torch.cat([torch.arange(n) for n in DOCS])[None]
    ids = torch.cat([torch.full((n,), i) for i, n in enumerate(DOCS)])[None]
    return torch.zeros(1, T, dtype=torch.long), pos, ids


@pytest.mark.parametrize("kind,kw,W", [("llama", {}, None), ("mistral", dict(sliding_window=100), 100)])
def test_packed_position_ids_reach_the_band_entry_in_every_layer(launches, kind, kw, W):
    model = _decoder(kind, **kw)
    tokens, pos, ids = _packed_inputs()
    with torch.no_grad():
        model(tokens, position_ids=pos, use_cache=False)  # (with a cache transformers does not look for packing)
    lo = ops.band_bounds(ids, W)[0]
    assert [name for name, _ in launches] == ["band"] * 2
    assert all(torch.equal(got, lo) for _, got in launches)


def _packed_mask(W=None, T=128):
    ids = torch.cat([torch.zeros(40, dtype=torch.long), torch.ones(T - 40, dtype=torch.long)])[None]
    inner = causal_mask_function if W is None else sliding_window_causal_mask_function(W)
    kw = {} if W is None else dict(local_size=W)
    return bf._padding_mask_interface(1, q_length=T, kv_length=T, allow_is_causal_skip=False,
                                      mask_function=and_masks(inner, packed_sequence_mask_function(ids)), **kw)


def _module():
    mod = torch.nn.Module()
    mod.is_causal = True
    return mod.eval()


@pytest.mark.parametrize("kw", [dict(dropout=0.1), dict(s_aux=torch.zeros(2)), dict(sliding_window=64), dict(softcap=30.0)])
def test_what_the_band_entry_does_not_take_goes_to_sdpa_with_the_dense_mask(launches, kw):
    q, mask = torch.zeros(1, 2, 128, 32), _packed_mask()
    bf._attention_interface(_module(), q, q[:, :1], q[:, :1], mask, **kw)
    assert [name for name, _ in launches] == ["sdpa"] and launches[0][1] is mask
    del launches[:]
    bf._attention_interface(_module(), q, q[:, :1], q[:, :1], mask, sliding_window=None)
    assert [name for name, _ in launches] == ["band"]


def test_a_windowed_band_wants_the_same_sliding_window(launches):
    q, mask = torch.zeros(1, 2, 128, 32), _packed_mask(W=48)
    bf._attention_interface(_module(), q, q[:, :1], q[:, :1], mask, sliding_window=48)
    bf._attention_interface(_module(), q, q[:, :1], q[:, :1], mask)
    bf._attention_interface(_module(), q, q[:, :1], q[:, :1], mask, sliding_window=None)
    assert [name for name, _ in launches] == ["band", "band", "sdpa"]


def test_the_switch_off_is_the_routing_of_before(launches):
    q, mask = torch.zeros(1, 2, 128, 32), _packed_mask()
    bf.packed_attention(False)
    try:
        bf._attention_interface(_module(), q, q[:, :1], q[:, :1], mask)
    finally:
        bf.packed_attention(True)
    assert [name for name, _ in launches] == ["sdpa"] and launches[0][1] is mask


def test_softcap_with_its_switch_on_runs_the_eager_chain_over_the_dense_mask(launches):
    q, mask = torch.zeros(1, 2, 128, 32), _packed_mask()
    bf.softcap_attention(True)
    try:
        bf._attention_interface(_module(), q, q[:, :1], q[:, :1], mask, softcap=30.0)
    finally:
        bf.softcap_attention(False)
    assert [name for name, _ in launches] == ["eager"] and launches[0][1] is mask


def test_a_gradient_goes_through_the_band_autograd_function(launches):
    q, mask = torch.zeros(1, 2, 128, 32, requires_grad=True), _packed_mask(W=48)
    k = torch.zeros(1, 1, 128, 32, requires_grad=True)
    out, _ = bf._attention_interface(_module(), q, k, k, mask)
    assert type(out.grad_fn).__name__ == "AttentionGqaBandFnBackward"
    out.sum().backward()
    assert [name for name, _ in launches] == ["band", "band_bwd"]
    lo, hi = mask._bf_band
    assert launches[0][1] is lo and launches[1][1] is hi
    assert q.grad.shape == q.shape and k.grad.shape == k.shape


def test_a_ragged_length_follows_the_ragged_switch(launches):
    q, mask = torch.zeros(1, 2, 100, 32), _packed_mask(T=100)
    bf._attention_interface(_module(), q, q[:, :1], q[:, :1], mask)
    bf.ragged_attention(False)
    try:
        bf._attention_interface(_module(), q, q[:, :1], q[:, :1], mask)
    finally:
        bf.ragged_attention(True)
    assert [name for name, _ in launches] == ["band", "sdpa"]


# ---------------------------------------------------------------------------------------------------- header, bindings
def _c_type_class(decl):
    if "*" in decl:
        return ("pointer", 8)
    words = [w for w in re.findall(r"[A-Za-z_][A-Za-z0-9_]*", decl) if w != "const"]
    table = {"float": ("float", 4), "double": ("float", 8), "int": ("int", 4), "int32_t": ("int", 4), "uint32_t": ("int", 4),
             "int64_t": ("int", 8), "uint64_t": ("int", 8), "size_t": ("int", 8), "void": ("void", 0)}
    assert words and words[0] in table, f"unknown C type in {decl!r}"
    return table[words[0]]


def _ctypes_class(t):
    if t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer):
        return ("pointer", ctypes.sizeof(t))
    code = getattr(t, "_type_", None)
    if code in ("f", "d"):
        return ("float", ctypes.sizeof(t))
    assert code in tuple("bBhHiIlLqQ"), f"unknown ctypes type {t!r}"
    return ("int", ctypes.sizeof(t))


def test_packed_header_prototypes_match_the_ctypes_signatures():
    header = open(os.path.join(ROOT, "include", "bayeformers_amd_packed.h")).read()
    assert '#include "bayeformers_amd_packed.h"' in open(os.path.join(ROOT, "include", "bayeformers_amd.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    header = re.sub(r"^\s*#.*$", "", header, flags=re.M)
    parsed = {}
    for ret, name, params in re.findall(r"([A-Za-z_][A-Za-z0-9_ \t\n\*]*?)\b(bf_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", header):
        assert name not in parsed, name
        parsed[name] = (_c_type_class(ret), [_c_type_class(a.strip()) for a in params.split(",")])
    assert set(parsed) == set(_C.PACKED_SYMBOLS) == {"bf_attention_fwd_gqa_band", "bf_attention_bwd_gqa_band"}
    for name, (res, args) in _C.PACKED_SYMBOLS.items():
        c_res, c_args = parsed[name]
        assert _ctypes_class(res) == c_res and len(args) == len(c_args), name
        for i, (a, c) in enumerate(zip(args, c_args)):
            assert _ctypes_class(a) == c, (name, i, a, c)
    assert not set(_C.PACKED_SYMBOLS) & set(_C.SYMBOLS) and len(_C.SYMBOLS) == 90


def test_packed_symbols_resolve_in_the_built_library():
    lib = _C.lib()
    for name, (res, args) in _C.PACKED_SYMBOLS.items():
        fn = getattr(lib, name)
        assert fn.restype is res and fn.argtypes == args
    assert lib.bf_version() == _C.ABI_VERSION == 6 and ctypes.sizeof(_C.bf_attn_gqa_t) == 96


def test_a_library_without_the_entries_asks_for_a_rebuild(monkeypatch):
    class Old:
        def __getattr__(self, name):
            if name in _C.PACKED_SYMBOLS:
                raise AttributeError(name)
            return getattr(real, name)

    real = ctypes.CDLL(_C.LIB_PATH)
    monkeypatch.setattr(_C, "_lib", None)
    monkeypatch.setattr(ctypes, "CDLL", lambda path: Old())
    with pytest.raises(_C.BayeFormersAMDError, match="rebuild"):
        _C.lib()


def _gqa(causal=1, B=1, T=256, H=4, Hkv=2, D=64):
    s = _C.bf_attn_gqa_t(B, T, H, Hkv, D, causal)
    for name in ("q_stride", "k_stride", "v_stride"):
        getattr(s, name)[:] = [T * H * D, D, H * D]
    return s


def _call(name, shape, lo=16, hi=16, q=16):
    f = getattr(_C.lib(), name)
    if name == "bf_attention_fwd_gqa_band":
        return f(q, 16, 16, lo, 16, 16, _C.BF_DT_BF16, ctypes.byref(shape), 0.125, None)
    return f(q, 16, 16, lo, hi, 16, 16, 16, 16, 16, 16, 16, _C.BF_DT_BF16, ctypes.byref(shape), 0.125, None)


ENTRIES = ["bf_attention_fwd_gqa_band", "bf_attention_bwd_gqa_band"]


@pytest.mark.parametrize("name", ENTRIES)
def test_band_entries_refuse_missing_bounds(name):
    assert _call(name, _gqa(), lo=None) == 1
    assert b"d_lo" in _C.lib().bf_last_error()
    if name == "bf_attention_bwd_gqa_band":
        assert _call(name, _gqa(), hi=None) == 1
        assert b"d_hi" in _C.lib().bf_last_error()
    assert _call(name, _gqa(), lo=18) == 1  # not 4-byte aligned
    assert b"aligned" in _C.lib().bf_last_error()


@pytest.mark.parametrize("name", ENTRIES)
@pytest.mark.parametrize("causal", [0, 2])
def test_band_entries_refuse_non_causal_shapes(name, causal):
    assert _call(name, _gqa(causal=causal)) == 1
    assert b"causal" in _C.lib().bf_last_error()


@pytest.mark.parametrize("name", ENTRIES)
@pytest.mark.parametrize("kw", [dict(D=96), dict(H=6, Hkv=4), dict(T=0), dict(B=70000)])
def test_band_entries_refuse_what_the_plain_entries_refuse(name, kw):
    assert _call(name, _gqa(**kw)) == 1 and _C.lib().bf_last_error()
    assert _call(name, _gqa(), q=None) == 1 and b"NULL" in _C.lib().bf_last_error()
    assert _call(name, _gqa(), q=8) == 1 and b"aligned" in _C.lib().bf_last_error()


# ---------------------------------------------------------------------------------------------------- the switch
def test_the_switch_is_on_by_default_follows_the_environment_and_is_baked(monkeypatch):
    assert bf.packed_attention_enabled()  # on by default (every test that flips it flips it back)
    assert set(ops.PACKED_CALLS) == {"fwd", "bwd"}
    model = bf.nn.Model(bf.nn.Linear(8, 8))
    on = graphs.baked_state(model)
    assert graphs.still_valid(model, on)
    bf.packed_attention(False)
    try:
        assert not bf.packed_attention_enabled()
        off = graphs.baked_state(model)
        assert on != off and not graphs.still_valid(model, on) and graphs.still_valid(model, off)
    finally:
        bf.packed_attention(True)
    assert graphs.still_valid(model, on)
    monkeypatch.setenv("BF_NO_PACKED_ATTENTION", "1")
    assert not bf.packed_attention_enabled() and graphs.baked_state(model) == off
    monkeypatch.delenv("BF_NO_PACKED_ATTENTION")
    assert bf.packed_attention_enabled()
    # the other counters keep their keys: the band launches count in PACKED_CALLS alone
    assert set(ops.GQA_CALLS) == {"fwd", "bwd", "fwd_window", "bwd_window"}
    assert set(ops.SOFTCAP_CALLS) == {"fwd", "bwd", "decode", "decode_len"}
    assert set(ops.DECODE_CALLS) == {"fwd", "len", "window", "len_window"}
