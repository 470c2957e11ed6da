"""Host side of the any-length encoder attention (no GPU): the predicate, the switch and what a captured forward bakes in,
the symbol table and its header, the refusals of the entries before any launch, and the keep-mask helper of
tests/encoder_any_ref.py against the oracle's mask at the lengths the existing entries take."""
import os
import re

import numpy as np
import pytest
import torch

import bayeformers_amd as bf
from bayeformers_amd import _C, graphs, ops
from encoder_any_ref import attention_keep_mask_any, keep_words_any, padded_length
from oracle import bayes_oracle as bo
from test_kept_fp8_cpu import _c_type_class, _ctypes_class

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"bf_attention_fwd_any", "bf_attention_fwd_any_dropout", "bf_attention_fwd_any_rows", "bf_attention_bwd_any",
           "bf_attention_bwd_any_dropout"}
SIBLING = {"bf_attention_fwd_any": "bf_attention_fwd", "bf_attention_fwd_any_dropout": "bf_attention_fwd_dropout",
           "bf_attention_fwd_any_rows": "bf_attention_fwd_rows", "bf_attention_bwd_any": "bf_attention_bwd",
           "bf_attention_bwd_any_dropout": "bf_attention_bwd_dropout"}
PTR = 4096  # an aligned non-NULL address: every call below is refused on its arguments, nothing is launched


@pytest.fixture(autouse=True)
def _switch_off_again():
    yield
    bf.encoder_ragged_attention(False)


class _AsDevice:
    """a CPU tensor that says is_cuda: the shape / stride / alignment part of the predicates without a GPU"""

    def __init__(self, t):
        self._t = t

    is_cuda = True

    def __getattr__(self, name):
        return getattr(self._t, name)


def _qkv(T, D=64, H=4, B=2, pad=0, dtype=torch.bfloat16):
    return [torch.zeros(B, T, H * D + pad, dtype=dtype)[:, :, :H * D].view(B, T, H, D).transpose(1, 2) for _ in range(3)]


# ------------------------------------------------------------------------------------------------------------- predicate
@pytest.mark.parametrize("T", [1, 100, 128, 200])
def test_predicate_takes_any_length(T):
    q, k, v = _qkv(T)
    assert not ops.attention_any_supported(q, k, v)  # a CPU tensor never runs the kernels
    assert ops.attention_any_supported(*[_AsDevice(t) for t in (q, k, v)])
    # and attention_supported keeps its limit: the any-length route is taken where it refuses
    assert ops.attention_supported(*[_AsDevice(t) for t in (q, k, v)]) is (T == 128)


def test_predicate_refuses_what_the_kernels_do_not_take():
    dev = lambda ts: [_AsDevice(t) for t in ts]
    assert not ops.attention_any_supported(*dev(_qkv(100, D=96)))                 # head size
    odd = _qkv(100, pad=4)
    assert odd[0].stride(2) % 8 == 4
    assert not ops.attention_any_supported(*dev(odd))                             # token stride no multiple of 8
    assert not ops.attention_any_supported(*dev(_qkv(100, pad=8)))                # a padded row: not the packed view
    assert not ops.attention_any_supported(*dev(_qkv(0)))                         # no token at all
    assert not ops.attention_any_supported(*dev(_qkv(100, dtype=torch.float32)))  # dtype
    q, k, v = _qkv(100)
    assert not ops.attention_any_supported(*dev([q, k[:, :2], v[:, :2]]))         # grouped K / V heads: the causal route's


# ---------------------------------------------------------------------------------------------------------------- switch
def test_switch_exists_is_off_by_default_flips_and_is_baked(monkeypatch):
    monkeypatch.delenv("BF_ENCODER_RAGGED_ATTENTION", raising=False)
    model = torch.nn.Linear(2, 2)
    assert not bf.encoder_ragged_attention_enabled()
    off = graphs.baked_state(model)
    assert graphs.still_valid(model, off)
    bf.encoder_ragged_attention()
    assert bf.encoder_ragged_attention_enabled()
    on = graphs.baked_state(model)
    assert on != off and not graphs.still_valid(model, off) and graphs.still_valid(model, on)
    bf.encoder_ragged_attention(False)
    assert not bf.encoder_ragged_attention_enabled() and graphs.still_valid(model, off)
    monkeypatch.setenv("BF_ENCODER_RAGGED_ATTENTION", "1")
    assert bf.encoder_ragged_attention_enabled() and graphs.baked_state(model) == on


def test_the_other_switches_keep_their_places_in_the_baked_state():
    model = torch.nn.Linear(2, 2)
    base = graphs.baked_state(model)
    assert len(base) == 11 and base[10] is False
    bf.chunked_attention(True)
    try:
        assert graphs.baked_state(model)[9] is True and graphs.baked_state(model)[10] is False
    finally:
        bf.chunked_attention(False)


def test_counters_exist():
    assert set(ops.ENCODER_ANY_CALLS) == {"fwd", "bwd", "rows"}
    assert all(isinstance(n, int) for n in ops.ENCODER_ANY_CALLS.values())


# ------------------------------------------------------------------------------------------------------ header, bindings
def test_symbol_table_lists_the_five_entries_with_their_siblings_arguments():
    assert set(_C.ENCODER_ANY_SYMBOLS) == ENTRIES
    for name, (res, args) in _C.ENCODER_ANY_SYMBOLS.items():
        s_res, s_args = _C.SYMBOLS[SIBLING[name]]
        assert res is s_res and list(args) == list(s_args), name
    others = [_C.SYMBOLS, _C.SOFTCAP_SYMBOLS, _C.FAMILY_BLOCK_SYMBOLS, _C.FAMILY_BLOCK_BWD_SYMBOLS, _C.PACKED_SYMBOLS,
              _C.FP8_SYMBOLS, _C.KV8_SYMBOLS, _C.CHUNK_SYMBOLS]
    for table in others:
        assert not set(_C.ENCODER_ANY_SYMBOLS) & set(table)
    assert len(_C.SYMBOLS) == 90 and _C.ABI_VERSION == 6
    main = open(os.path.join(ROOT, "include", "bayeformers_amd.h")).read()
    assert not any(name in main for name in ENTRIES)  # (the main header is as it was)


def test_header_prototypes_match_the_ctypes_signatures():
    header = open(os.path.join(ROOT, "include", "bayeformers_amd_encoder_any.h")).read()
    assert '#include "bayeformers_amd.h"' in header
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    header = re.sub(r"^\s*#.*$", "", header, flags=re.M)
    parsed = {}
    for ret, name, params in re.findall(r"([A-Za-z_][A-Za-z0-9_ \t\n\*]*?)\b(bf_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", header):
        assert name not in parsed, name
        parsed[name] = (_c_type_class(ret), [_c_type_class(a.strip()) for a in params.split(",")])
    assert set(parsed) == ENTRIES
    for name, (res, args) in _C.ENCODER_ANY_SYMBOLS.items():
        c_res, c_args = parsed[name]
        assert _ctypes_class(res) == c_res and len(args) == len(c_args), name
        for i, (a, c) in enumerate(zip(args, c_args)):
            assert _ctypes_class(a) == c, (name, i, a, c)


def test_symbols_resolve_in_the_built_library():
    lib = _C.lib()
    for name, (res, args) in _C.ENCODER_ANY_SYMBOLS.items():
        fn = getattr(lib, name)
        assert fn.restype is res and fn.argtypes == args
    assert lib.bf_version() == _C.ABI_VERSION


# ------------------------------------------------------------------------------------------------------------- refusals
def _fwd(T=100, D=64, stride=None, H=2, B=2, q=PTR, mask=None, dtype=None):
    dtype = _C.BF_DT_BF16 if dtype is None else dtype
    return _C.lib().bf_attention_fwd_any(q, PTR, PTR, mask, None, PTR, None, dtype, B, T, H, D, H * 64 if stride is None else stride,
                                         0.125, None)


def _bwd(T=100, D=64, stride=None, H=2, B=2, lse=PTR, mask=None):
    return _C.lib().bf_attention_bwd_any(PTR, PTR, PTR, mask, None, PTR, PTR, lse, PTR, PTR, PTR, PTR, _C.BF_DT_BF16, B, T, H, D,
                                         H * 64 if stride is None else stride, 0.125, None)


def test_the_entries_refuse_bad_arguments_before_any_launch():
    lib = _C.lib()
    cases = [
        (lambda: _fwd(T=0), b"must be positive"), (lambda: _bwd(T=0), b"must be positive"),
        (lambda: _fwd(D=96), b"head size"), (lambda: _bwd(D=96), b"head size"),
        (lambda: _fwd(stride=2 * 64 + 4), b"token stride"), (lambda: _bwd(stride=2 * 64 + 4), b"token stride"),
        (lambda: _fwd(stride=64), b"token stride"),
        (lambda: _fwd(q=PTR + 2), b"16-byte aligned"),
        (lambda: _fwd(mask=PTR + 2), b"mask must be 4-byte aligned"), (lambda: _bwd(mask=PTR + 2), b"mask must be 4-byte aligned"),
        (lambda: _bwd(lse=PTR + 2), b"lse and delta must be 4-byte aligned"),
        (lambda: _fwd(B=65536), b"exceeds the grid"),
        (lambda: _fwd(dtype=_C.BF_DT_F32), b"dtype"),
        (lambda: _fwd(q=None), b"NULL"),
        (lambda: lib.bf_attention_fwd_any_rows(PTR, PTR, PTR, None, None, PTR, _C.BF_DT_BF16, 2, 100, 2, 64, 128, 17, 0.125, None),
         b"q_rows=17"),
        (lambda: lib.bf_attention_fwd_any_rows(PTR, PTR, PTR, None, None, PTR, _C.BF_DT_BF16, 2, 5, 2, 64, 128, 8, 0.125, None),
         b"exceeds T"),
        (lambda: lib.bf_attention_fwd_any_dropout(PTR, PTR, PTR, None, None, PTR, None, _C.BF_DT_BF16, 2, 100, 2, 64, 128, 0.125,
                                                  1.0, 1, 1, 1, 0, None, None, None), b"p must be in"),
        (lambda: lib.bf_attention_bwd_any_dropout(PTR, PTR, PTR, None, None, PTR, PTR, PTR, PTR, PTR, PTR, PTR, _C.BF_DT_BF16, 2,
                                                  100, 2, 64, 128, 0.125, 0.1, None, None), b"keep bits are needed"),
        # at a multiple of 128 the sibling's own checks answer, in its own words
        (lambda: _fwd(T=256, mask=PTR + 4), b"bf_attention_fwd: mask must be 16-byte aligned"),
        (lambda: _bwd(T=256, mask=PTR + 4), b"bf_attention_bwd: mask must be 16-byte aligned"),
    ]
    for i, (call, text) in enumerate(cases):
        rc = call()
        err = lib.bf_last_error()
        assert rc == 1, i
        assert err and text in err, (i, err)


def test_the_python_rows_wrapper_refuses_more_rows_than_tokens():
    q, k, v = _qkv(5)
    with pytest.raises(_C.BayeFormersAMDError, match="q_rows=8"):
        ops.attention_forward_rows_any(q, k, v, None, 0.125, q_rows=8)


# ------------------------------------------------------------------------------------------------------ keep-mask helper
@pytest.mark.parametrize("T", [128, 256])
def test_keep_mask_helper_is_the_oracles_at_multiples_of_128(T):
    B, H, p, seed, call, site = 2, 3, 0.1, 0x5EED, 7, 11
    mine = attention_keep_mask_any(B, H, T, p, seed, call, site)
    assert mine.dtype == np.uint8 and np.array_equal(mine, bo.attention_keep_mask(B, H, T, p, seed, call, site))
    assert np.array_equal(attention_keep_mask_any(B, H, T, p, seed, call, site, with_pad_keys=True), mine)


def test_keep_mask_helper_at_a_ragged_length():
    B, H, T, p, seed, call, site = 2, 2, 100, 0.25, 0x5EED, 3, 5
    keep = attention_keep_mask_any(B, H, T, p, seed, call, site)
    assert keep.shape == (B, H, T, T) and padded_length(T) == 128
    assert abs(float(keep.mean()) - 0.75) < 0.01
    full = attention_keep_mask_any(B, H, T, p, seed, call, site, with_pad_keys=True)
    assert full.shape == (B, H, T, 128) and np.array_equal(full[..., :T], keep)
    # a query row's 16 groups are consecutive, and (sequence, head) slabs follow each other: T * (Tp/32) * 4 groups each
    g = bo.dropout_keep(((1 * H + 1) * T + 7) * 16, 16, p, seed, call, site).reshape(4, 4, 2, 4)  # [c, lg, e, j]
    row = np.ascontiguousarray(g.transpose(0, 2, 1, 3)).reshape(128)                                # key = (2c + e)*16 + 4 lg + j
    assert np.array_equal(full[1, 1, 7], row)
    # another call number draws another mask; a shard's first_group continues the whole batch's numbering
    assert not np.array_equal(keep, attention_keep_mask_any(B, H, T, p, seed, call + 1, site))
    second = attention_keep_mask_any(1, H, T, p, seed, call, site, first_group=1 * H * T * 16)
    assert np.array_equal(second[0], keep[1])
    words = keep_words_any(torch.from_numpy(full))
    assert words.shape == (B, H, T, 4) and words.dtype == torch.int32
    assert int(words[1, 1, 7, 2]) & 1 == int(full[1, 1, 7, 8])  # word lg = 2, bit 0: c = 0, e = 0, j = 0 -> key 4 lg


def test_dropout_first_group_of_a_shard_counts_padded_key_groups():
    d = ops.Dropout(0.1, 1, 1, 1, origin=(1, 1))
    B, H, T = 2, 2, 100
    assert d.first_group(B, H * T * ops._keep_words_any(T) * 4) == B * H * T * 16
    assert ops._keep_words_any(128) == 4 and ops._keep_words_any(129) == 8 and ops._keep_words_any(1) == 4
