"""Host side of pinned_samples(keep_weights="fp8") (no GPU): the header and symbol table of the FP8 entries, the memory figure,
the argument checks, and the torch restatement of the format (tests/fp8_rows_ref.py) on itself."""
import ctypes
import os
import re

import pytest
import torch

import bayeformers_amd as bf
import bayeformers_amd.nn as bnn
from bayeformers_amd import _C
from bayeformers_amd import random as bfr
from bayeformers_amd.plan import kept_weight_bytes
from bayeformers_amd.sampling import sample_generate
from fp8_rows_ref import dequantize_rows, quantize_rows, row_exponent

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"bf_fp8_rows_quantize", "bf_fp8_rows_dequantize", "bf_gemm_nt_skinny_fp8", "bf_gemm_nt_skinny_fp8_workspace_bytes"}


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


def test_fp8_header_prototypes_match_the_ctypes_signatures():
    header = open(os.path.join(ROOT, "include", "bayeformers_amd_fp8.h")).read()
    assert '#include "bayeformers_amd_fp8.h"' in open(os.path.join(ROOT, "include", "bayeformers_amd.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    header = re.sub(r"^\s*#.*$", "", header, flags=re.M)
    parsed = {}
    for ret, name, params in re.findall(r"([A-Za-z_][A-Za-z0-9_ \t\n\*]*?)\b(bf_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", header):
        assert name not in parsed, name
        parsed[name] = (_c_type_class(ret), [_c_type_class(a.strip()) for a in params.split(",")])
    assert set(parsed) == set(_C.FP8_SYMBOLS) == ENTRIES
    for name, (res, args) in _C.FP8_SYMBOLS.items():
        c_res, c_args = parsed[name]
        assert _ctypes_class(res) == c_res and len(args) == len(c_args), name
        for i, (a, c) in enumerate(zip(args, c_args)):
            assert _ctypes_class(a) == c, (name, i, a, c)
    assert not set(_C.FP8_SYMBOLS) & set(_C.SYMBOLS) and len(_C.SYMBOLS) == 90


def test_fp8_symbols_resolve_in_the_built_library():
    lib = _C.lib()
    for name, (res, args) in _C.FP8_SYMBOLS.items():
        fn = getattr(lib, name)
        assert fn.restype is res and fn.argtypes == args
    assert lib.bf_version() == _C.ABI_VERSION == 6


def test_a_library_without_the_fp8_entries_asks_for_a_rebuild(monkeypatch):
    class Old:
        def __getattr__(self, name):
            if name in _C.FP8_SYMBOLS:
                raise AttributeError(name)
            return getattr(real, name)

    real = ctypes.CDLL(_C.LIB_PATH)
    monkeypatch.setattr(_C, "_lib", None)
    monkeypatch.setattr(ctypes, "CDLL", lambda path: Old())
    with pytest.raises(_C.BayeFormersAMDError, match="lacks bf_fp8_rows_quantize.*rebuild"):
        _C.lib()


def test_the_fp8_skinny_kernel_splits_k_as_the_bf16_one():
    """The same split-K rule: the two entries ask for the same fp32 scratch at every shape."""
    lib = _C.lib()
    for S in (1, 4, 10):
        for M in (1, 16, 64):
            for N, K in ((16, 32), (100, 64), (1024, 1024), (200, 4128), (32000, 1024), (1024, 2816), (64, 16384)):
                assert lib.bf_gemm_nt_skinny_fp8_workspace_bytes(S, M, N, K) == lib.bf_gemm_nt_skinny_workspace_bytes(S, M, N, K)
    assert lib.bf_gemm_nt_skinny_fp8_workspace_bytes(1, 4, 200, 4128) > 0


def test_fp8_entries_refuse_before_any_launch():
    lib = _C.lib()
    a = 4096  # an aligned non-NULL address: every call below is refused on its arguments, nothing is launched
    assert lib.bf_fp8_rows_quantize(a, _C.BF_DT_F16, a, a, a, 1, 16, 32, None) == 1
    assert b"bf16" in lib.bf_last_error()
    assert lib.bf_fp8_rows_dequantize(a, a, a, a, _C.BF_DT_F32, 1, 16, 32, None) == 1
    assert b"bf16" in lib.bf_last_error()
    assert lib.bf_gemm_nt_skinny_fp8(a, _C.BF_DT_F16, 64, a, a, a, None, a, _C.BF_DT_F16, 1, 1, 16, 64, 0, None, 0, None) == 1
    assert b"bf16" in lib.bf_last_error()
    assert lib.bf_gemm_nt_skinny_fp8(a, _C.BF_DT_BF16, 48, a, a, a, None, a, _C.BF_DT_BF16, 1, 1, 16, 48, 0, None, 0, None) == 1
    assert b"K % 32" in lib.bf_last_error()
    assert lib.bf_gemm_nt_skinny_fp8(a, _C.BF_DT_BF16, 65 * 64, a, a, a, None, a, _C.BF_DT_BF16, 1, 65, 16, 64, 0, None, 0, None) == 1
    assert b"M <= 64" in lib.bf_last_error()
    assert lib.bf_gemm_nt_skinny_fp8(a, _C.BF_DT_BF16, 4 * 4128, a, a, a, None, a, _C.BF_DT_BF16, 1, 4, 200, 4128, 0, None, 0, None) == 1
    assert b"workspace" in lib.bf_last_error()


# ---------------------------------------------------------------------------------------------------- the memory figure
def _small_llama():
    from transformers import LlamaConfig, LlamaForCausalLM

    cfg = LlamaConfig(hidden_size=64, num_attention_heads=4, num_key_value_heads=2, num_hidden_layers=2, intermediate_size=128,
                      vocab_size=100, max_position_embeddings=64, tie_word_embeddings=False)
    torch.manual_seed(0)
    return bf.to_bayesian(LlamaForCausalLM(cfg).eval(), delta=0.05, freeze=True).eval()


def test_kept_weight_bytes_fp8_hand_count_llama():
    model = _small_llama()
    # per layer: q 64x64, k and v 32x64 (2 heads of 16), o 64x64, gate and up 128x64, down 64x128; lm_head 100x64; no biases
    per_layer = 64 * 64 + 2 * 32 * 64 + 64 * 64 + 2 * 128 * 64 + 64 * 128
    P = 2 * per_layer + 100 * 64
    rows = 2 * (64 + 2 * 32 + 64 + 2 * 128 + 64) + 100  # output rows: one fp32 scale each per sample
    for S in (1, 4, 10):
        assert kept_weight_bytes(model, S, torch.bfloat16, fp8=True) == P * 2 + S * (P + rows * 4)
    # unchanged without the flag
    assert kept_weight_bytes(model, 4, torch.bfloat16) == kept_weight_bytes(model, 4, torch.bfloat16, fp8=False) == 4 * P * 2
    assert kept_weight_bytes(model, 2, torch.float32) == 2 * P * 4
    for dt in (torch.float16, torch.float32):
        with pytest.raises(ValueError, match="bfloat16"):
            kept_weight_bytes(model, 4, dt, fp8=True)


def test_kept_weight_bytes_fp8_counts_biases():
    model = bnn.Model(torch.nn.Sequential(bnn.Linear(32, 16), bnn.Linear(16, 8, bias=False)))
    centre = (16 * 32 + 8 * 16) * 2
    per_sample = (16 * 32 + 16 * 4) + (8 * 16 + 8 * 4) + 16 * 4  # bytes and scales of both layers, the one fp32 bias
    assert kept_weight_bytes(model, 5, torch.bfloat16, fp8=True) == centre + 5 * per_sample
    assert kept_weight_bytes(model, 5, torch.bfloat16) == 5 * ((16 * 32 + 8 * 16) * 2 + 16 * 4)


# ---------------------------------------------------------------------------------------------------- argument checks
def _tiny():
    return bnn.Model(torch.nn.Sequential(bnn.Linear(32, 16))).eval()


def test_keep_weights_fp8_arguments_refused_before_any_reservation():
    model = _tiny()
    bf.manual_seed(1, next_sample=7)
    need = kept_weight_bytes(model, 3, torch.bfloat16, fp8=True)
    assert need != kept_weight_bytes(model, 3, torch.bfloat16)
    with torch.no_grad(), model.monte_carlo(3):
        for bad in ("fp4", "FP8", "", 2, None):
            with pytest.raises(ValueError, match="keep_weights"):
                with model.pinned_samples(keep_weights=bad):
                    pass
        bf.set_compute_dtype("fp32")
        try:
            with pytest.raises(ValueError, match="bfloat16"):
                with model.pinned_samples(keep_weights="fp8"):
                    pass
        finally:
            bf.set_compute_dtype("bf16")
        with pytest.raises(ValueError, match=f"fp8.*{need} bytes.*max_bytes={need - 1}"):
            with model.pinned_samples(keep_weights="fp8", max_bytes=need - 1):
                pass
        # within the budget, but not plannable: the layers are not on a ROCm device
        with pytest.raises(ValueError, match="ROCm"):
            with model.pinned_samples(keep_weights="fp8", max_bytes=need):
                pass
    with pytest.raises(RuntimeError, match="no_grad"):
        with model.pinned_samples(keep_weights="fp8"):
            pass
    assert bfr.STATE.next_sample == 7 and model.__dict__.get("_pinned") is None


def test_sample_generate_passes_fp8_and_its_budget_through():
    model = _small_llama()
    bf.manual_seed(1, next_sample=3)
    ids = torch.zeros(1, 4, dtype=torch.long)
    with torch.no_grad():
        with pytest.raises(ValueError, match="fp8.*max_bytes=1"):
            sample_generate(model, ids, samples=2, max_new_tokens=2, keep_weights="fp8", max_bytes=1)
        with pytest.raises(ValueError, match="keep_weights"):
            sample_generate(model, ids, samples=2, max_new_tokens=2, keep_weights="int8")
    assert bfr.STATE.next_sample == 3


# ---------------------------------------------------------------------------------------------------- the reference on itself
def test_row_exponent_rule():
    # a = m 2^x: m = 0.875 exactly gives x - 9 (a 2^-e = 448), the next fp32 above gives x - 8
    for x in (-20, -3, 0, 1, 9, 30):
        a = torch.tensor([0.875 * 2.0 ** x, 0.5 * 2.0 ** x, 0.9 * 2.0 ** x], dtype=torch.float32)
        a = torch.cat([a, torch.nextafter(a[:1], torch.tensor([float("inf")]))])
        assert row_exponent(a).tolist() == [x - 9, x - 9, x - 8, x - 8]
        e = row_exponent(a).double()
        scaled = a.double() * 2.0 ** -e
        assert bool((scaled <= 448).all()) and bool((scaled * 2 > 448).all())  # the smallest such e
    assert float(torch.tensor(448.0)) * 2.0 ** -int(row_exponent(torch.tensor([448.0]))[0]) == 448.0
    assert row_exponent(torch.tensor([0.0, 2.0 ** -100, 2.0 ** -140, 2.0 ** 100])).tolist() == [0, -64, -64, 64]


def test_zero_deviation_rows_and_the_clamp():
    c = torch.randn(5, 64).to(torch.bfloat16)
    c[3, 7] = 1.0
    w = c[None].repeat(2, 1, 1).clone()
    w[1, 3, 7] = 1.5
    q, scale = quantize_rows(w, c)
    zero_rows = torch.ones(2, 5, dtype=torch.bool)
    zero_rows[1, 3] = False
    assert bool((q[zero_rows] == 0).all()) and bool((scale[zero_rows] == 1.0).all())
    assert torch.equal(dequantize_rows(q, scale, c), w)  # the one nonzero deviation, 0.5, is a power of two: exact
    # -0 survives (W = -0 on a +0 centre), and a deviation past 448 * 2^64 is clamped, never NaN
    c = torch.zeros(1, 32, dtype=torch.bfloat16)
    w = torch.zeros(2, 1, 32, dtype=torch.bfloat16)
    w[0, 0, 1] = -0.0
    w[1, 0, 0], w[1, 0, 1] = 2.0 ** 100, -(2.0 ** 80)
    q, scale = quantize_rows(w, c)
    assert q[0, 0, 1] == 0x80 and scale[0, 0] == 1.0
    assert q[1, 0, 0] == 0x7E and q[1, 0, 1] == 0xFE and scale[1, 0] == 2.0 ** 64  # +-448


def _moped_rows(S, N, K, seed, delta=0.05):
    g = torch.Generator().manual_seed(seed)
    mu = torch.randn(N, K, generator=g) * 0.05
    w = mu[None] + delta * mu.abs()[None] * torch.randn(S, N, K, generator=g)
    return w.to(torch.bfloat16), mu.to(torch.bfloat16)


@pytest.mark.parametrize("S,N,K", [(4, 33, 256), (2, 7, 4128)])
def test_dequantised_weights_stay_within_the_format_bound(S, N, K):
    """|W^ - W16| <= 2^-4 |d| + one bf16 ulp of W^ on MOPED-like rows (sigma = 0.05 |mu|): e4m3 keeps 3 mantissa bits, so
    its rounding is at most 2^-4 relative for normal values — and at most half a subnormal step 2^-10 * scale below that,
    which is 2^-4 of a deviation no smaller than 2^-6 * scale."""
    w, c = _moped_rows(S, N, K, seed=K)
    q, scale = quantize_rows(w, c)
    arg = (w.float() - c.float()[None]) / scale[..., None]
    assert float(arg.abs().max()) <= 448.0
    assert float(arg.abs().amax(-1).min()) > 224.0  # every row uses the top binade
    w_hat = dequantize_rows(q, scale, c)
    d = (w.double() - c.double()[None]).abs()
    ulp = 2.0 ** (torch.frexp(w_hat.float().abs())[1].double() - 8)  # bf16: 8 significant bits
    bound = 2.0 ** -4 * torch.maximum(d, 2.0 ** -6 * scale.double()[..., None]) + ulp
    err = (w_hat.double() - w.double()).abs()
    assert bool((err <= bound).all()), float((err - bound).max())
    # and the point of centring: the error is a small fraction of the posterior's width, not of the weight
    sigma = 0.05 * c.double().abs()[None]
    big = c.double().abs()[None] > 2.0 ** -6
    assert float((err[big.expand_as(err)] / sigma.expand_as(err)[big.expand_as(err)]).mean()) < 0.1
