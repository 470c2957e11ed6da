"""Logit soft-capping (Gemma 2) on the causal attention kernels, the part that needs no GPU: the float64 restatement
(tests/softcap_ref.py) against autograd and against the restatements the other kernels' tests use, the three C entries'
refusals, the routing of `_causal_attention` under `softcap_attention()`, the capped fallback against the model's own eager
chain, a tiny Gemma 2, the static cache's guard and the captured state."""
import ctypes

import pytest
import torch

transformers = pytest.importorskip("transformers")

import bayeformers_amd as bf  # noqa: E402
import softcap_ref  # noqa: E402
from bayeformers_amd import _C, ops  # noqa: E402

REAL_DECODE_SUPPORTED = ops.attention_decode_supported  # (the routing fixture replaces the module's attribute)


@pytest.fixture(autouse=True)
def _switch_off_again(monkeypatch):
    monkeypatch.delenv("BF_SOFTCAP_ATTENTION", raising=False)
    bf.softcap_attention(False)
    yield
    bf.softcap_attention(False)


# ---------------------------------------------------------------------------------------------------- the restatement
def _qkv(B, H, Hkv, Tq, Tk, D, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, H, Tq, D, generator=g, dtype=torch.float64) * scale
    k, v = (torch.randn(B, Hkv, Tk, D, generator=g, dtype=torch.float64) for _ in range(2))
    return q, k, v, torch.randn(B, Tq, H, D, generator=g, dtype=torch.float64)


def _key_mask(B, Tk, pad):
    m = torch.zeros(B, Tk, dtype=torch.float64)
    if pad > 0:
        m[1, :pad] = float("-inf")  # left padding: rows with no visible key
    elif pad < 0:
        m[1, Tk + pad:] = float("-inf")
    return m


@pytest.mark.parametrize("softcap,qscale", [(None, 1.0), (2.0, 1.0), (50.0, 32.0)], ids=["plain", "cap2", "cap50_q32"])
@pytest.mark.parametrize("Tq,Tk,W,pad", [(19, 19, None, 0), (19, 19, 5, 6), (19, 19, 1, -4), (7, 23, None, 5), (7, 23, 4, 0)])
def test_closed_form_gradients_are_autograds(softcap, qscale, Tq, Tk, W, pad):
    B, H, Hkv, D = 2, 4, 2, 8
    q, k, v, go = _qkv(B, H, Hkv, Tq, Tk, D, seed=Tq + Tk + (W or 0), scale=qscale)
    mask = _key_mask(B, Tk, pad) if pad else None
    got = softcap_ref.reference(q, k, v, mask, D ** -0.5, W, softcap, go)
    want = softcap_ref.autograd_reference(q, k, v, mask, D ** -0.5, W, softcap, go)
    for n, a, b in zip(("out", "lse", "dq", "dk", "dv"), got, want):
        assert a.shape == b.shape, n
        assert torch.equal(torch.isfinite(a), torch.isfinite(b)), n
        fin = torch.isfinite(a)
        assert (a[fin] - b[fin]).abs().max().item() <= 1e-12 * max(1.0, b[fin].abs().max().item()), n
    if pad > 0 and Tq == Tk:  # the dead rows: output 0, lse = +inf, zero gradients
        assert (got[1][1, :, :pad] == float("inf")).all() and (got[0][1, :pad] == 0).all() and (got[2][1, :pad] == 0).all()


@pytest.mark.parametrize("W,pad", [(None, 0), (None, 6), (None, -4), (5, 6), (1, 0), (40, -4)])
def test_without_a_cap_it_is_the_restatement_the_other_kernels_are_held_to(W, pad):
    from test_gpu_causal_attention import reference as causal_reference
    from test_gpu_sliding_window import reference as window_reference

    B, H, Hkv, T, D = 2, 4, 2, 21, 8
    q, k, v, go = _qkv(B, H, Hkv, T, T, D, seed=3 + (W or 0))
    mask = _key_mask(B, T, pad) if pad else None
    got = softcap_ref.reference(q, k, v, mask, D ** -0.5, W, None, go)
    if W is None:
        want = causal_reference(q, k, v, mask, D ** -0.5, True, go)
    else:
        want = window_reference(q, k, v, mask, D ** -0.5, W, go)
    for n, a, b in zip(("out", "lse", "dq", "dk", "dv"), got, want):
        assert a.shape == b.shape and torch.equal(torch.isfinite(a), torch.isfinite(b)), n
        fin = torch.isfinite(a)
        assert (a[fin] - b[fin]).abs().max().item() <= 1e-13 * max(1.0, b[fin].abs().max().item()), n


def test_the_cap_is_not_a_detail_on_unit_logits():
    """The GPU test's choice of cap: softcap = 2 moves every quantity by tens of percent on randn inputs, 50 does not."""
    B, H, Hkv, T, D = 2, 4, 2, 64, 16
    q, k, v, go = _qkv(B, H, Hkv, T, T, D, seed=9)
    plain = softcap_ref.reference(q, k, v, None, D ** -0.5, None, None, go)
    for cap, lo, hi in ((2.0, 0.05, 10.0), (50.0, 0.0, 2e-2)):
        capped = softcap_ref.reference(q, k, v, None, D ** -0.5, None, cap, go)
        for i in (0, 2, 3, 4):
            d = (capped[i] - plain[i]).abs().max().item() / plain[i].abs().max().item()
            assert lo < d < hi, (cap, i, d)


# ---------------------------------------------------------------------------------------------------- the C entries
PTR = 0x10000  # a 16-byte aligned non-NULL address: every refusal below comes before anything is launched or read


def _gqa_shape(D=64, causal=1, T=128):
    s = _C.bf_attn_gqa_t(1, T, 4, 2, D, causal)
    for name in ("q_stride", "k_stride", "v_stride"):
        getattr(s, name)[:] = [T * 4 * D, D, 4 * D]
    return s


def _decode_shape(D=64, Tq=1, Tk=64):
    s = _C.bf_attn_decode_t(1, Tq, Tk, 4, 2, D)
    for name in ("q_stride", "k_stride", "v_stride"):
        getattr(s, name)[:] = [Tk * 4 * D, Tk * D, D]
    return s


def _entries():
    lib = _C.lib()

    def fwd(shape, window, softcap, dt=_C.BF_DT_BF16, q=PTR):
        return lib.bf_attention_fwd_gqa_softcap(q, PTR, PTR, None, None, PTR, PTR, dt, ctypes.byref(shape), window, softcap,
                                                0.125, None)

    def bwd(shape, window, softcap, dt=_C.BF_DT_BF16, q=PTR):
        return lib.bf_attention_bwd_gqa_softcap(q, PTR, PTR, None, None, PTR, PTR, PTR, PTR, PTR, PTR, PTR, dt,
                                                ctypes.byref(shape), window, softcap, 0.125, None)

    def dec(shape, window, softcap, dt=_C.BF_DT_BF16, q=PTR):
        return lib.bf_attention_decode_gqa_softcap(q, PTR, PTR, None, None, None, PTR, PTR, dt, ctypes.byref(shape), window,
                                                   softcap, 0.125, None)

    return lib, (("fwd", fwd, _gqa_shape), ("bwd", bwd, _gqa_shape), ("decode", dec, _decode_shape))


def test_the_three_entries_are_declared_bound_and_exported():
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    declared = open(os.path.join(root, "include", "bayeformers_amd_softcap.h")).read()
    assert '#include "bayeformers_amd_softcap.h"' in open(os.path.join(root, "include", "bayeformers_amd.h")).read()
    lib = _C.lib()
    assert sorted(_C.SOFTCAP_SYMBOLS) == ["bf_attention_bwd_gqa_softcap", "bf_attention_decode_gqa_softcap",
                                          "bf_attention_fwd_gqa_softcap"]
    for name, (res, args) in _C.SOFTCAP_SYMBOLS.items():
        assert name + "(" in declared
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype == res
    # the window entries' arguments with (int32 window, float softcap) before scaling; decode: the _len_window entry's
    for new, old in (("bf_attention_fwd_gqa_softcap", "bf_attention_fwd_gqa_window"),
                     ("bf_attention_bwd_gqa_softcap", "bf_attention_bwd_gqa_window"),
                     ("bf_attention_decode_gqa_softcap", "bf_attention_decode_gqa_len_window")):
        plain = _C.SYMBOLS[old][1]
        assert _C.SOFTCAP_SYMBOLS[new][1] == plain[:-2] + [ctypes.c_float] + plain[-2:]


def test_the_softcap_header_prototypes_match_the_ctypes_signatures():
    """tests/test_host_api.py's parse of the main header, applied to include/bayeformers_amd_softcap.h and
    _C.SOFTCAP_SYMBOLS: the argument count and, for the return value and each argument, the class and width."""
    import os
    import re

    from test_host_api import _c_type_class, _ctypes_class

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "bayeformers_amd_softcap.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    header = re.sub(r"^\s*#.*$", "", header, flags=re.M)
    parsed = {}
    for ret, name, params in re.findall(r"([A-Za-z_][A-Za-z0-9_ \t\n\*]*?)\b(bf_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", header):
        assert name not in parsed, name
        parsed[name] = (_c_type_class(ret), [_c_type_class(a.strip()) for a in params.split(",")])
    assert set(parsed) == set(_C.SOFTCAP_SYMBOLS) and not set(parsed) & set(_C.SYMBOLS)
    for name, (res, args) in _C.SOFTCAP_SYMBOLS.items():
        c_res, c_args = parsed[name]
        assert _ctypes_class(res) == c_res, (name, "return")
        assert len(args) == len(c_args), (name, len(args), len(c_args))
        for i, (a, c) in enumerate(zip(args, c_args)):
            assert _ctypes_class(a) == c, (name, i, a, c)


def test_entries_refuse_a_softcap_whose_folded_constants_overflow():
    """scaling / softcap (a denormal softcap) or softcap * log2(e) (close to FLT_MAX) not finite: a tanh argument of
    0 * inf or inf - inf would be NaN"""
    lib, entries = _entries()
    for name, call, shape in entries:
        for softcap in (1e-45, 3e38):
            assert call(shape(), 0, softcap) == 1 and b"softcap" in lib.bf_last_error(), (name, softcap)
        assert call(shape(), 0, 1e-30, q=None) == 1 and b"NULL" in lib.bf_last_error(), name  # (finite constants: accepted)


@pytest.mark.parametrize("softcap", [0.0, -1.0, float("inf"), float("-inf"), float("nan")])
def test_entries_refuse_a_softcap_that_is_not_finite_and_positive(softcap):
    lib, entries = _entries()
    for name, call, shape in entries:
        assert call(shape(), 0, softcap) == 1 and b"softcap" in lib.bf_last_error(), name
        assert call(shape(), 48, softcap) == 1 and b"softcap" in lib.bf_last_error(), name


def test_entries_refuse_a_negative_window_a_non_causal_shape_and_what_the_plain_entries_refuse():
    lib, entries = _entries()
    for name, call, shape in entries:
        assert call(shape(), -1, 50.0) == 1 and b"window" in lib.bf_last_error(), name
        assert call(shape(D=96), 0, 50.0) == 1 and b"head size" in lib.bf_last_error(), name
        assert call(shape(), 0, 50.0, dt=_C.BF_DT_F32) == 1 and b"bf16 or fp16" in lib.bf_last_error(), name
        assert call(shape(), 48, 50.0, q=None) == 1 and b"NULL" in lib.bf_last_error(), name
        assert call(shape(), 0, 50.0, q=PTR + 8) == 1 and b"aligned" in lib.bf_last_error(), name
    for name, call, shape in entries[:2]:
        for window in (0, 48):
            assert call(shape(causal=0), window, 50.0) == 1 and b"causal" in lib.bf_last_error(), name
        assert call(shape(T=0), 0, 50.0) == 1 and b"T=0" in lib.bf_last_error(), name
    dec = entries[2][1]
    assert dec(_decode_shape(Tq=17), 0, 50.0) == 1 and b"Tq=17" in lib.bf_last_error()
    assert dec(_decode_shape(Tq=4, Tk=3), 0, 50.0) == 1 and b"Tk=3" in lib.bf_last_error()
    rc = lib.bf_attention_decode_gqa_softcap(PTR, PTR, PTR, None, None, PTR + 4, PTR, PTR, _C.BF_DT_BF16,
                                             ctypes.byref(_decode_shape()), 0, 50.0, 0.125, None)
    assert rc == 1 and b"kv_len" in lib.bf_last_error()


# ---------------------------------------------------------------------------------------------------- routing
@pytest.fixture
def launches(monkeypatch):
    """The fixture of tests/test_head256_cpu.py with fakes that accept `softcap`: pretend the kernels apply to CPU tensors
    and record (entry, window, softcap) of each call; the dispatch rules are NOT replaced by "always" here except decode's,
    so a rule the soft-cap path consulted would show."""
    seen = []
    monkeypatch.setattr(ops, "attention_supported", lambda *a, **k: True)
    monkeypatch.setattr(ops, "attention_decode_supported", lambda *a, **k: True)
    monkeypatch.setattr(ops, "decode_kernel_wins", lambda *a, **k: seen.append(("decode_kernel_wins",)) or True)
    real_rule = ops.prefill_kernel_wins
    monkeypatch.setattr(ops, "prefill_kernel_wins", lambda *a, **k: seen.append(("prefill_kernel_wins",)) or real_rule(*a, **k))

    def zeros(q):
        return torch.zeros(q.shape[0], q.shape[2], q.shape[1], q.shape[3], dtype=q.dtype)

    def fwd(q, k, v, key_mask, scaling, causal=True, mask_off=None, want_lse=False, window=None, softcap=None):
        seen.append(("gqa", window, softcap))
        return (zeros(q), torch.zeros(q.shape[:3])) if want_lse else zeros(q)

    def dec(q, k, v, key_mask, scaling, mask_off=None, workspace=None, window=None, softcap=None):
        seen.append(("decode", window, softcap))
        return zeros(q)

    def dec_len(q, k, v, kv_len, key_mask, scaling, mask_off=None, workspace=None, window=None, softcap=None):
        seen.append(("decode_len", window, softcap))
        return zeros(q)

    import transformers.integrations.sdpa_attention as sa

    real_sdpa = sa.sdpa_attention_forward

    def sdpa(*a, **k):
        seen.append(("sdpa", None, None))
        k.pop("s_aux", None), k.pop("softcap", None)
        return real_sdpa(*a, **k)

    monkeypatch.setattr(ops, "attention_forward_gqa", fwd)
    monkeypatch.setattr(ops, "attention_forward_decode", dec)
    monkeypatch.setattr(ops, "attention_forward_decode_len", dec_len)
    monkeypatch.setattr(sa, "sdpa_attention_forward", sdpa)
    return seen


def _module(training=False):
    mod = torch.nn.Module()
    mod.is_causal = True
    mod.num_key_value_groups = 2
    mod.train(training)
    return mod


def _masks(W=48):
    """(name, q, k, mask, entry, window) of the calls the kernels take"""
    from transformers.masking_utils import causal_mask_function, sliding_window_causal_mask_function

    q, k = torch.zeros(2, 2, 128, 32), torch.zeros(2, 1, 128, 32)
    pad = torch.ones(2, 128, dtype=torch.long)
    pad[1, 120:] = 0
    causal = bf._padding_mask_interface(2, q_length=128, kv_length=128, mask_function=causal_mask_function, attention_mask=pad)
    assert getattr(causal, "_bf_causal", False)
    sliding = bf._padding_mask_interface(2, q_length=128, kv_length=128, attention_mask=pad,
                                         mask_function=sliding_window_causal_mask_function(W))
    assert getattr(sliding, "_bf_window", None) == W
    q1, kc = torch.zeros(2, 2, 1, 32), torch.zeros(2, 1, 40, 32)
    step = bf._padding_mask_interface(2, q_length=1, kv_length=40, q_offset=39, attention_mask=torch.ones(2, 40, dtype=torch.long),
                                      mask_function=sliding_window_causal_mask_function(W))
    assert getattr(step, "_bf_decode", False) and step._bf_window == W
    fixed = bf._padding_mask_interface(2, q_length=1, kv_length=40, q_offset=torch.tensor(7), mask_function=causal_mask_function,
                                       attention_mask=None, allow_is_causal_skip=False)
    assert getattr(fixed, "_bf_kv_len", None) is not None
    fixed_w = bf._padding_mask_interface(2, q_length=1, kv_length=40, q_offset=torch.tensor(7), attention_mask=None,
                                         mask_function=sliding_window_causal_mask_function(W), allow_is_causal_skip=False)
    assert fixed_w._bf_kv_len is not None and fixed_w._bf_window == W
    return [("prefill", q, k, None, "gqa", None), ("prefill, padding mask", q, k, causal, "gqa", None),
            ("prefill, sliding mask", q, k, sliding, "gqa", W), ("decode", q1, kc, None, "decode", None),
            ("decode, sliding mask", q1, kc, step, "decode", W), ("fixed capacity", q1, kc, fixed, "decode_len", None),
            ("fixed capacity, sliding mask", q1, kc, fixed_w, "decode_len", W)]


def test_with_the_switch_off_every_softcap_call_goes_to_sdpa(launches):
    assert not bf.softcap_attention_enabled()
    for name, q, k, mask, _, W in _masks():
        del launches[:]
        kw = {} if W is None else dict(sliding_window=W)
        bf._attention_interface(_module(), q, k, k, mask, softcap=50.0, **kw)
        assert [e for e in launches if e[0] not in ("decode_kernel_wins", "prefill_kernel_wins")] == [("sdpa", None, None)], name


def test_with_the_switch_on_the_kernels_take_the_cap_and_the_window(launches):
    bf.softcap_attention()
    assert bf.softcap_attention_enabled()
    for name, q, k, mask, entry, W in _masks():
        del launches[:]
        kw = {} if W is None else dict(sliding_window=W)
        out, _ = bf._attention_interface(_module(), q, k, k, mask, softcap=50.0, **kw)
        assert launches == [(entry, W, 50.0)], (name, launches)  # (and neither dispatch rule was asked)
        assert out.shape == (q.shape[0], q.shape[2], q.shape[1], q.shape[3])
        del launches[:]
        bf._attention_interface(_module(), q, k, k, mask, softcap=None, **kw)  # no cap: today's call, no softcap argument
        assert [e for e in launches if len(e) == 3] == [(entry, W, None)], name


def test_with_the_switch_on_gradients_run_the_autograd_function_with_the_cap(launches, monkeypatch):
    bf.softcap_attention()
    q = torch.zeros(1, 2, 128, 32, requires_grad=True)
    k = torch.zeros(1, 1, 128, 32)
    bf._attention_interface(_module(), q, k, k, None, softcap=30.0)
    assert launches == [("gqa", None, 30.0)]


def test_sinks_and_a_disagreeing_window_still_go_away_with_the_switch_on(launches):
    bf.softcap_attention()
    _, q, k, sliding, _, W = _masks()[2]
    bf._attention_interface(_module(), q, k, k, None, softcap=50.0, s_aux=torch.zeros(2))
    bf._attention_interface(_module(), q, k, k, sliding, softcap=50.0, sliding_window=W + 1)
    assert [e for e in launches if len(e) == 3] == [("sdpa", None, None)] * 2


def test_what_the_kernels_do_not_take_runs_the_capped_fallback_never_sdpa(launches, monkeypatch):
    bf.softcap_attention()
    seen = []
    real = bf._softcap_eager
    monkeypatch.setattr(bf, "_softcap_eager", lambda *a, **k: seen.append(a[-1]) or real(*a, **k))
    q, k = torch.randn(1, 2, 128, 32), torch.randn(1, 1, 128, 32)
    out, _ = bf._attention_interface(_module(training=True), q, k, k, None, dropout=0.1, softcap=50.0)  # attention dropout
    assert out.shape == (1, 128, 2, 32)
    fake_decode = ops.attention_decode_supported  # (the fixture's: always True)
    qc, kc = torch.randn(1, 2, 40, 64).bfloat16(), torch.randn(1, 1, 100, 64).bfloat16()
    monkeypatch.setattr(ops, "attention_decode_supported", lambda q, k, v, check_device=True: REAL_DECODE_SUPPORTED(q, k, v, False))
    assert ops.attention_decode_supported(qc[:, :, :16], kc, kc) and not ops.attention_decode_supported(qc, kc, kc)
    out, _ = bf._attention_interface(_module(), qc, kc, kc, None, softcap=50.0)  # a cached chunk of 40 queries
    monkeypatch.setattr(ops, "attention_decode_supported", fake_decode)
    assert out.shape == (1, 40, 2, 64)
    other = torch.ones(1, 1, 128, 128, dtype=torch.bool).tril()  # a mask _padding_mask_interface did not build
    bf._attention_interface(_module(), q, k, k, other, softcap=50.0, is_causal=True)
    monkeypatch.setattr(ops, "attention_supported", lambda *a, **k: False)  # an unsupported shape or dtype
    bf._attention_interface(_module(), q, k, k, None, softcap=50.0)
    monkeypatch.setattr(ops, "attention_decode_supported", lambda *a, **k: False)
    bf._attention_interface(_module(), qc[:, :, :1], kc, kc, None, softcap=50.0)
    assert seen == [50.0] * 5 and launches == []


@pytest.mark.parametrize("Tq,Tk,kind", [(24, 24, "none"), (24, 24, "bool"), (5, 24, "none"), (5, 24, "bool"), (1, 24, "none"),
                                        (24, 24, "additive")])
def test_the_capped_fallback_is_gemma2s_eager_attention(Tq, Tk, kind):
    from transformers.models.gemma2.modeling_gemma2 import eager_attention_forward

    g = torch.Generator().manual_seed(Tq + Tk)
    q = torch.randn(2, 4, Tq, 16, generator=g) * 6
    k, v = (torch.randn(2, 2, Tk, 16, generator=g) for _ in range(2))
    allowed = softcap_ref.visible(Tq, Tk, 9 if kind != "none" else None, "cpu")[None, None].expand(2, 1, Tq, Tk).clone()
    if kind != "none":
        allowed[1, :, :, Tk - 3:] = False
    lowest = torch.finfo(torch.float32).min
    additive = torch.zeros(2, 1, Tq, Tk).masked_fill(~allowed, lowest)
    mask = {"none": None, "bool": allowed, "additive": additive}[kind]
    mod = _module()
    got = bf._softcap_eager(mod, q, k, v, mask, 0.0, 0.25, 7.0)
    want, _ = eager_attention_forward(mod, q, k, v, additive, dropout=0.0, scaling=0.25, softcap=7.0)
    assert got.shape == want.shape == (2, Tq, 4, 16)
    assert torch.equal(got, want)
    uncapped, _ = eager_attention_forward(mod, q, k, v, additive, dropout=0.0, scaling=0.25, softcap=None)
    assert (uncapped - want).abs().max().item() > 0.05  # (the cap is not a detail here)


# ---------------------------------------------------------------------------------------------------- a tiny Gemma 2
W = 48


def _gemma2(**kw):
    from transformers import AutoConfig, AutoModelForCausalLM

    base = dict(hidden_size=64, num_attention_heads=4, num_key_value_heads=2, head_dim=32, num_hidden_layers=2,
                intermediate_size=128, vocab_size=64, max_position_embeddings=512, sliding_window=W,
                layer_types=["sliding_attention", "full_attention"], attn_logit_softcapping=50.0, query_pre_attn_scalar=32,
                attn_implementation="sdpa")
    base.update(kw)
    torch.manual_seed(0)
    model = AutoModelForCausalLM.from_config(AutoConfig.for_model("gemma2", **base)).eval()
    assert type(model).__name__ == "Gemma2ForCausalLM"
    return model


def test_a_tiny_gemma2_routes_its_layers_as_window_and_cap_then_cap(launches):
    model = _gemma2()
    assert bf.fuse_attention(model)
    ids = torch.zeros(1, 128, dtype=torch.long)
    with torch.no_grad():
        model(ids, use_cache=False)
        assert [e for e in launches if len(e) == 3] == [("sdpa", None, None)] * 2  # off: the framework, WITHOUT the cap
        bf.softcap_attention()
        del launches[:]
        out = model(ids, use_cache=True)
        assert launches == [("gqa", W, 50.0), ("gqa", None, 50.0)]
        del launches[:]
        model(torch.zeros(1, 1, dtype=torch.long), past_key_values=out.past_key_values, use_cache=True)
        assert launches == [("decode", W, 50.0), ("decode", None, 50.0)]
    del launches[:]
    model(ids, attention_mask=torch.ones_like(ids), use_cache=False)  # gradients recorded: AttentionGqaFn
    assert launches == [("gqa", W, 50.0), ("gqa", None, 50.0)]


def test_static_cache_takes_gemma2_with_the_switch_on_and_raises_with_it_off():
    from transformers.cache_utils import StaticLayer

    from bayeformers_amd.sampling import _SLIDING_STATIC_FAMILIES, _static_cache

    assert "gemma2" in _SLIDING_STATIC_FAMILIES
    model = bf.to_bayesian(_gemma2(), delta=0.05, freeze=True).eval()
    assert bf.fuse_attention(model)
    with pytest.raises(RuntimeError, match="softcap_attention"):
        _static_cache(model, 200)
    bf.softcap_attention()
    cache = _static_cache(model, 200)
    assert len(cache.layers) == 2 and all(type(layer) is StaticLayer and layer.max_cache_len == 200 for layer in cache.layers)
    plain = bf.to_bayesian(_gemma2(attn_logit_softcapping=None), delta=0.05, freeze=True).eval()
    assert bf.fuse_attention(plain)
    bf.softcap_attention(False)
    assert len(_static_cache(plain, 64).layers) == 2  # no cap in the config: nothing to guard


def test_the_switch_is_off_by_default_follows_the_environment_and_is_baked(monkeypatch):
    from bayeformers_amd import graphs

    model = torch.nn.Linear(2, 2)
    assert not bf.softcap_attention_enabled()
    off = graphs.baked_state(model)
    assert graphs.still_valid(model, off)
    bf.softcap_attention()
    on = graphs.baked_state(model)
    assert on != off and not graphs.still_valid(model, off) and graphs.still_valid(model, on)
    bf.softcap_attention(False)
    assert graphs.still_valid(model, off)
    monkeypatch.setenv("BF_SOFTCAP_ATTENTION", "1")
    assert bf.softcap_attention_enabled() and graphs.baked_state(model) == on


def test_the_counters_of_the_other_entries_keep_their_keys():
    assert ops.SOFTCAP_CALLS.keys() == {"fwd", "bwd", "decode", "decode_len"}
    assert ops.GQA_CALLS.keys() == {"fwd", "bwd", "fwd_window", "bwd_window"}
    assert ops.DECODE_CALLS.keys() == {"fwd", "len", "window", "len_window"}
