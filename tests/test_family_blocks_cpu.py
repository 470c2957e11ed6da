"""Host side of fuse_decoder_blocks(families=...) for Qwen3 and Gemma 1 / 2 / 3 (no GPU): the float64 restatement of the
three ops (tests/family_blocks_ref.py) against transformers' own modules, the bindings and the header of the three C
entries, their argument checks, and which models the rewrite takes."""
import ctypes
import os
import re

import pytest
import torch

transformers = pytest.importorskip("transformers")

import bayeformers_amd as bf  # noqa: E402
from bayeformers_amd import _C, ops  # noqa: E402
from family_blocks_ref import geglu_ref, norm_add_rmsnorm_ref, qknorm_rope_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["bf_geglu", "bf_norm_add_rmsnorm", "bf_qknorm_rope"]


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


# ------------------------------------------------------------------------------- the restatement is HF's arithmetic
def test_reference_equals_hf_modules_in_float64():
    """Gemma2RMSNorm (around the residual add, as Gemma2DecoderLayer.forward chains them), Qwen3RMSNorm / Gemma3RMSNorm per
    head + apply_rotary_pos_emb, and gelu(approximate="tanh") * up, restated line for line in float64 (the modules upcast
    to float32 inside): only reassociation separates them from the restatement (1e-12 relative)."""
    import torch.nn.functional as F
    from transformers.models.qwen3.modeling_qwen3 import apply_rotary_pos_emb

    g = torch.Generator().manual_seed(31)
    x, r = (torch.randn(5, 7, 96, generator=g, dtype=torch.float64) for _ in range(2))
    w_pre, w_out = (torch.randn(96, generator=g, dtype=torch.float64) * 0.5 for _ in range(2))

    def gemma_norm(t, w, eps):  # Gemma2RMSNorm.forward: _norm(x) * (1.0 + weight)
        return t * torch.rsqrt(t.pow(2).mean(-1, keepdim=True) + eps) * (1.0 + w)

    def qwen_norm(t, w, eps):  # Qwen3RMSNorm.forward: weight * (x * rsqrt(variance + eps))
        return w * (t * torch.rsqrt(t.pow(2).mean(-1, keepdim=True) + eps))

    hidden = r + gemma_norm(x, w_pre, 1e-6)  # residual + post_attention_layernorm(attn_out)
    u, z, y = norm_add_rmsnorm_ref(x, w_pre, r, w_out, 1e-6, 1e-5, 1)
    assert _rel(z, hidden) < 1e-12 and _rel(y, gemma_norm(hidden, w_out, 1e-5)) < 1e-12
    u, z, y = norm_add_rmsnorm_ref(x, None, r, w_out, 0.0, 1e-5, 1)  # Gemma 1: add, then the norm
    assert torch.equal(u, x) and torch.equal(z, r + x) and _rel(y, gemma_norm(r + x, w_out, 1e-5)) < 1e-12
    u, z, y = norm_add_rmsnorm_ref(x, None, None, w_out, 0.0, 1e-5, 0)  # offset 0: Qwen3RMSNorm
    assert torch.equal(z, x) and _rel(y, qwen_norm(x, w_out, 1e-5)) < 1e-12
    # the rounding points: u and z are values of the dtype, y comes from the rounded z
    xb, rb = x.bfloat16(), r.bfloat16()
    u, z, y = norm_add_rmsnorm_ref(xb, w_pre, rb, w_out, 1e-6, 1e-5, 1, torch.bfloat16)
    assert torch.equal(u, u.bfloat16().double()) and torch.equal(z, (rb.double() + u).bfloat16().double())
    assert _rel(y, gemma_norm(z, w_out, 1e-5)) < 1e-12

    B, H, Hkv, T, D = 2, 4, 2, 9, 64
    q = torch.randn(B, H, T, D, generator=g, dtype=torch.float64)
    k = torch.randn(B, Hkv, T, D, generator=g, dtype=torch.float64)
    ang = torch.randn(B, T, D, generator=g, dtype=torch.float64)
    cos, sin = ang.cos(), ang.sin()
    wq, wk = (torch.randn(D, generator=g, dtype=torch.float64) for _ in range(2))
    for norm, off in ((qwen_norm, 0), (gemma_norm, 1)):
        hq, hk = apply_rotary_pos_emb(norm(q, wq, 1e-6), norm(k, wk, 1e-6), cos, sin)
        assert _rel(qknorm_rope_ref(q, cos, sin, wq, 1e-6, off)[0], hq) < 1e-12
        assert _rel(qknorm_rope_ref(k, cos, sin, wk, 1e-6, off)[0], hk) < 1e-12
    hq, _ = apply_rotary_pos_emb(q, k, cos[:1], sin[:1])
    assert _rel(qknorm_rope_ref(q, cos[:1], sin[:1], None, 0.0, 0)[0], hq) < 1e-12

    gate = torch.randn(6, 40, generator=g, dtype=torch.float64) * 4
    up = torch.randn(6, 40, generator=g, dtype=torch.float64)
    assert _rel(geglu_ref(gate, up), F.gelu(gate, approximate="tanh") * up) < 1e-12
    hard = torch.tensor([-800.0, -100.0, -30.0, 30.0, 100.0, 800.0], dtype=torch.float64)
    got = geglu_ref(hard, torch.ones_like(hard))
    assert torch.isfinite(got).all() and got[0] == 0 and got[-1] == 800.0


# ------------------------------------------------------------------------------------------- bindings, header, checks
def test_the_three_entries_are_declared_bound_and_exported():
    declared = open(os.path.join(ROOT, "include", "bayeformers_amd_family_blocks.h")).read()
    main = open(os.path.join(ROOT, "include", "bayeformers_amd.h")).read()
    assert main.count('#include "bayeformers_amd_family_blocks.h"') == 1
    lib = _C.lib()
    assert sorted(_C.FAMILY_BLOCK_SYMBOLS) == NAMES and not set(NAMES) & set(_C.SYMBOLS) and not set(NAMES) & set(_C.SOFTCAP_SYMBOLS)
    for name, (res, args) in _C.FAMILY_BLOCK_SYMBOLS.items():
        assert name + "(" in declared and name + "(" not in main
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype == res
    assert _C.FAMILY_BLOCK_SYMBOLS["bf_geglu"] == _C.SYMBOLS["bf_swiglu"]
    rope = _C.SYMBOLS["bf_rope_qk"][1]  # bf_rope_qk's arguments with (gamma_q, gamma_k, param_dtype, offset, eps) behind cs_dtype
    assert _C.FAMILY_BLOCK_SYMBOLS["bf_qknorm_rope"][1] == rope[:5] + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                                                       ctypes.c_float] + rope[5:]
    assert _C.ABI_VERSION == 6 and lib.bf_version() == 6
    assert ops.FAMILY_BLOCK_CALLS.keys() == {"norm_add_norm", "qknorm_rope", "geglu"}
    assert ops.BLOCK_CALLS.keys() == {"rmsnorm", "rope", "swiglu"}


def test_the_header_prototypes_match_the_ctypes_signatures():
    """tests/test_host_api.py's parse of the main header, applied to include/bayeformers_amd_family_blocks.h and
    _C.FAMILY_BLOCK_SYMBOLS: the argument count and, for the return value and each argument, the class and width."""
    from test_host_api import _c_type_class, _ctypes_class

    header = open(os.path.join(ROOT, "include", "bayeformers_amd_family_blocks.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    header = re.sub(r"^\s*#.*$", "", header, flags=re.M)
    parsed = {}
    for ret, name, params in re.findall(r"([A-Za-z_][A-Za-z0-9_ \t\n\*]*?)\b(bf_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", header):
        assert name not in parsed, name
        parsed[name] = (_c_type_class(ret), [_c_type_class(a.strip()) for a in params.split(",")])
    assert set(parsed) == set(_C.FAMILY_BLOCK_SYMBOLS) and not set(parsed) & set(_C.SYMBOLS)
    for name, (res, args) in _C.FAMILY_BLOCK_SYMBOLS.items():
        c_res, c_args = parsed[name]
        assert _ctypes_class(res) == c_res, (name, "return")
        assert len(args) == len(c_args), (name, len(args), len(c_args))
        for i, (a, c) in enumerate(zip(args, c_args)):
            assert _ctypes_class(a) == c, (name, i, a, c)


def test_a_library_without_the_entries_asks_for_a_rebuild(monkeypatch):
    """A library from before these entries reports the same ABI version: lib() names the missing symbol and the rebuild
    instead of raising a bare AttributeError."""
    monkeypatch.setattr(_C, "_lib", None)
    monkeypatch.setitem(_C.FAMILY_BLOCK_SYMBOLS, "bf_not_in_this_library", (ctypes.c_int, []))
    with pytest.raises(_C.BayeFormersAMDError, match="lacks bf_not_in_this_library.*rebuild"):
        _C.lib()
    assert _C._lib is None


def _err():
    return _C.lib().bf_last_error().decode()


def test_norm_add_rmsnorm_refuses_bad_arguments_without_a_device():
    f = _C.lib().bf_norm_add_rmsnorm
    ok = dict(x=4096, gp=32, res=8192, go=16, pd=_C.BF_DT_F32, off=1, z=12288, y=16384, dt=_C.BF_DT_BF16, rows=4, N=64)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["x"], a["gp"], a["res"], a["go"], a["pd"], a["off"], a["z"], a["y"], a["dt"], a["rows"], a["N"], 1e-6, 1e-6,
                 None)

    assert call(x=None) == 1 and "null pointer" in _err()
    assert call(y=None) == 1 and "null pointer" in _err()
    assert call(go=None) == 1 and "null pointer" in _err()
    assert call(x=4104) == 1 and "16-byte aligned" in _err()
    assert call(gp=40) == 1 and "16-byte aligned" in _err()
    assert call(z=8) == 1 and "16-byte aligned" in _err()
    assert call(N=60) == 1 and "multiple of 8" in _err()
    assert call(N=8200) == 1 and "at most 8192" in _err()
    assert call(off=2) == 1 and "weight_offset=2" in _err()
    assert call(off=-1) == 1 and "weight_offset" in _err()
    assert call(dt=7) == 1 and "unknown dtype" in _err()
    assert call(pd=_C.BF_DT_F16) == 1 and "gammas must be fp32" in _err()
    assert call(rows=-1) == 1 and "bad shape" in _err()
    assert call(rows=0) == 0 and call(rows=0, gp=None, res=None, z=None) == 0  # nothing to do: no launch, no device needed


def test_qknorm_rope_refuses_bad_arguments_without_a_device():
    f = _C.lib().bf_qknorm_rope

    def shape(D=64, cos_batch=1, stride=64, B=2):
        s = _C.bf_rope_t(B, 4, 8, 2, D, cos_batch)
        for name in ("q_stride", "k_stride", "q_out_stride", "k_out_stride"):
            getattr(s, name)[:] = [4 * 8 * D, stride, 8 * D]
        return s

    def call(s, q=4096, cos=16, dt=_C.BF_DT_BF16, cd=_C.BF_DT_F32, gq=48, gk=64, pd=_C.BF_DT_F32, off=0):
        return f(q, 8192, cos, 32, cd, gq, gk, pd, off, 1e-6, q, 8192, dt, ctypes.byref(s) if s is not None else None, None)

    assert call(None) == 1 and "shape is NULL" in _err()
    assert call(shape(D=96)) == 1 and "head_dim=96 must be 64, 128 or 256" in _err()
    assert call(shape(D=512)) == 1 and "head_dim=512" in _err()
    assert call(shape(cos_batch=3)) == 1 and "cos_batch" in _err()
    assert call(shape(), q=None) == 1 and "null pointer" in _err()
    assert call(shape(), cos=24) == 1 and "16-byte aligned" in _err()
    assert call(shape(), gk=72) == 1 and "16-byte aligned" in _err()
    assert call(shape(stride=60)) == 1 and "multiples of 8" in _err()
    assert call(shape(stride=-64)) == 1 and "multiples of 8" in _err()
    assert call(shape(), off=2) == 1 and "weight_offset=2" in _err()
    assert call(shape(), dt=9) == 1 and "unknown dtype" in _err()
    assert call(shape(), cd=_C.BF_DT_F16) == 1 and "cos / sin must be fp32" in _err()
    assert call(shape(), pd=_C.BF_DT_F16) == 1 and "gammas must be fp32" in _err()
    for D in (64, 128, 256):  # an empty batch: nothing to do, no launch, no device needed; with and without gammas
        assert call(shape(D=D, B=0, cos_batch=1)) == 0 and call(shape(D=D, B=0), gq=None, gk=None) == 0


def test_geglu_refuses_bad_arguments_without_a_device():
    f = _C.lib().bf_geglu
    assert f(None, 64, 4096, 64, 8192, 64, _C.BF_DT_BF16, 4, 64, None) == 1 and "null pointer" in _err()
    assert f(4096, 64, 8192, 64, None, 64, _C.BF_DT_BF16, 4, 64, None) == 1 and "null pointer" in _err()
    assert f(4104, 64, 4096, 64, 8192, 64, _C.BF_DT_BF16, 4, 64, None) == 1 and "16-byte aligned" in _err()
    assert f(4096, 64, 8192, 64, 12288, 64, _C.BF_DT_BF16, 4, 60, None) == 1 and "multiple of 8" in _err()
    assert f(4096, 32, 8192, 64, 12288, 64, _C.BF_DT_BF16, 4, 64, None) == 1 and "row strides" in _err()
    assert f(4096, 68, 8192, 64, 12288, 64, _C.BF_DT_BF16, 4, 64, None) == 1 and "row strides" in _err()
    assert f(4096, 64, 8192, 64, 12288, 64, 5, 4, 64, None) == 1 and "unknown dtype" in _err()
    assert f(4096, 64, 8192, 64, 12288, 64, _C.BF_DT_F32, -1, 64, None) == 1 and "bad shape" in _err()
    assert f(4096, 64, 8192, 64, 12288, 64, _C.BF_DT_F32, 0, 64, None) == 0


def test_ops_refuse_cpu_tensors():
    x = torch.randn(4, 64)
    w = torch.ones(64)
    with pytest.raises(_C.BayeFormersAMDError, match="ROCm device"):
        ops.norm_add_rmsnorm(x, w, x, w, 1e-6, 1e-6)
    with pytest.raises(_C.BayeFormersAMDError, match="ROCm device"):
        ops.geglu(x, x)
    q = torch.randn(1, 2, 3, 64)
    with pytest.raises(_C.BayeFormersAMDError, match="ROCm device"):
        ops.qknorm_rope(q, q, torch.ones(1, 3, 64), torch.zeros(1, 3, 64), w, w)
    norm = torch.nn.RMSNorm(64)
    assert not ops.norm_add_rmsnorm_supported(x, norm, x, norm) and not ops.geglu_supported(x, x)
    assert not ops.qknorm_rope_supported(q, q, torch.ones(1, 3, 64), torch.zeros(1, 3, 64), w, w)


# ----------------------------------------------------------------------------------------------- which models it rewrites
KINDS = {"qwen3": "qwen3", "gemma": "gemma", "gemma2": "gemma2", "gemma3": "gemma3"}


def _tiny(kind, layers=3, **kw):
    import transformers as tf

    cfg_cls, model_cls = {"qwen3": (tf.Qwen3Config, tf.Qwen3ForCausalLM), "gemma": (tf.GemmaConfig, tf.GemmaForCausalLM),
                          "gemma2": (tf.Gemma2Config, tf.Gemma2ForCausalLM),
                          "gemma3": (tf.Gemma3TextConfig, tf.Gemma3ForCausalLM)}[kind]
    cfg = cfg_cls(hidden_size=128, num_attention_heads=2, num_key_value_heads=1, num_hidden_layers=layers,
                  intermediate_size=256, vocab_size=97, max_position_embeddings=64, tie_word_embeddings=False,
                  head_dim=64, **kw)
    torch.manual_seed(3)
    model = model_cls(cfg).eval()
    if kind != "qwen3":  # Gemma's norm weights start at zero: (1 + weight) with a weight that shows
        g = torch.Generator().manual_seed(4)
        with torch.no_grad():
            for name, p in model.named_parameters():
                if name.endswith("norm.weight"):
                    p.copy_(0.3 * torch.randn(p.shape, generator=g))
    return model


def _forwards(kind):
    layer = {"qwen3": bf._decoder_layer_forward, "gemma": bf._gemma_layer_forward, "gemma2": bf._sandwich_layer_forward,
             "gemma3": bf._sandwich_layer_forward}[kind]
    mlp = bf._swiglu_mlp_forward if kind == "qwen3" else bf._geglu_mlp_forward
    norm = bf._rmsnorm_forward if kind == "qwen3" else bf._gemma_rmsnorm_forward
    return layer, mlp, norm


@pytest.mark.parametrize("families", ["named", "all"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_rewrites_every_layer_once_and_declines_off_device(kind, families):
    model = _tiny(kind)
    ids = torch.randint(0, 97, (2, 12), generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        ref = model(input_ids=ids, output_hidden_states=True)
    keys = list(model.state_dict().keys())
    assert bf.fuse_decoder_blocks(model) == 0  # the default families leave it alone ...
    assert bf.fuse_decoder_blocks(model, families=("llama", "qwen2")) == 0
    assert "forward" not in model.model.layers[0].__dict__ and "forward" not in model.model.norm.__dict__
    fam = "all" if families == "all" else (kind,) if kind != "gemma2" else kind  # (a tuple of names or a single name)
    assert bf.fuse_decoder_blocks(model, families=fam) == 3
    assert bf.fuse_decoder_blocks(model, families=fam) == 0 and bf.fuse_decoder_blocks(model, families="all") == 0
    assert bf.fuse_decoder_blocks(model, backward=True, families="all") == 0  # ... and no backward flag appears
    assert not any(hasattr(m, "_bf_blocks_backward") for m in model.modules())
    assert list(model.state_dict().keys()) == keys  # the recorded next norm is not a child of the layer
    layer = model.model.layers[0]
    f_layer, f_mlp, f_norm = _forwards(kind)
    assert layer.forward.__func__ is f_layer and layer._bf_next_norm[0] is model.model.layers[1].input_layernorm
    assert model.model.layers[-1]._bf_next_norm[0] is model.model.norm
    assert layer.mlp.forward.__func__ is f_mlp and layer.self_attn.forward.__func__ is bf._family_attention_forward
    assert layer.input_layernorm.forward.__func__ is f_norm and model.model.norm.forward.__func__ is f_norm
    assert "forward" not in layer.post_attention_layernorm.__dict__
    before, before_old = dict(ops.FAMILY_BLOCK_CALLS), dict(ops.BLOCK_CALLS)
    with torch.no_grad():
        got = model(input_ids=ids, output_hidden_states=True)
    # fp32 on the CPU: every fast form declines and the modules' own forwards run — the same bits
    assert torch.equal(got.logits, ref.logits)
    assert all(torch.equal(a, b) for a, b in zip(got.hidden_states, ref.hidden_states))
    # with gradients recorded as well
    rec = model(input_ids=ids, output_hidden_states=True)
    assert torch.equal(rec.logits, ref.logits) and all(torch.equal(a, b) for a, b in zip(rec.hidden_states, ref.hidden_states))
    loss = model(input_ids=ids, labels=ids).loss
    loss.backward()
    assert model.model.layers[0].mlp.gate_proj.weight.grad is not None
    assert ops.FAMILY_BLOCK_CALLS == before and ops.BLOCK_CALLS == before_old


def test_unknown_families_are_an_error_and_named_families_take_only_their_own():
    with pytest.raises(ValueError, match="unknown families"):
        bf.fuse_decoder_blocks(_tiny("qwen3"), families=("qwen3", "olmo"))
    assert bf.fuse_decoder_blocks(_tiny("gemma2"), families=("gemma", "gemma3", "qwen3")) == 0
    assert bf.fuse_decoder_blocks(_tiny("gemma"), families=("gemma2",)) == 0


def test_converted_models_are_rewritten_too():
    for kind in KINDS:
        bmodel = bf.to_bayesian(_tiny(kind, layers=2), delta=0.05, freeze=True)
        assert bf.fuse_decoder_blocks(bmodel, families=kind) == 2 and bf.fuse_decoder_blocks(bmodel, families="all") == 0


def test_a_gemma_around_another_activation_is_declined():
    for kind, key in (("gemma", "hidden_act"), ("gemma2", "hidden_activation"), ("gemma3", "hidden_activation")):
        model = _tiny(kind, **{key: "silu"})
        assert type(model.model.layers[0].mlp.act_fn).__name__.startswith("SiLU")
        assert bf.fuse_decoder_blocks(model, families="all") == 0
        assert "forward" not in model.model.layers[0].__dict__ and "forward" not in model.model.norm.__dict__
    assert bf.fuse_decoder_blocks(_tiny("qwen3", hidden_act="gelu_pytorch_tanh"), families="all") == 0
