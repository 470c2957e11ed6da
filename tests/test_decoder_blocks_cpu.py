"""Host side of fuse_decoder_blocks (no GPU): the float64 restatement of the three ops against transformers' own modules,
the C-ABI entries' argument checks, and which models the rewrite takes."""
import ctypes

import pytest
import torch

transformers = pytest.importorskip("transformers")

import bayeformers_amd as bf  # noqa: E402
from bayeformers_amd import _C, ops  # noqa: E402
from decoder_blocks_ref import add_rmsnorm_ref, rope_ref, swiglu_ref  # noqa: E402


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


# ------------------------------------------------------------------------------- the restatement is HF's arithmetic
def test_reference_equals_hf_modules_in_float64():
    """LlamaRMSNorm, apply_rotary_pos_emb and SiLUActivation(g) * u run in float64 on the CPU: only reassociation separates
    them from tests/decoder_blocks_ref.py (1e-12 relative)."""
    from transformers.activations import ACT2FN
    from transformers.models.llama.modeling_llama import LlamaRMSNorm, apply_rotary_pos_emb

    g = torch.Generator().manual_seed(11)
    x = torch.randn(5, 7, 96, generator=g, dtype=torch.float64)
    r = torch.randn(5, 7, 96, generator=g, dtype=torch.float64)
    norm = LlamaRMSNorm(96, eps=1e-5).double()
    with torch.no_grad():
        norm.weight.copy_(torch.randn(96, generator=g, dtype=torch.float64))
        # (the module upcasts to float32 inside: restate its forward in float64, line for line)
        h = r + x
        hf = norm.weight * (h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + norm.variance_epsilon))
    z, y = add_rmsnorm_ref(x, r, norm.weight.detach(), norm.variance_epsilon)
    assert torch.equal(z, r + x) and _rel(y, hf) < 1e-12
    z0, y0 = add_rmsnorm_ref(x, None, norm.weight.detach(), norm.variance_epsilon)
    assert torch.equal(z0, x)
    assert _rel(y0, norm.weight.detach() * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + 1e-5))) < 1e-12

    B, H, Hkv, T, D = 2, 4, 2, 9, 64
    q = torch.randn(B, H, T, D, generator=g, dtype=torch.float64)
    k = torch.randn(B, Hkv, T, D, generator=g, dtype=torch.float64)
    ang = torch.randn(B, T, D, generator=g, dtype=torch.float64)
    cos, sin = ang.cos(), ang.sin()
    hq, hk = apply_rotary_pos_emb(q, k, cos, sin)
    assert _rel(rope_ref(q, cos, sin)[0], hq) < 1e-12 and _rel(rope_ref(k, cos, sin)[0], hk) < 1e-12
    assert _rel(rope_ref(q, cos[:1], sin[:1])[0], apply_rotary_pos_emb(q, k, cos[:1], sin[:1])[0]) < 1e-12

    gate = torch.randn(6, 40, generator=g, dtype=torch.float64) * 4
    up = torch.randn(6, 40, generator=g, dtype=torch.float64)
    assert _rel(swiglu_ref(gate, up), ACT2FN["silu"](gate) * up) < 1e-12
    hard = torch.tensor([-800.0, -100.0, -30.0, 30.0, 100.0, 800.0], dtype=torch.float64)
    got = swiglu_ref(hard, torch.ones_like(hard))
    assert torch.isfinite(got).all() and got[0] == 0 and got[-1] == 800.0


# ------------------------------------------------------------------------------------------- bindings, argument checks
def test_symbols_are_bound_and_struct_matches_header():
    assert {"bf_add_rmsnorm", "bf_rope_qk", "bf_swiglu"} <= set(_C.SYMBOLS)
    lib = _C.lib()
    for name in ("bf_add_rmsnorm", "bf_rope_qk", "bf_swiglu"):
        assert getattr(lib, name).argtypes == _C.SYMBOLS[name][1]
    # 6 int32 + 4 x 3 int64 = 120 bytes, as a C compiler lays out bf_rope_t
    assert ctypes.sizeof(_C.bf_rope_t) == 120 and _C.bf_rope_t.q_stride.offset == 24
    assert ops.BLOCK_CALLS.keys() == {"rmsnorm", "rope", "swiglu"}
    assert "fuse_decoder_blocks" in bf.__all__


def _err():
    return _C.lib().bf_last_error().decode()


def test_add_rmsnorm_refuses_bad_arguments_without_a_device():
    f = _C.lib().bf_add_rmsnorm
    ok = dict(x=4096, res=8192, gamma=16, pd=_C.BF_DT_F32, z=12288, y=16384, dt=_C.BF_DT_BF16, rows=4, N=64)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["x"], a["res"], a["gamma"], a["pd"], a["z"], a["y"], a["dt"], a["rows"], a["N"], 1e-6, None)

    assert call(x=None) == 1 and "null pointer" in _err()
    assert call(y=None) == 1 and "null pointer" in _err()
    assert call(gamma=None) == 1 and "null pointer" in _err()
    assert call(x=4104) == 1 and "16-byte aligned" in _err()
    assert call(z=8) == 1 and "16-byte aligned" in _err()
    assert call(N=60) == 1 and "multiple of 8" in _err()
    assert call(N=8200) == 1 and "at most 8192" in _err()
    assert call(dt=7) == 1 and "unknown dtype" in _err()
    assert call(pd=_C.BF_DT_F16) == 1 and "gamma must be fp32" in _err()
    assert call(rows=-1) == 1 and "bad shape" in _err()
    assert call(rows=0) == 0  # nothing to do: no launch, no device needed


def test_rope_qk_refuses_bad_arguments_without_a_device():
    f = _C.lib().bf_rope_qk

    def shape(D=64, cos_batch=1, stride=64):
        s = _C.bf_rope_t(2, 4, 8, 2, D, cos_batch)
        for name in ("q_stride", "k_stride", "q_out_stride", "k_out_stride"):
            getattr(s, name)[:] = [4 * 8 * D, stride, 8 * D]
        return s

    def call(s, q=4096, cos=16, dt=_C.BF_DT_BF16, cd=_C.BF_DT_F32):
        return f(q, 8192, cos, 32, cd, q, 8192, dt, ctypes.byref(s) if s is not None else None, None)

    assert call(None) == 1 and "shape is NULL" in _err()
    assert call(shape(D=96)) == 1 and "head_dim=96 must be 64 or 128" in _err()
    assert call(shape(cos_batch=3)) == 1 and "cos_batch" in _err()
    assert call(shape(), q=None) == 1 and "null pointer" in _err()
    assert call(shape(), cos=24) == 1 and "16-byte aligned" in _err()
    assert call(shape(stride=60)) == 1 and "multiples of 8" in _err()
    assert call(shape(), dt=9) == 1 and "unknown dtype" in _err()
    assert call(shape(), cd=_C.BF_DT_F16) == 1 and "cos / sin must be fp32" in _err()


def test_swiglu_refuses_bad_arguments_without_a_device():
    f = _C.lib().bf_swiglu
    assert f(None, 64, 4096, 64, 8192, 64, _C.BF_DT_BF16, 4, 64, None) == 1 and "null pointer" in _err()
    assert f(4104, 64, 4096, 64, 8192, 64, _C.BF_DT_BF16, 4, 64, None) == 1 and "16-byte aligned" in _err()
    assert f(4096, 64, 8192, 64, 12288, 64, _C.BF_DT_BF16, 4, 60, None) == 1 and "multiple of 8" in _err()
    assert f(4096, 32, 8192, 64, 12288, 64, _C.BF_DT_BF16, 4, 64, None) == 1 and "row strides" in _err()
    assert f(4096, 68, 8192, 64, 12288, 64, _C.BF_DT_BF16, 4, 64, None) == 1 and "row strides" in _err()
    assert f(4096, 64, 8192, 64, 12288, 64, 5, 4, 64, None) == 1 and "unknown dtype" in _err()
    assert f(4096, 64, 8192, 64, 12288, 64, _C.BF_DT_F32, 0, 64, None) == 0


def test_ops_refuse_cpu_tensors():
    x = torch.randn(4, 64)
    with pytest.raises(_C.BayeFormersAMDError, match="ROCm device"):
        ops.add_rmsnorm(x, None, torch.ones(64), 1e-6)
    with pytest.raises(_C.BayeFormersAMDError, match="ROCm device"):
        ops.swiglu(x, x)
    q = torch.randn(1, 2, 3, 64)
    with pytest.raises(_C.BayeFormersAMDError, match="ROCm device"):
        ops.rope_qk(q, q, torch.ones(1, 3, 64), torch.zeros(1, 3, 64))
    assert not ops.rmsnorm_supported(x, None, torch.nn.LayerNorm(64)) and not ops.swiglu_supported(x, x)


def test_row_stride_of_views():
    buf = torch.zeros(6, 2, 128)
    assert ops._row_stride(buf) == 128 and ops._row_stride(buf.view(12, 128)[:, :64]) == 128
    assert ops._row_stride(buf.view(6, 1, 256)[..., 128:]) == 256  # halves of a stacked buffer at one token per row
    assert ops._row_stride(buf[:, :1]) == 256 and ops._row_stride(buf[:, :, :64].transpose(0, 1)) is None
    assert ops._row_stride(buf[0, 0]) == 128


# ----------------------------------------------------------------------------------------------- which models it rewrites
def _tiny(kind, layers=3, **kw):
    import transformers as tf

    cfg_cls, model_cls = {"llama": (tf.LlamaConfig, tf.LlamaForCausalLM), "mistral": (tf.MistralConfig, tf.MistralForCausalLM),
                          "qwen2": (tf.Qwen2Config, tf.Qwen2ForCausalLM), "qwen3": (tf.Qwen3Config, tf.Qwen3ForCausalLM)}[kind]
    cfg = cfg_cls(hidden_size=128, num_attention_heads=2, num_key_value_heads=1, num_hidden_layers=layers,
                  intermediate_size=256, vocab_size=97, max_position_embeddings=64, tie_word_embeddings=False,
                  head_dim=64, **kw)
    torch.manual_seed(3)
    return model_cls(cfg).eval()


@pytest.mark.parametrize("kind", ["llama", "mistral", "qwen2"])
def test_rewrites_every_layer_once_and_declines_off_device(kind):
    model = _tiny(kind)
    ids = torch.randint(0, 97, (2, 12), generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        ref = model(input_ids=ids, output_hidden_states=True)
    keys = list(model.state_dict().keys())
    assert bf.fuse_decoder_blocks(model) == 3
    assert bf.fuse_decoder_blocks(model) == 0  # nothing is rewritten twice
    assert list(model.state_dict().keys()) == keys  # the recorded next norm is not a child of the layer
    layer = model.model.layers[0]
    assert layer.forward.__func__ is bf._decoder_layer_forward and layer._bf_next_norm[0] is model.model.layers[1].input_layernorm
    assert model.model.layers[-1]._bf_next_norm[0] is model.model.norm
    assert layer.mlp.forward.__func__ is bf._swiglu_mlp_forward
    assert layer.self_attn.forward.__func__ is bf._decoder_attention_forward
    before = dict(ops.BLOCK_CALLS)
    with torch.no_grad():
        got = model(input_ids=ids, output_hidden_states=True)
    # fp32 on the CPU: every fast form declines and the modules' own forwards run — the same bits
    assert torch.equal(got.logits, ref.logits)
    assert all(torch.equal(a, b) for a, b in zip(got.hidden_states, ref.hidden_states))
    assert ops.BLOCK_CALLS == before
    # with gradients recorded as well
    loss = model(input_ids=ids, labels=ids).loss
    loss.backward()
    assert model.model.layers[0].mlp.gate_proj.weight.grad is not None and ops.BLOCK_CALLS == before


def test_converted_model_is_rewritten_too():
    bmodel = bf.to_bayesian(_tiny("llama", layers=2), delta=0.05, freeze=True)
    assert bf.fuse_decoder_blocks(bmodel) == 2 and bf.fuse_decoder_blocks(bmodel) == 0


def test_other_architectures_are_left_alone():
    import transformers as tf

    qwen3 = _tiny("qwen3")
    assert bf.fuse_decoder_blocks(qwen3) == 0
    assert "forward" not in qwen3.model.layers[0].__dict__ and "forward" not in qwen3.model.norm.__dict__
    bert = tf.BertForSequenceClassification(tf.BertConfig(hidden_size=64, num_attention_heads=2, num_hidden_layers=2,
                                                          intermediate_size=128, vocab_size=50))
    assert bf.fuse_decoder_blocks(bert) == 0
    # head sizes the rotary kernel does not take, and an MLP around another activation
    assert bf.fuse_decoder_blocks(_tiny("llama", hidden_act="gelu")) == 0
    import transformers

    cfg = transformers.LlamaConfig(hidden_size=96, num_attention_heads=2, num_key_value_heads=2, num_hidden_layers=2,
                                   intermediate_size=128, vocab_size=50, max_position_embeddings=32)
    assert bf.fuse_decoder_blocks(transformers.LlamaForCausalLM(cfg)) == 0  # head_dim 48
