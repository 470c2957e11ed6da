"""Bayesian LoRA without a GPU: the float64 reference of tests/lora_ref.py against torch.autograd, the conversion entry
(to_bayesian_lora, lora_state_dict), the kept-sample byte count and the C-ABI table (include/bayeformers_amd_lora.h)."""
import ctypes
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lora_ref  # noqa: E402

import bayeformers_amd as bf  # noqa: E402
import bayeformers_amd.nn as bnn  # noqa: E402
from bayeformers_amd import _C, ops  # noqa: E402

TARGETS = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")


def test_reference_gradients_match_autograd():
    S, M, N, K, r, scale = 3, 5, 24, 16, 8, 2.0
    g = torch.Generator().manual_seed(3)
    x = torch.randn(S * M, K, generator=g, dtype=torch.float64, requires_grad=True)
    mu = (0.3 * torch.randn(r, K, generator=g)).double().requires_grad_()
    rho = (-2.0 + 0.5 * torch.randn(r, K, generator=g)).double().requires_grad_()
    b = torch.randn(N, r, generator=g, dtype=torch.float64, requires_grad=True)
    w0 = torch.randn(N, K, generator=g, dtype=torch.float64, requires_grad=True)
    b0 = torch.randn(N, generator=g, dtype=torch.float64)
    dy = torch.randn(S * M, N, generator=g, dtype=torch.float64)
    eps = lora_ref.eps_host((r, K), 0x5EED, 7, S, 12)
    assert eps.shape == (S, r, K) and not torch.equal(eps[0], eps[1])
    a_s = mu[None] + torch.nn.functional.softplus(rho)[None] * eps  # the differentiable float64 forward
    y, h = lora_ref.forward(x, a_s, b, w0, b0, scale, S)
    for s in range(S):  # the restatement is the formula, sample by sample
        xs = x[s * M:(s + 1) * M]
        assert torch.allclose(y[s * M:(s + 1) * M], xs @ w0.t() + b0 + scale * (xs @ a_s[s].t()) @ b.t(), rtol=1e-12, atol=1e-12)
    (y * dy).sum().backward()
    hand = lora_ref.backward(x.detach(), dy, a_s.detach(), b.detach(), w0.detach(), scale, S, eps, rho.detach())
    assert torch.allclose(hand["dx"], x.grad, rtol=1e-10, atol=1e-10)
    assert torch.allclose(hand["dmu"], mu.grad, rtol=1e-10, atol=1e-10)
    assert torch.allclose(hand["drho"], rho.grad, rtol=1e-10, atol=1e-10)
    assert torch.allclose(hand["dB"], b.grad, rtol=1e-10, atol=1e-10)
    assert w0.grad is not None  # autograd has a dW0; the layer has none (frozen base): nothing in `hand` carries it
    assert set(hand) == {"g", "dx", "dA", "dB", "dmu", "drho"}


def test_sample_a_matches_fp32_formula():
    r, K, S = 8, 16, 2
    mu, rho = torch.randn(r, K), torch.full((r, K), -4.5)
    eps = lora_ref.eps_host((r, K), 1, 0, S, 4)
    a = lora_ref.sample_a(mu, rho, eps)
    assert a.dtype == torch.float64 and a.shape == (S, r, K)
    assert torch.equal(a[1].float(), mu + torch.nn.functional.softplus(rho) * eps[1].float())


def _tiny_llama():
    from transformers import LlamaConfig, LlamaForCausalLM

    cfg = LlamaConfig(hidden_size=64, num_attention_heads=4, num_key_value_heads=2, num_hidden_layers=2, intermediate_size=96,
                      vocab_size=128, max_position_embeddings=64, tie_word_embeddings=False)
    torch.manual_seed(0)
    return LlamaForCausalLM(cfg).eval()


def test_to_bayesian_lora_swaps_targets_and_freezes_the_rest():
    src = _tiny_llama()
    model = bf.to_bayesian_lora(src, r=8, alpha=16)
    assert isinstance(model, bnn.Model)
    swapped = {n for n, m in model.named_modules() if isinstance(m, bnn.LoRALinear)}
    want = {n for n, m in src.named_modules() if m.__class__ is torch.nn.Linear and n.endswith(TARGETS)}
    assert len(want) == 14 and swapped == {"model." + n for n in want}
    assert isinstance(model.model.lm_head, torch.nn.Linear)  # not a target: left alone
    assert not any(isinstance(m, bnn.Linear) for m in model.modules())
    for n, m in model.named_modules():
        if isinstance(m, bnn.LoRALinear):
            ref = src.get_submodule(n[len("model."):])
            assert (m.r, m.scale) == (8, 2.0) and m.base_bias is None
            assert torch.equal(m.base_weight, ref.weight) and not m.base_weight.requires_grad
            assert m.lora_B.dtype == torch.float32 and m.lora_B.shape == (ref.out_features, 8) and not m.lora_B.any()
            assert m.lora_A.mu.shape == (8, ref.in_features) and m.lora_A.mu.dtype == torch.float32
            bound = 1.0 / ref.in_features ** 0.5  # kaiming_uniform_(a=sqrt(5)) on [r, K]: U(-1/sqrt(K), 1/sqrt(K))
            assert m.lora_A.mu.abs().max() <= bound and m.lora_A.mu.abs().max() > 0.5 * bound
            assert -5.0 <= m.lora_A.rho.min() and m.lora_A.rho.max() <= -4.0
    trainable = {n for n, p in model.named_parameters() if p.requires_grad}
    assert trainable == set(bf.lora_state_dict(model)) and len(trainable) == 3 * 14
    assert all(n.endswith(("lora_A.mu", "lora_A.rho", "lora_B")) for n in trainable)
    # the source model is untouched (deep copy)
    assert all(p.requires_grad for p in src.parameters())


def test_from_frequentist_shares_the_source_storage():
    lin = torch.nn.Linear(16, 24)
    layer = bnn.LoRALinear.from_frequentist(lin, r=8, alpha=8)
    assert layer.base_weight.data_ptr() == lin.weight.data_ptr() and layer.base_bias.data_ptr() == lin.bias.data_ptr()
    assert not layer.base_weight.requires_grad and not layer.base_bias.requires_grad
    assert [g is layer.lora_A and sid == 2 * layer.layer_id for g, _, sid in layer.gaussians()] == [True]
    assert not isinstance(layer, bnn.Linear)
    half = layer.to(torch.bfloat16)  # the base follows the model's dtype, the fp32 masters stay
    assert half.base_weight.dtype == torch.bfloat16 and half.lora_B.dtype == torch.float32
    assert half.lora_A.mu.dtype == torch.float32


def test_lora_state_dict_round_trips():
    model = bf.to_bayesian_lora(_tiny_llama(), r=8)
    sd = {k: torch.randn_like(v) for k, v in bf.lora_state_dict(model).items()}
    full = set(model.state_dict())
    assert set(sd) <= full
    other = bf.to_bayesian_lora(_tiny_llama(), r=8)
    missing, unexpected = other.load_state_dict(sd, strict=False)
    assert not unexpected and set(missing) == full - set(sd)
    got = bf.lora_state_dict(other)
    assert all(torch.equal(got[k], sd[k]) for k in sd)


def test_to_bayesian_lora_refusals():
    src = _tiny_llama()
    with pytest.raises(ValueError, match="target_modules"):
        bf.to_bayesian_lora(src, r=8, target_modules=("no_such_proj",))
    for bad in (0, -8, 8.0, True, "8"):
        with pytest.raises(ValueError, match="positive int"):
            bf.to_bayesian_lora(src, r=bad)


def test_kept_weight_bytes_counts_the_adapters_only():
    model = bf.to_bayesian_lora(_tiny_llama(), r=8)
    S = 3
    per_layer = 4 * 64 + 2 * 64 + 96  # K of q/k/v/o (64 each), gate/up (64 each), down (96)
    assert bf.kept_weight_bytes(model, S, torch.bfloat16) == 2 * S * 8 * per_layer * 2
    assert bf.kept_weight_bytes(model, S, torch.bfloat16, fp8=True) == 2 * S * 8 * per_layer * 2  # never FP8
    # beside full-Bayesian layers they add to what those keep
    mixed = bnn.Model(torch.nn.Sequential(bnn.Linear(16, 8), bnn.LoRALinear(8, 8, r=8)))
    assert bf.kept_weight_bytes(mixed, S, torch.float16) == S * (16 * 8 * 2 + 8 * 4) + S * 8 * 8 * 2


def test_lora_supported_is_the_kernels_class():
    assert ops.lora_supported(torch.bfloat16, 64, 64, 8) and ops.lora_supported(torch.float16, 264, 136, 64)
    assert not ops.lora_supported(torch.float32, 64, 64, 8)
    assert not ops.lora_supported(torch.bfloat16, 64, 64, 12)
    assert not ops.lora_supported(torch.bfloat16, 64, 60, 8)
    assert not ops.lora_supported(torch.bfloat16, 60, 64, 8)
    assert not ops.lora_supported(torch.bfloat16, 64, 64, 72)


def test_header_declares_the_bound_entries():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "bayeformers_amd_lora.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(bf_lora_\w+)\s*\(", text))
    assert declared == set(_C.LORA_SYMBOLS)
    others = [_C.SYMBOLS, _C.SOFTCAP_SYMBOLS, _C.FAMILY_BLOCK_SYMBOLS, _C.FAMILY_BLOCK_BWD_SYMBOLS, _C.PACKED_SYMBOLS,
              _C.FP8_SYMBOLS, _C.KV8_SYMBOLS, _C.CHUNK_SYMBOLS, _C.ENCODER_ANY_SYMBOLS]
    assert not any(set(_C.LORA_SYMBOLS) & set(t) for t in others)
    lib = _C.lib()
    for name, (res, args) in _C.LORA_SYMBOLS.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    # the size twins answer without a device; refusals come before any launch and name the condition
    assert lib.bf_lora_fwd_workspace_bytes(2, 5, 64, 64, 8, _C.BF_DT_BF16) == 0
    assert lib.bf_lora_bwd_workspace_bytes(2, 5, 64, 64, 8, _C.BF_DT_BF16) > 0
    for (N, K, r), word in (((64, 64, 12), "r % 8 == 0"), ((64, 60, 8), "K % 8 == 0"), ((64, 64, 72), "8 <= r <= 64")):
        rc = lib.bf_lora_fwd(None, None, None, None, None, ctypes.c_float(1.0), _C.BF_DT_BF16, 1, 1, N, K, r, None, 0, None)
        assert rc == 1 and word in lib.bf_last_error().decode()
