"""Bayesian mixture-of-experts layers without a GPU: the float64 restatement of tests/moe_ref.py against the framework's own
experts modules, the conversion entry (to_bayesian(experts=...)), the kept-sample byte count, the routing predicate and the
C-ABI table (include/bayeformers_amd_moe.h)."""
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import moe_ref  # noqa: E402

import bayeformers_amd as bf  # noqa: E402
import bayeformers_amd.nn as bnn  # noqa: E402
from bayeformers_amd import _C, ops  # noqa: E402
from bayeformers_amd.nn.layers.experts import is_experts_module  # noqa: E402


def _mixtral_config(**kw):
    from transformers import MixtralConfig

    return MixtralConfig(hidden_size=64, intermediate_size=32, num_local_experts=4, num_experts_per_tok=2, num_attention_heads=4,
                         num_key_value_heads=2, num_hidden_layers=2, vocab_size=128, max_position_embeddings=64,
                         sliding_window=None, tie_word_embeddings=False, **kw)


def _qwen3_moe_config(**kw):
    from transformers import Qwen3MoeConfig

    return Qwen3MoeConfig(hidden_size=64, intermediate_size=96, moe_intermediate_size=32, num_experts=8, num_experts_per_tok=2,
                          num_attention_heads=4, num_key_value_heads=2, head_dim=16, num_hidden_layers=2, vocab_size=128,
                          max_position_embeddings=64, decoder_sparse_step=1, mlp_only_layers=[], tie_word_embeddings=False, **kw)


def _tiny_mixtral():
    from transformers import MixtralForCausalLM

    torch.manual_seed(0)
    return MixtralForCausalLM(_mixtral_config()).eval()


def _framework_experts(kind):
    if kind == "mixtral":
        from transformers.models.mixtral.modeling_mixtral import MixtralExperts

        mod = MixtralExperts(_mixtral_config())
    else:
        from transformers.models.qwen3_moe.modeling_qwen3_moe import Qwen3MoeExperts

        mod = Qwen3MoeExperts(_qwen3_moe_config())
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for p in mod.parameters():
            p.copy_(0.3 * torch.randn(p.shape, generator=g))
    return mod.double()


# --------------------------------------------------------------------------------------------------- 1. the restatement
@pytest.mark.parametrize("kind", ["mixtral", "qwen3_moe"])
def test_reference_is_the_framework_experts_forward(kind):
    """S = 1: tests/moe_ref.py stage by stage, and its vectorised forward, equal `*Experts.forward` in float64."""
    mod = _framework_experts(kind)
    E, I, H, k, R = mod.num_experts, mod.intermediate_dim, mod.hidden_dim, 2, 23
    g = torch.Generator().manual_seed(1)
    x = torch.randn(R, H, generator=g, dtype=torch.float64)
    logits = torch.randn(R, E, generator=g, dtype=torch.float64)
    wts, idx = torch.topk(torch.softmax(logits, -1), k, dim=-1)
    with torch.no_grad():
        want = mod(x, idx, wts)
    w_gu, w_d = mod.gate_up_proj.detach()[None], mod.down_proj.detach()[None]
    h = moe_ref.gate_up(x, idx, w_gu, 1)
    y = moe_ref.down(h, idx, w_d, 1)
    got = moe_ref.combine(y, idx, wts, E)
    assert (got - want).abs().max().item() <= 1e-12
    assert (moe_ref.forward(x, idx, wts, w_gu, w_d, 1) - want).abs().max().item() <= 1e-12
    # the composite the layer's unsupported calls and its backward run is the same function
    comp = ops.moe_composite(x, idx, wts, w_gu, w_d, 1, mod.act_fn)
    assert (comp - want).abs().max().item() <= 1e-12
    # the sentinel: a slot sent to E contributes nothing (the framework's own loop cannot take it: its one_hot has E classes)
    idx_d = idx.clone()
    idx_d[::3, 1] = E
    dropped = moe_ref.forward(x, idx_d, wts, w_gu, w_d, 1)
    keep = torch.where(idx_d == E, torch.zeros_like(wts), wts)
    with torch.no_grad():
        want_d = mod(x, idx, keep)
    assert (dropped - want_d).abs().max().item() <= 1e-12
    assert (moe_ref.combine(moe_ref.down(moe_ref.gate_up(x, idx_d, w_gu, 1), idx_d, w_d, 1), idx_d, wts, E)
            - want_d).abs().max().item() <= 1e-12
    assert (ops.moe_composite(x, idx_d, wts, w_gu, w_d, 1, mod.act_fn) - want_d).abs().max().item() <= 1e-12


def test_reference_samples_are_sample_major():
    """S > 1: slab s of the rows meets weights s — the reference equals S separate S = 1 calls."""
    S, M, E, k, H, I = 3, 5, 4, 2, 16, 8
    g = torch.Generator().manual_seed(2)
    x = torch.randn(S * M, H, generator=g, dtype=torch.float64)
    w_gu = torch.randn(S, E, 2 * I, H, generator=g, dtype=torch.float64)
    w_d = torch.randn(S, E, H, I, generator=g, dtype=torch.float64)
    wts, idx = torch.topk(torch.softmax(torch.randn(S * M, E, generator=g, dtype=torch.float64), -1), k, dim=-1)
    idx[3, 0] = E
    whole = moe_ref.forward(x, idx, wts, w_gu, w_d, S)
    for s in range(S):
        sl = slice(s * M, (s + 1) * M)
        part = moe_ref.forward(x[sl], idx[sl], wts[sl], w_gu[s:s + 1], w_d[s:s + 1], 1)
        assert torch.allclose(whole[sl], part, rtol=1e-12, atol=1e-12)
    stages = moe_ref.combine(moe_ref.down(moe_ref.gate_up(x, idx, w_gu, S), idx, w_d, S), idx, wts, E)
    assert torch.allclose(stages, whole, rtol=1e-12, atol=1e-12)
    assert torch.allclose(ops.moe_composite(x, idx, wts, w_gu, w_d, S, torch.nn.functional.silu), whole, rtol=1e-12, atol=1e-12)


def test_reference_route():
    S, M, E, k = 2, 5, 3, 2
    idx = torch.tensor([[0, 1], [2, 0], [3, 1], [1, 0], [0, 2],      # sample 0 (3 = E: dropped)
                        [2, 1], [2, 0], [1, 3], [2, 1], [0, 2]])     # sample 1
    offsets, slots = moe_ref.route(idx, S, E)
    assert offsets.tolist() == [0, 4, 7, 9, 11, 14, 18]
    assert slots.tolist() == [0, 3, 7, 8, 1, 5, 6, 2, 9, 13, 18, 11, 14, 17, 10, 12, 16, 19]
    nt = moe_ref.max_tiles(S, E, S * M, k)
    assert nt == 20 // 16 + 6 == ops.moe_max_tiles(S, E, S * M, k)
    t = moe_ref.tiles(offsets, nt)
    assert t[:6].tolist() == [[0, 0, 4], [1, 4, 3], [2, 7, 2], [3, 9, 2], [4, 11, 3], [5, 14, 4]] and not t[6:].any()
    # a group longer than a tile
    offsets, slots = moe_ref.route(torch.zeros(37, 1, dtype=torch.long), 1, 2)
    assert moe_ref.tiles(offsets, 4).tolist() == [[0, 0, 16], [0, 16, 16], [0, 32, 5], [0, 0, 0]]


# ----------------------------------------------------------------------------------------------------- 2. the conversion
def _expected_keys(src, swap_experts, moped=False):
    """The converted model's state-dict keys from the UNCONVERTED module list: an nn.Linear's keys become a bnn.Linear's, an
    experts module's (when swapped) a bnn.Experts', everything else stays.  moped: the priors are Gaussians (delta=...)."""
    keys = set()
    for name, mod in src.named_modules():
        prefix = "model." + (name + "." if name else "")
        if mod.__class__ is torch.nn.Linear:
            twin = bnn.Linear(mod.in_features, mod.out_features, mod.bias is not None)
            if moped:
                twin.weight_prior = bnn.Gaussian(torch.Size((1,)))
            keys |= {prefix + k for k in twin.state_dict()}
        elif swap_experts and is_experts_module(mod):
            twin = bnn.Experts(2, 8, 8)
            if moped:
                twin.gate_up_proj_prior, twin.down_proj_prior = bnn.Gaussian(torch.Size((1,))), bnn.Gaussian(torch.Size((1,)))
            keys |= {prefix + k for k in twin.state_dict()}
        else:
            own = list(mod.named_parameters(recurse=False)) + [(n, b) for n, b in mod.named_buffers(recurse=False)
                                                               if n not in mod._non_persistent_buffers_set]
            keys |= {prefix + n for n, _ in own}
    return keys


def test_experts_keyword_off_keeps_todays_conversion():
    src = _tiny_mixtral()
    for kw in ({}, {"experts": False}):
        torch.manual_seed(3)
        model = bf.to_bayesian(src, **kw)
        assert set(model.state_dict()) == _expected_keys(src, False)
        assert not any(isinstance(m, bnn.Experts) for m in model.modules())
        assert sum(is_experts_module(m) for m in model.modules()) == 2
    a = bf.to_bayesian(src, delta=0.05)
    b = bf.to_bayesian(src, delta=0.05, experts=False)
    sa, sb = a.state_dict(), b.state_dict()
    assert sa.keys() == sb.keys() and all(torch.equal(sa[k], sb[k]) for k in sa)


def test_to_bayesian_experts_swaps_every_experts_module():
    src = _tiny_mixtral()
    delta = 0.05
    model = bf.to_bayesian(src, delta=delta, experts=True)
    assert set(model.state_dict()) == _expected_keys(src, True, moped=True)
    assert set(bf.to_bayesian(src, experts=True).state_dict()) == _expected_keys(src, True)
    names = [n for n, m in src.named_modules() if is_experts_module(m)]
    assert len(names) == 2
    layers = [model.model.get_submodule(n) for n in names]
    assert all(isinstance(l, bnn.Experts) and not isinstance(l, bnn.Linear) for l in layers)
    assert [l for l in model.modules() if isinstance(l, bnn.Experts)] == layers
    own = {"gate_up_proj.mu", "gate_up_proj.rho", "down_proj.mu", "down_proj.rho", "log_prior", "log_variational_posterior"}
    for n, l in zip(names, layers):
        ref = src.get_submodule(n)
        assert own <= set(l.state_dict())
        assert (l.num_experts, l.hidden_dim, l.intermediate_dim) == (4, 64, 32) and l.act_fn.__class__ is ref.act_fn.__class__
        for g, prior, w in ((l.gate_up_proj, l.gate_up_proj_prior, ref.gate_up_proj), (l.down_proj, l.down_proj_prior, ref.down_proj)):
            # bnn.Linear's MOPED formula: mu = w, rho = log(exp(delta |w|) - 1) with -inf -> 0, prior N(w, softplus(1))
            rho = torch.log(torch.exp(delta * torch.abs(w.data)) - 1.0)
            rho[rho == float("-inf")] = 0.0
            assert g.mu.dtype == torch.float32 and torch.equal(g.mu, w) and torch.equal(g.rho, rho) and g.mu.requires_grad
            assert isinstance(prior, bnn.Gaussian) and torch.equal(prior.mu, w) and torch.equal(prior.rho, torch.ones_like(w))
        streams = [(g is t, sid) for (g, _, sid), t in zip(l.gaussians(), (l.gate_up_proj, l.down_proj))]
        assert streams == [(True, 2 * l.layer_id), (True, 2 * l.layer_id + 1)]
    # the router stays the framework's and deterministic; the attention projections and the head convert as ever
    gate = model.model.get_submodule(names[0].rsplit(".", 1)[0] + ".gate")
    assert gate.__class__ is src.get_submodule(names[0].rsplit(".", 1)[0] + ".gate").__class__
    assert isinstance(model.model.lm_head, bnn.Linear)
    # frozen means, and the model's layer order gives the Philox streams
    frozen = bf.to_bayesian(src, delta=delta, freeze=True, experts=True)
    fl = [m for m in frozen.modules() if isinstance(m, bnn.Experts)]
    assert all(not l.gate_up_proj.mu.requires_grad and not l.down_proj.mu.requires_grad and l.down_proj.rho.requires_grad for l in fl)
    # the experts take the Philox streams after every other layer's: those keep the draws of the conversion without experts
    kids = frozen.fused_children()
    assert len(kids) == 2 * 4 + 2 + 1
    assert [l.layer_id for l in kids if not isinstance(l, bnn.Experts)] == list(range(9))
    assert [l.layer_id for l in kids if isinstance(l, bnn.Experts)] == [9, 10]
    assert [l.layer_id for l in bf.to_bayesian(src, delta=delta).fused_children()] == list(range(9))
    # without delta: the initialization's draw and the given prior, as bnn.Linear
    plain = bf.to_bayesian(src, experts=True)
    pl = [m for m in plain.modules() if isinstance(m, bnn.Experts)][0]
    assert pl.gate_up_proj_prior is bnn.DEFAULT_SCALED_GAUSSIAN_MIXTURE and pl.gate_up_proj.rho.max() <= -4.0


def test_structure_test_leaves_other_modules_alone():
    class Biased(torch.nn.Module):  # gpt-oss's form: biases beside the two tensors
        def __init__(self):
            super().__init__()
            self.num_experts, self.act_fn = 2, torch.nn.SiLU()
            self.gate_up_proj = torch.nn.Parameter(torch.zeros(2, 16, 8))
            self.gate_up_proj_bias = torch.nn.Parameter(torch.zeros(2, 16))
            self.down_proj = torch.nn.Parameter(torch.zeros(2, 8, 8))

    class Plain(torch.nn.Module):
        def __init__(self, shape_d=(2, 8, 8), with_attrs=True):
            super().__init__()
            if with_attrs:
                self.num_experts, self.act_fn = 2, torch.nn.SiLU()
            self.gate_up_proj = torch.nn.Parameter(torch.zeros(2, 16, 8))
            self.down_proj = torch.nn.Parameter(torch.zeros(*shape_d))

    assert is_experts_module(Plain()) and not is_experts_module(Biased())
    assert not is_experts_module(Plain(shape_d=(2, 8, 16))) and not is_experts_module(Plain(with_attrs=False))
    assert not is_experts_module(torch.nn.Linear(4, 4)) and not is_experts_module(bnn.Experts(2, 8, 8))
    net = torch.nn.Sequential(Biased(), Plain(), torch.nn.Linear(8, 8))
    model = bf.to_bayesian(net, experts=True)
    assert [type(m).__name__ for m in model.model] == ["Biased", "Experts", "Linear"]
    assert isinstance(model.model[2], bnn.Linear)


def test_layer_surface():
    layer = bnn.Experts(4, 16, 8)
    assert layer.gate_up_proj.mu.shape == (4, 16, 16) and layer.down_proj.mu.shape == (4, 16, 8)
    half = layer.to(torch.bfloat16)  # fp32 masters whatever the model's dtype
    assert half.gate_up_proj.mu.dtype == torch.float32 and half.down_proj.rho.dtype == torch.float32
    with pytest.raises(_C.BayeFormersAMDError, match="ROCm device"):
        layer(torch.zeros(2, 16), torch.zeros(2, 2, dtype=torch.long), torch.ones(2, 2))


def test_kept_weight_bytes_counts_the_experts():
    src = _tiny_mixtral()
    S = 3
    base = bf.kept_weight_bytes(bf.to_bayesian(src), S, torch.bfloat16)
    full = bf.kept_weight_bytes(bf.to_bayesian(src, experts=True), S, torch.bfloat16)
    assert full - base == 2 * S * 4 * (2 * 32 * 64 + 64 * 32) * 2  # two layers, E = 4, both tensors, 2 bytes
    assert bf.kept_weight_bytes(bnn.Model(bnn.Experts(2, 8, 8)), 2, torch.float32) == 2 * 2 * 3 * 8 * 8 * 4


def test_refusals_that_name_experts():
    model = bf.to_bayesian(_tiny_mixtral(), delta=0.05, experts=True).eval()
    prev = {torch.float32: "fp32", torch.bfloat16: "bf16", torch.float16: "fp16"}[bf.get_compute_dtype()]
    bf.set_compute_dtype("bf16")
    try:
        with torch.no_grad(), pytest.raises(ValueError, match="Experts"):
            with model.pinned_samples(keep_weights="fp8"):
                pass
        with torch.no_grad(), pytest.raises(ValueError, match="Experts"):
            with model.posterior_mean():
                pass
    finally:
        bf.set_compute_dtype(prev)


# ------------------------------------------------------------------------------------------------- 3. predicate and ABI
def test_moe_supported_is_the_kernels_class():
    silu = torch.nn.SiLU()
    from transformers.activations import ACT2FN

    assert ops.moe_supported(torch.bfloat16, 64, 32, 4, 2, silu) and ops.moe_supported(torch.float16, 96, 40, 8, 8, ACT2FN["silu"])
    assert ops.moe_supported(torch.bfloat16, 64, 32, 128, 8, torch.nn.functional.silu, S=2)
    assert not ops.moe_supported(torch.float32, 64, 32, 4, 2, silu)
    assert not ops.moe_supported(torch.bfloat16, 64, 36, 4, 2, silu)
    assert not ops.moe_supported(torch.bfloat16, 60, 32, 4, 2, silu)
    assert not ops.moe_supported(torch.bfloat16, 64, 32, 4, 2, ACT2FN["gelu"])
    assert not ops.moe_supported(torch.bfloat16, 64, 32, 4, ops.MOE_MAX_TOPK + 1, silu)
    assert ops.moe_supported(torch.bfloat16, 64, 32, ops.MOE_MAX_GROUPS // 2, 2, silu, S=2)
    assert not ops.moe_supported(torch.bfloat16, 64, 32, ops.MOE_MAX_GROUPS // 2 + 1, 2, silu, S=2)
    assert not ops.moe_supported(torch.bfloat16, 64, 32, 4, 2, silu, torch.zeros(4, 64, dtype=torch.bfloat16))  # a host tensor


def test_default_route_follows_the_measurement():
    """profiles/bayesian_moe.md: the kernels up to 128 rows per (sample, expert) group on average, the loop above."""
    silu = torch.nn.SiLU()
    assert ops.moe_kernel_wins(4, 8, 2, 8) and ops.moe_kernel_wins(4, 128, 8, 4096)   # decode steps; Qwen3-MoE-shaped prefill
    assert not ops.moe_kernel_wins(4, 8, 2, 4096)                                      # Mixtral-shaped prefill: 256 rows a group
    assert ops.moe_kernel_wins(4, 8, 2, 2048) and not ops.moe_kernel_wins(4, 8, 2, 2064)
    assert ops.moe_supported(torch.bfloat16, 4096, 14336, 8, 2, silu, S=4, rows=8)
    assert not ops.moe_supported(torch.bfloat16, 4096, 14336, 8, 2, silu, S=4, rows=4096)
    assert ops.moe_supported(torch.bfloat16, 4096, 14336, 8, 2, silu, S=4)  # the kernels' class itself


def test_header_declares_the_bound_entries():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "bayeformers_amd_moe.h")).read()
    assert (f"#define BF_MOE_TILE_ROWS {_C.BF_MOE_TILE_ROWS}" in text and f"#define BF_MOE_MAX_TOPK {_C.BF_MOE_MAX_TOPK}" in text
            and f"#define BF_MOE_MAX_GROUPS {_C.BF_MOE_MAX_GROUPS}" in text)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(bf_moe_\w+)\s*\(", text))
    assert declared == set(_C.MOE_SYMBOLS)
    others = [_C.SYMBOLS, _C.SOFTCAP_SYMBOLS, _C.FAMILY_BLOCK_SYMBOLS, _C.FAMILY_BLOCK_BWD_SYMBOLS, _C.PACKED_SYMBOLS,
              _C.FP8_SYMBOLS, _C.KV8_SYMBOLS, _C.CHUNK_SYMBOLS, _C.ENCODER_ANY_SYMBOLS, _C.LORA_SYMBOLS, _C.LRT_SYMBOLS]
    assert not any(set(_C.MOE_SYMBOLS) & set(t) for t in others)
    lib = _C.lib()
    for name, (res, args) in _C.MOE_SYMBOLS.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    # the size twins answer without a device; refusals come before any launch and name the entry and the condition
    assert lib.bf_moe_max_tiles(2, 3, 10, 2) == moe_ref.max_tiles(2, 3, 10, 2) == 7
    assert lib.bf_moe_route_workspace_bytes(2, 3, 10, 2) >= 6 * 4
    assert lib.bf_moe_gate_up_workspace_bytes(2, 3, 10, 2, 64, 32, _C.BF_DT_BF16) == 0
    assert lib.bf_moe_down_workspace_bytes(2, 3, 10, 2, 64, 32, _C.BF_DT_BF16) == 0 and lib.bf_moe_combine_workspace_bytes(10, 2, 64) == 0
    bf16 = _C.BF_DT_BF16
    for (S, E, R, k, H, I, dt), word in (((1, 4, 4, 2, 64, 36, bf16), "I % 8 == 0"), ((1, 4, 4, 2, 60, 32, bf16), "H % 8 == 0"),
                                         ((1, 4, 4, 2, 64, 32, _C.BF_DT_F32), "16-bit"), ((1, 4, 4, 17, 64, 32, bf16), "k <= 16"),
                                         ((2, 2049, 4, 2, 64, 32, bf16), "S*E <= 4096"), ((3, 4, 4, 2, 64, 32, bf16), "R % S == 0")):
        for entry in ("bf_moe_gate_up", "bf_moe_down"):
            rc = getattr(lib, entry)(None, None, None, None, None, dt, S, E, R, k, H, I, None, 0, None)
            msg = lib.bf_last_error().decode()
            assert rc == 1 and entry in msg and word in msg, msg
    rc = lib.bf_moe_route(None, None, None, None, 2, 2049, 4, 2, None, 0, None)
    assert rc == 1 and "bf_moe_route" in lib.bf_last_error().decode() and "S*E <= 4096" in lib.bf_last_error().decode()
    rc = lib.bf_moe_combine(None, None, None, _C.BF_DT_F16, None, bf16, 4, 4, 2, 64, None, 0, None)
    assert rc == 1 and "bf_moe_combine" in lib.bf_last_error().decode() and "weights dtype" in lib.bf_last_error().decode()
