# -*- coding: utf-8 -*-
"""bayeformers_amd — MI355X-native Monte-Carlo variational forward path with the BayeFormers API.

    from bayeformers_amd import to_bayesian
    import bayeformers_amd.nn as bnn

`to_bayesian` mirrors /root/reference/bayeformers/__init__.py:19-63.
"""
import os
import threading
import types
from copy import deepcopy
from typing import Optional, Union

import torch.nn

from . import nn  # noqa: F401  (bayeformers_amd.nn)
from .nn import TORCH2BAYE
from . import random as bfr
from .nn.model import Model
from .nn.parameters.base import Parameter
from .nn.parameters.gaussian import DEFAULT_SCALED_GAUSSIAN_MIXTURE
from .nn.parameters.initializations import DEFAULT_UNIFORM, Initialization
from .attention import (_ATTENTION_NAME, _CHUNKED_ATTENTION, _attention_interface, _causal_attention,  # noqa: F401
                        _marks_of, _padding_mask_interface, _softcap_eager, chunked_attention, chunked_attention_enabled,
                        encoder_ragged_attention, encoder_ragged_attention_enabled, fuse_attention, packed_attention,
                        packed_attention_enabled, ragged_attention, ragged_attention_enabled, softcap_attention,
                        softcap_attention_enabled)
from .ops import invalidate_caches  # noqa: F401
from .plan import kept_weight_bytes, kv_cache_bytes  # noqa: F401
from .random import (get_compute_dtype, manual_seed, set_compute_dtype, set_kl_gradient,  # noqa: F401
                     use_device_counter)

__all__ = ["to_bayesian", "to_bayesian_lora", "lora_state_dict", "invalidate_caches", "fuse_activations", "fuse_residual_layernorm", "fuse_shared_inputs", "fuse_ffn_pairs", "fuse_attention", "fuse_embeddings", "fuse_decoder_blocks", "enable_embedding", "nn", "manual_seed", "set_compute_dtype", "get_compute_dtype",
           "use_device_counter", "set_kl_gradient", "kept_weight_bytes", "kv_cache_bytes", "local_reparameterization"]


def to_bayesian(model: torch.nn.Module, initialization: Optional[Initialization] = DEFAULT_UNIFORM,
                prior: Optional[Parameter] = DEFAULT_SCALED_GAUSSIAN_MIXTURE, delta: float = None,
                freeze: bool = False, experts: bool = False) -> Model:
    """Deep-copy `model`, swap every layer whose exact class is in TORCH2BAYE for its Bayesian equivalent
    (`from_frequentist(layer, initialization, prior, delta, freeze)`, children visited in `named_children` order,
    depth first) and wrap the result in `bnn.Model`.

    Arguments / keyword arguments are the reference's: `delta` not None selects MOPED initialisation from the
    pretrained weights (Krishnan et al., arXiv:1906.05323), `freeze` freezes the posterior means.

    experts=True (an extension, off by default: the conversion and its state dict are otherwise what they were): also swap
    every child that is a mixture-of-experts block's experts module BY STRUCTURE (nn.layers.experts.is_experts_module: 3-D
    parameters gate_up_proj [E, 2I, H] and down_proj [E, H, I], `num_experts` and `act_fn`, no other parameter of its own —
    transformers' MixtralExperts, Qwen3MoeExperts and their relatives) for a bnn.Experts with the same arguments.  Routers
    stay deterministic; experts with biases (gpt-oss) stay untouched; a shared expert made of nn.Linear layers (Qwen2-MoE)
    converts as it always did."""
    from .nn.layers.experts import is_experts_module

    def swap(module):
        for name, child in module.named_children():
            bayesian_cls = TORCH2BAYE.get(child.__class__)
            if bayesian_cls is None and experts and is_experts_module(child):
                bayesian_cls = nn.Experts
            if bayesian_cls is not None:
                setattr(module, name, bayesian_cls.from_frequentist(child, initialization, prior, delta, freeze))
            swap(child)

    new_model = deepcopy(model)
    swap(new_model)
    return Model(model=new_model)


LORA_TARGET_MODULES = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")


def to_bayesian_lora(model: torch.nn.Module, r: int = 16, alpha: float = 32, target_modules=LORA_TARGET_MODULES,
                     initialization: Optional[Initialization] = DEFAULT_UNIFORM,
                     prior: Optional[Parameter] = DEFAULT_SCALED_GAUSSIAN_MIXTURE) -> Model:
    """Deep-copy `model`, put a Bayesian rank-`r` adapter (bnn.LoRALinear: a Gaussian posterior on the LoRA A factor, a plain
    B factor starting at zero, scale alpha / r) on every child whose exact class is nn.Linear and whose name ends with one of
    `target_modules`, freeze everything else and wrap the result in `bnn.Model`.  The pretrained weights stay where they are,
    shared by all Monte-Carlo samples; a freshly converted model computes the pretrained function.  Only `lora_A.mu`,
    `lora_A.rho` and `lora_B` of the adapters require gradients afterwards (`lora_state_dict` returns exactly those).

    Not covered: LoRA dropout, a Bayesian B, DoRA / rsLoRA scaling, adapters on nn.Embedding or fused-QKV modules, merging
    adapters into the base."""
    if isinstance(r, bool) or not isinstance(r, int) or r < 1:
        raise ValueError(f"to_bayesian_lora: r={r!r} (a positive int)")
    targets = (target_modules,) if isinstance(target_modules, str) else tuple(target_modules)
    swapped = []

    def swap(module):
        for name, child in module.named_children():
            if child.__class__ is torch.nn.Linear and name.endswith(targets):
                setattr(module, name, nn.LoRALinear.from_frequentist(child, r, alpha, initialization, prior))
                swapped.append(name)
            else:
                swap(child)

    new_model = deepcopy(model)
    swap(new_model)
    if not swapped:
        raise ValueError(f"to_bayesian_lora: no nn.Linear child is named like one of target_modules={targets}")
    adapters = {id(p) for m in new_model.modules() if isinstance(m, nn.LoRALinear)
                for p in (m.lora_A.mu, m.lora_A.rho, m.lora_B)}
    for p in new_model.parameters():
        p.requires_grad = id(p) in adapters
    return Model(model=new_model)


def lora_state_dict(model: torch.nn.Module) -> dict:
    """The adapter tensors of a `to_bayesian_lora` model alone — `<layer>.lora_A.mu`, `<layer>.lora_A.rho`, `<layer>.lora_B`
    under their state-dict keys (detached, not copied): what a fine-tuning run has to save.  Load it back with
    `model.load_state_dict(sd, strict=False)`."""
    out = {}
    for name, m in model.named_modules():
        if isinstance(m, nn.LoRALinear):
            prefix = name + "." if name else ""
            out[prefix + "lora_A.mu"] = m.lora_A.mu.detach()
            out[prefix + "lora_A.rho"] = m.lora_A.rho.detach()
            out[prefix + "lora_B"] = m.lora_B.detach()
    return out


def local_reparameterization(model: torch.nn.Module, enable: bool = True, kl: str = "sampled") -> int:
    """Switch every bnn.Linear of `model` to the local reparameterisation estimator (Kingma, Salimans, Welling 2015) or back:
    the layer samples its pre-activations, y = m + sqrt(v) * zeta with m = x mu^T + mu_b and v = x^2 (sigma^2)^T + sigma_b^2,
    instead of S weight tensors — noise per row rather than per sample, no sampled weights in memory, and ONE [2][N][K]
    weight-gradient contraction over all S*M rows (include/bayeformers_amd_lrt.h).  Opt-in: the default
    estimator and its bits are untouched, and `enable=False` restores them.  bnn.LoRALinear and bnn.Embedding are left alone.
    Returns the number of layers switched.

    kl="sampled" (default): log_prior / log_variational_posterior are those of the weight draws the default estimator makes
    for the same seed — the same bits, and set_kl_gradient(True) works unchanged.  kl="analytic": every sample's log-probs are
    the closed-form expectations E_q log p and E_q log q; Gaussian priors only (what to_bayesian(delta=...) makes), refused
    otherwise, and refused under set_kl_gradient(True) (no gradient of the closed form yet).

    Works under sample_bayesian, sample_predictive, GraphedSampler, training_step, GraphedTrainingStep, the reference's serial
    loop and Model.posterior_mean() (nothing is sampled there).  sample_generate and Model.pinned_samples(keep_weights=...)
    refuse a model with local layers: their contract is one weight draw per text."""
    from .nn.parameters.gaussian import Gaussian

    if kl not in ("sampled", "analytic"):
        raise ValueError(f"local_reparameterization: kl={kl!r} (\"sampled\" or \"analytic\")")
    layers = [m for m in model.modules() if isinstance(m, nn.Linear)]
    if enable and kl == "analytic":
        if bfr.STATE.kl_gradient:
            raise ValueError("local_reparameterization: kl=\"analytic\" has no KL gradient yet — it cannot be combined with "
                             "set_kl_gradient(True); use kl=\"sampled\"")
        for l in layers:
            priors = [l.weight_prior] + ([l.bias_prior] if isinstance(l.bias, Gaussian) else [])
            if not all(isinstance(p, Gaussian) for p in priors):
                raise ValueError("local_reparameterization: kl=\"analytic\" needs a Gaussian prior on every layer "
                                 "(to_bayesian(delta=...)); a layer has a mixture or user-defined prior")
    for l in layers:
        l.local, l.local_kl = bool(enable), (kl if enable else "sampled")
    for m in model.modules():
        if isinstance(m, Model):
            m._plan = None  # (the sampling plan holds exactly the layers that draw weights)
            cache = m.__dict__.get("_graphs")
            if cache is not None:
                cache.close()  # captured forwards replay the other estimator's launches
    return len(layers)


def enable_embedding(enable: bool = True) -> None:
    """Opt in to converting torch.nn.Embedding tables too (bnn.Embedding — an extension, the reference's TORCH2BAYE
    holds only nn.Linear).  Off by default so that `to_bayesian` converts exactly what the reference converts."""
    if enable:
        TORCH2BAYE[torch.nn.Embedding] = nn.Embedding
    else:
        TORCH2BAYE.pop(torch.nn.Embedding, None)


class _FusedIntoDense(torch.nn.Module):
    """Placeholder left where an activation was folded into the preceding Bayesian layer's GEMM epilogue."""

    def forward(self, x):
        return x


def _is_exact_gelu(fn) -> bool:
    if isinstance(fn, torch.nn.GELU):
        return fn.approximate == "none"
    if fn is torch.nn.functional.gelu:
        return True
    # transformers.activations.GELUActivation (ACT2FN["gelu"]): .act is torch.nn.functional.gelu
    return fn.__class__.__name__ == "GELUActivation" and getattr(fn, "act", None) is torch.nn.functional.gelu


def fuse_activations(model: torch.nn.Module) -> int:
    """Fold `dense -> exact GELU` pairs into the dense layer's GEMM epilogue (bf_gemm_nt_act).

    Recognises the HuggingFace pattern `module.dense` (a bnn.Linear) followed by `module.intermediate_act_fn`
    (BertIntermediate and its relatives).  Forward-only optimisation: whenever a gradient may be needed the layer
    falls back to a separate GELU so autograd stays intact.  Returns the number of fused pairs."""
    fused = 0
    for m in model.modules():
        dense = getattr(m, "dense", None)
        act = getattr(m, "intermediate_act_fn", None)
        if isinstance(dense, nn.Linear) and act is not None and _is_exact_gelu(act):
            dense.activation = "gelu"
            m.intermediate_act_fn = _FusedIntoDense().train(m.training)  # (a fresh module would be in training mode)
            fused += 1
    return fused


def _dense_residual_norm_forward(self, hidden_states, input_tensor):
    """forward of an HF `*Output` block — LayerNorm(dropout(dense(h)) + input) — with the residual add and the
    normalisation done by one HBM pass (bf_add_layernorm) behind the Bayesian dense layer's GEMM; with gradients
    enabled the same kernel runs inside an autograd function whose backward is bf_add_layernorm_bwd."""
    return _residual_norm(self, self.dense(hidden_states), input_tensor)


def _residual_norm(self, hidden_states, input_tensor):
    """The part of an HF `*Output` block behind its dense layer: LayerNorm(dropout(h) + input)."""
    from . import ops

    ln = self.LayerNorm
    dropping = self.dropout.training and self.dropout.p > 0  # (the dropout module's own mode, as its forward reads it)
    if not ops.layernorm_supported(hidden_states, input_tensor, ln):
        return ln((self.dropout(hidden_states) if dropping else hidden_states) + input_tensor)
    # training mode (/root/reference/examples/bert_glue.py:221): the hidden dropout runs INSIDE the kernel, its Philox mask
    # regenerated in the backward pass — no mask tensor, no extra pass over the dense output
    drop = ops.Dropout(self.dropout.p, bfr.STATE.seed, bfr.dropout_call(), bfr.dropout_site(self), bfr.dropout_origin(),
                       bfr.dropout_counter()) if dropping else None
    if torch.is_grad_enabled() and (hidden_states.requires_grad or input_tensor.requires_grad or ln.weight.requires_grad):
        if ops._NO_TWIN:
            return ops.AddLayerNormFn.apply(hidden_states, input_tensor, ln.weight, ln.bias, ln.eps, drop)
        # The output of such a block has two consumers in a transformer layer — the next dense layer and the next block's
        # residual connection.  The block hands out `y` with its second alias attached; the next block of this kind takes
        # the alias as its residual input, so the two gradients reach this block's backward separately and are added
        # inside its kernel (AddLayerNormFn, twin).  A consumer that does not know about the alias just uses `y`.
        residual = getattr(input_tensor, "_bf_twin", None)
        y, y2 = ops.AddLayerNormFn.apply(hidden_states, residual if residual is not None else input_tensor, ln.weight, ln.bias,
                                         ln.eps, drop, True)
        y._bf_twin = y2
        return y
    return ops.add_layernorm(hidden_states, input_tensor, ln.weight, ln.bias, ln.eps, drop)


def _layernorm_forward(self, input):
    """nn.LayerNorm.forward on bf_add_layernorm (no residual), differentiable through bf_add_layernorm_bwd."""
    from . import ops

    if input.shape[-1] != self.normalized_shape[0] or not ops.layernorm_supported(input, None, self):
        return torch.nn.functional.layer_norm(input, self.normalized_shape, self.weight, self.bias, self.eps)
    if torch.is_grad_enabled() and (input.requires_grad or self.weight.requires_grad):
        return ops.AddLayerNormFn.apply(input, None, self.weight, self.bias, self.eps)
    return ops.add_layernorm(input, None, self.weight, self.bias, self.eps)


def _ffn_pair_chunk(self, attention_output):
    """`feed_forward_chunk` of an HF transformer layer — output(intermediate(a), a) — with the two Bayesian dense layers and
    the GELU between them as ONE autograd node (nn.layers.linear._FFNPairFn) when a gradient is recorded and both layers were
    sampled by the model's cross-layer plan; anything else (inference, layers outside the plan, another activation) runs
    the module's own method."""
    from . import ops
    from .nn.layers.linear import _FFNPairFn
    from .nn.parameters.gaussian import Gaussian

    up, down = self.intermediate.dense, self.output.dense
    ctx = bfr.STATE.ctx
    a = attention_output
    plan = ctx.plan if ctx is not None else None
    usable = (plan is not None and torch.is_grad_enabled() and id(up) in plan.group_of and id(down) in plan.group_of
              and not up._small_m and not down._small_m and up.activation == "gelu" and down.activation is None
              and isinstance(self.intermediate.intermediate_act_fn, _FusedIntoDense)
              and up._shared_input is None and down._shared_input is None
              and isinstance(up.bias, Gaussian) and isinstance(down.bias, Gaussian)
              and a.is_cuda and a.dtype in (torch.bfloat16, torch.float16) and a.shape[-1] == up.in_features
              and up.out_features % 8 == 0 and (a.numel() // up.in_features) % ctx.S == 0
              and (a.numel() // up.in_features) // ctx.S > 128
              and (a.requires_grad or any(p.requires_grad for l in (up, down) for p in l.parameters())))
    if not usable:
        return self._bf_plain_ffn_chunk(attention_output)
    S, seed, base = ctx.S, bfr.STATE.seed, ctx.sample_base
    w1, b1 = plan.ensure(up, ctx.token, seed, base, ctx.lp_buf)
    w2, b2 = plan.ensure(down, ctx.token, seed, base, ctx.lp_buf)
    if w1.dtype != a.dtype or w2.dtype != a.dtype:
        return self._bf_plain_ffn_chunk(attention_output)
    x2 = a.reshape(-1, up.in_features)
    params = [t for l in (up, down) for t in (l.weight.mu, l.weight.rho, l.bias.mu, l.bias.rho)]
    y = _FFNPairFn.apply(x2 if x2.is_contiguous() else x2.contiguous(), up, down, S, seed, base, w1, b1, w2, b2, *params)
    for l in (up, down):  # what Linear.forward leaves behind: the log-probs of this forward are the plan's
        l._lp_view, l._lp_dirty = ctx.slot(l), True
    y = y.view(*a.shape[:-1], down.out_features)
    out = self.output
    if getattr(out.LayerNorm, "_bf_fused", False) and isinstance(out.forward, types.MethodType) and out.forward.__func__ is _dense_residual_norm_forward:
        return _residual_norm(out, y, a)
    return out.LayerNorm(out.dropout(y) + a)


def fuse_ffn_pairs(model: torch.nn.Module) -> int:
    """Make the feed-forward pair of every HuggingFace-style transformer layer (modules with `intermediate.dense` and
    `output.dense` as bnn.Linear children and a `feed_forward_chunk` method) ONE autograd node in training: the GELU's
    backward then rides in the epilogue of the down-projection's input-gradient GEMM (bf_gemm_nn_actgrad) instead of a pass
    of its own over the intermediate-sized gradient.  Call after `fuse_activations`.  Training-time rewrite; inference is
    untouched.  Returns the number of layers rewritten."""
    fused = 0
    for m in model.modules():
        inter, out = getattr(m, "intermediate", None), getattr(m, "output", None)
        if (inter is not None and out is not None and isinstance(getattr(inter, "dense", None), nn.Linear)
                and isinstance(getattr(out, "dense", None), nn.Linear) and hasattr(m, "feed_forward_chunk")
                and isinstance(getattr(out, "LayerNorm", None), torch.nn.LayerNorm) and hasattr(out, "dropout")
                and inter.dense.out_features == out.dense.in_features and not hasattr(m, "_bf_plain_ffn_chunk")):
            m._bf_plain_ffn_chunk = m.feed_forward_chunk
            m.feed_forward_chunk = types.MethodType(_ffn_pair_chunk, m)
            fused += 1
    return fused


def fuse_residual_layernorm(model: torch.nn.Module) -> int:
    """Fuse `LayerNorm(dropout(dense(h)) + input)` blocks whose dense layer is a bnn.Linear (HF BertSelfOutput,
    BertOutput and their relatives: attributes `dense`, `dropout`, `LayerNorm`, forward(hidden_states,
    input_tensor)) into dense GEMM -> one add+LayerNorm pass.  Inference-time optimisation, like fuse_activations.
    Returns the number of fused blocks."""
    fused = 0
    for m in model.modules():
        dense, ln, drop = getattr(m, "dense", None), getattr(m, "LayerNorm", None), getattr(m, "dropout", None)
        if (isinstance(dense, nn.Linear) and isinstance(ln, torch.nn.LayerNorm) and isinstance(drop, torch.nn.Dropout)
                and ln.elementwise_affine and ln.bias is not None and len(ln.normalized_shape) == 1
                and ln.normalized_shape[0] == dense.out_features and dense.out_features % 8 == 0
                and dense.out_features <= 4096 and m.__class__.__name__.endswith("Output")):
            m.forward = types.MethodType(_dense_residual_norm_forward, m)
            ln._bf_fused = True
            fused += 1
    # the remaining stand-alone LayerNorms (the embedding block's) run on the same kernel without a residual
    for m in model.modules():
        if (isinstance(m, torch.nn.LayerNorm) and not getattr(m, "_bf_fused", False) and m.elementwise_affine
                and m.bias is not None and len(m.normalized_shape) == 1 and m.normalized_shape[0] % 8 == 0
                and m.normalized_shape[0] <= 4096):
            m.forward = types.MethodType(_layernorm_forward, m)
            m._bf_fused = True
    return fused


def _embeddings_forward(self, input_ids=None, token_type_ids=None, position_ids=None, inputs_embeds=None,
                        past_key_values_length: int = 0):
    """forward of an HF `*Embeddings` block — LayerNorm(word[ids] + type[type_ids] + pos[pos_ids]) — as one pass
    (bf_embed_layernorm) when it is the plain inference case; anything else runs the module's own forward."""
    from . import ops

    w, t, p, ln = self.word_embeddings, self.token_type_embeddings, self.position_embeddings, self.LayerNorm
    dropping = self.dropout.training and self.dropout.p > 0
    plain = (input_ids is not None and inputs_embeds is None and input_ids.dim() == 2 and input_ids.is_cuda
             and input_ids.dtype == torch.long
             and not (torch.is_grad_enabled() and (w.weight.requires_grad or t.weight.requires_grad or
                                                   p.weight.requires_grad or ln.weight.requires_grad))
             and w.weight.dtype == t.weight.dtype == p.weight.dtype and w.weight.dtype in ops._TORCH2BF
             and ln.weight.dtype in (torch.float32, w.weight.dtype) and ln.bias is not None
             and ln.bias.dtype == ln.weight.dtype and w.weight.shape[1] % 8 == 0 and w.weight.shape[1] <= 4096
             and past_key_values_length + input_ids.shape[1] <= p.weight.shape[0]
             and (token_type_ids is None or token_type_ids.dtype == torch.long)
             and (position_ids is None or (position_ids.dtype == torch.long and position_ids.dim() == 2
                                           and position_ids.shape[1] == input_ids.shape[1]
                                           and position_ids.shape[0] in (1, input_ids.shape[0]))))
    if not plain:
        # training: the module's own forward — but on ONE copy of the batch when the ids are sample_bayesian's S-fold
        # repeat of it (the block is deterministic without dropout, every copy gets the same rows): the table gradients
        # are then scattered from B*T rows instead of S*B*T, after one sum over the copies
        rep = getattr(input_ids, "_bf_repeat", None) if input_ids is not None else None
        orig = rep[1]() if rep is not None else None  # (samples, weak reference to the tensor the ids repeat)
        if orig is not None and inputs_embeds is None:
            S = rep[0]
            B = orig.shape[0]

            def one_copy(t):  # a per-row companion of the ids: None, its own original, or rows that cannot differ
                if t is None or t.shape[0] == 1:
                    return t, True
                r = getattr(t, "_bf_repeat", None)
                src = r[1]() if r is not None else None
                if src is not None and r[0] == S and src.shape[0] == B:
                    return src, True
                if t.shape[0] == S * B and t.stride(0) == 0:
                    return t[:B], True
                return None, False

            tt, ok1 = one_copy(token_type_ids)
            pp, ok2 = one_copy(position_ids)
            if ok1 and ok2 and orig.dim() == 2 and orig.shape[0] * S == input_ids.shape[0]:
                # training mode: the block up to its LayerNorm is still the same for every copy — only the dropout that
                # ends it draws a mask per copy, so it moves behind the repeat
                saved = self.dropout
                if dropping:
                    self.dropout = torch.nn.Identity()
                try:
                    e = self._bf_plain_forward(input_ids=orig, token_type_ids=tt, position_ids=pp, inputs_embeds=None,
                                               past_key_values_length=past_key_values_length)
                finally:
                    self.dropout = saved
                e = e.repeat(S, *([1] * (e.dim() - 1)))
                return torch.nn.functional.dropout(e, saved.p, training=True) if dropping else e
        return self._bf_plain_forward(input_ids=input_ids, token_type_ids=token_type_ids, position_ids=position_ids,
                                      inputs_embeds=inputs_embeds, past_key_values_length=past_key_values_length)
    if position_ids is None and past_key_values_length:
        position_ids = self.position_ids[:, past_key_values_length:input_ids.shape[1] + past_key_values_length]
    e = ops.embed_layernorm(input_ids, token_type_ids, position_ids, w.weight, t.weight, p.weight, ln.weight, ln.bias,
                            ln.eps)
    return torch.nn.functional.dropout(e, self.dropout.p, training=True) if dropping else e


def fuse_embeddings(model: torch.nn.Module) -> int:
    """Run embedding blocks of the HuggingFace BERT family (modules holding `word_embeddings`,
    `token_type_embeddings`, `position_embeddings`, `LayerNorm`, `dropout`) as ONE launch: three table gathers, two
    full-size adds and the LayerNorm of their result become bf_embed_layernorm.  Inference-time rewrite like the other
    fuse_* functions: with dropout active, gradients needed or unusual arguments the module's own forward runs.
    Only blocks whose default positions are 0 .. L-1 (BERT, ELECTRA, ...) are rewritten; the RoBERTa family, which derives
    position ids from the padding mask, keeps its own forward.  Returns the number of blocks rewritten."""
    fused = 0
    for m in model.modules():
        parts = [getattr(m, n, None) for n in ("word_embeddings", "token_type_embeddings", "position_embeddings")]
        ln, drop = getattr(m, "LayerNorm", None), getattr(m, "dropout", None)
        if (all(isinstance(e, torch.nn.Embedding) for e in parts) and isinstance(ln, torch.nn.LayerNorm)
                and isinstance(drop, torch.nn.Dropout) and ln.elementwise_affine and ln.bias is not None
                and getattr(m, "position_embedding_type", "absolute") == "absolute"
                # RoBERTa-style blocks (XLM-R, CamemBERT, ...) number positions from padding_idx + 1 and skip padding
                # tokens (create_position_ids_from_input_ids): not the arange positions the kernel assumes — left alone
                and not hasattr(m, "padding_idx") and not hasattr(m, "create_position_ids_from_input_ids")
                and not hasattr(m, "_bf_plain_forward")):
            m._bf_plain_forward = m.forward
            m.forward = types.MethodType(_embeddings_forward, m)
            fused += 1
    return fused


def fuse_shared_inputs(model: torch.nn.Module, names=("query", "key", "value")) -> int:
    """Multiply the activations of an attention block by its query / key / value weights in ONE launch
    (bf_gemm_nt_layers): marks modules that hold `names` as bnn.Linear children of one shape (HF BertSelfAttention
    and its relatives, which call them on the same hidden states).  The sampling plan then lays their sampled
    weights out back to back, and whichever of the layers runs first computes all outputs; a layer that is handed a
    different input simply runs on its own.  With gradients enabled the launch sits in one autograd node whose backward
    computes ONE input gradient for the three layers (bf_gemm_nn_layers).  Returns the number of fused blocks."""
    fused = 0
    for m in model.modules():
        group = tuple(getattr(m, n, None) for n in names)
        if all(isinstance(l, nn.Linear) for l in group) and len({(l.in_features, l.out_features) for l in group}) == 1:
            for l in group:
                l._shared_input = group
            fused += 1
    if isinstance(model, Model):
        model.refresh()
    return fused


_POOLED_LAST_LAYER = [True]
_POOLED_ACTIVE = threading.local()  # .layers: ids of the last layers whose head said "narrow" for the call running on this thread


def pooled_last_layer(enable: bool = True) -> None:
    """Switch the narrow last encoder layer of pooled-head models (installed by `fuse_attention`) on or off for this
    process; BF_NO_POOLED_LAST_LAYER in the environment switches it off too.  Off: the layer runs on every row.  The switch
    is part of what a captured forward bakes in (graphs.baked_state): a forward replayed from a HIP graph is captured again
    at its next call after a flip."""
    _POOLED_LAST_LAYER[0] = bool(enable)


def pooled_last_layer_enabled() -> bool:
    return _POOLED_LAST_LAYER[0] and os.environ.get("BF_NO_POOLED_LAST_LAYER") is None


def _pooled_active(layer) -> bool:
    return id(layer) in getattr(_POOLED_ACTIVE, "layers", ())


def _hooked(module: torch.nn.Module) -> bool:
    """Does a hook watch `module`?  transformers' own output-capturing hooks do not count: it leaves them on the layers for
    good after the first call that asked for hidden states or attentions, and they do nothing in a call that asks for
    neither (such a call keeps the full path by its arguments).  They are told by the module their closure was defined in,
    `transformers.utils.output_capturing` — checked against transformers 5.15; should a release move it, the hooks count as
    anybody's and the full layer runs from the first call that asked for hidden states on: slower, never wrong."""
    fwd = [h for h in module._forward_hooks.values()
           if getattr(h, "__module__", None) != "transformers.utils.output_capturing"]
    return bool(fwd or module._forward_pre_hooks or module._backward_hooks or module._backward_pre_hooks)


def _pooled_head_forward(self, *args, **kwargs):
    """forward of a BertForSequenceClassification: decides, per call, whether the last encoder layer may compute the
    [CLS] rows alone (the head reads pooler(hidden[:, 0]) and nothing else of that layer), tells the layer, and runs the
    module's own forward.  Everything the narrow layer cannot honour keeps the full path: hidden states or attentions
    asked for (arguments or config), gradients recorded, training mode, a hook on the encoder, the pooler or any module of
    the last layer, a fusion that is not installed."""
    import torch.nn.modules.module as tmod

    bert = self.bert
    last = bert.encoder.layer[-1]
    cfg = self.config
    # (any module in training mode: nn.Dropout modules switched back on in an eval() model — Monte-Carlo dropout — drop inside
    # the full layer's kernels, which the narrow layer does not do)
    narrow = (pooled_last_layer_enabled()
              and not torch.is_grad_enabled() and not self.training and not bert.training
              and not any(m.training for m in last.modules()) and not any(m.training for m in bert.pooler.modules())
              and bert.pooler is not None
              and not kwargs.get("output_hidden_states") and not kwargs.get("output_attentions")
              and not getattr(cfg, "output_hidden_states", False) and not getattr(cfg, "output_attentions", False)
              and not getattr(cfg, "is_decoder", False) and not getattr(cfg, "add_cross_attention", False)
              and not (tmod._global_forward_hooks or tmod._global_forward_pre_hooks or tmod._global_backward_hooks
                       or tmod._global_backward_pre_hooks)
              and not _hooked(bert.encoder) and not _hooked(bert.encoder.layer)
              and not any(_hooked(m) for m in bert.pooler.modules()) and not any(_hooked(m) for m in last.modules())
              and _pooled_fusions_installed(last))
    if not narrow:
        return self._bf_plain_forward(*args, **kwargs)
    before = getattr(_POOLED_ACTIVE, "layers", frozenset())
    _POOLED_ACTIVE.layers = before | {id(last)}  # (per thread: two threads on one model do not see each other's verdict)
    try:
        return self._bf_plain_forward(*args, **kwargs)
    finally:
        _POOLED_ACTIVE.layers = before


def _pooled_fusions_installed(last) -> bool:
    """residual+LayerNorm, query/key/value and attention fusions on the last layer, and the GELU in the up-projection."""
    so, out, sa = last.attention.output, last.output, last.attention.self

    def ln_fused(m):
        f = m.__dict__.get("forward")
        return isinstance(f, types.MethodType) and f.__func__ is _dense_residual_norm_forward

    dense = (so.dense, last.intermediate.dense, out.dense)
    return (ln_fused(so) and ln_fused(out) and all(isinstance(l, nn.Linear) for l in dense)
            and all(l.activation is None for l in (so.dense, out.dense))
            and last.intermediate.dense.activation == "gelu"
            and isinstance(last.intermediate.intermediate_act_fn, _FusedIntoDense)
            and all(isinstance(getattr(sa, n, None), nn.Linear) and getattr(sa, n)._shared_input is not None
                    for n in ("query", "key", "value"))
            and getattr(sa.config, "_attn_implementation", None) == _ATTENTION_NAME
            and last.chunk_size_feed_forward == 0)


def _pooled_last_layer_forward(self, hidden_states, attention_mask=None, encoder_hidden_states=None,
                               encoder_attention_mask=None, past_key_values=None, **kwargs):
    """forward of the LAST BertLayer under a pooled head (`_pooled_head_forward` said so for this call): everything behind
    the key / value projections is computed for the [CLS] row of each sequence alone — one query row per (sequence, head)
    against all keys and values (bf_attention_fwd_rows), the three dense layers on B rows per sample (bf_gemm_nt_rows) on
    the weights the sampling plan drew anyway, the two residual+LayerNorm passes on those rows (bf_add_layernorm_rows reads
    the residual where it lies).  Returns [S*B, 1, hidden]: the pooler's hidden[:, 0] is that row.  Per row the arithmetic
    is the full layer's, except that the dense layers sum over k in the streaming kernel's order.  Whatever this form does
    not take — no sampling plan, another dtype, cached keys, an attention mask with per-query structure — runs the
    module's own forward on every row."""
    from . import ops

    def full():
        return self._bf_plain_layer_forward(hidden_states, attention_mask, encoder_hidden_states,
                                            encoder_attention_mask=encoder_attention_mask, past_key_values=past_key_values,
                                            **kwargs)

    if not _pooled_active(self):
        return full()
    ctx = bfr.STATE.ctx
    plan = ctx.plan if ctx is not None else None
    sa, so, up, down = self.attention.self, self.attention.output, self.intermediate.dense, self.output
    dense = (so.dense, up, down.dense)
    h = hidden_states
    if (plan is None or ctx.kept is not None or encoder_hidden_states is not None or past_key_values is not None
            or torch.is_grad_enabled() or any(m.training for m in self.modules()) or h.dim() != 3 or not h.is_cuda or not h.is_contiguous()
            or h.dtype not in (torch.bfloat16, torch.float16) or plan.cdt != h.dtype
            or h.shape[0] % ctx.S or any(id(l) not in plan.group_of or l._small_m for l in dense)
            or any(l.in_features % 32 or l.out_features % 8 for l in dense)
            # a layer so small that the full layer runs the single small-M kernel outside the sampling plan keeps doing so
            # (the plan holds exactly the layers it would hold without this rewrite)
            or any(h.shape[0] * h.shape[1] // ctx.S <= ops.fused_small_rows(l.out_features, l.in_features) for l in dense)
            or not ops.layernorm_supported(h[:, :1], None, so.LayerNorm)
            or not ops.layernorm_supported(h[:, :1], None, down.LayerNorm)):
        return full()
    Bt, T, Hd = h.shape
    S = ctx.S
    M = Bt // S
    H, D = sa.num_attention_heads, sa.attention_head_size
    q = sa.query(h).view(Bt, T, H, D).transpose(1, 2)  # (one stacked launch serves the three)
    k = sa.key(h).view(Bt, T, H, D).transpose(1, 2)
    v = sa.value(h).view(Bt, T, H, D).transpose(1, 2)
    key_mask = mask_off = None
    rows_attention = ops.attention_supported(q, k, v)
    rows_any = not rows_attention and encoder_ragged_attention_enabled() and ops.attention_any_supported(q, k, v)
    rows_attention = rows_attention or rows_any
    if rows_attention and attention_mask is not None:
        marks = _marks_of(attention_mask)
        if marks.key_mask is not None and marks.key_mask.shape == (Bt, T):
            key_mask, mask_off = marks.key_mask, marks.mask_off
        else:
            rows_attention = False
    if rows_attention:
        rows_fn = ops.attention_forward_rows_any if rows_any else ops.attention_forward_rows
        a = rows_fn(q, k, v, key_mask, sa.scaling, mask_off, q_rows=1).view(Bt, Hd)
        a_row_stride = Hd
    else:
        # the attention this length or mask needs, on every query; its [CLS] rows are read where they lie
        from transformers.modeling_utils import ALL_ATTENTION_FUNCTIONS

        fn = ALL_ATTENTION_FUNCTIONS.get_interface(sa.config._attn_implementation, None)
        a, _ = fn(sa, q, k, v, attention_mask, dropout=0.0, scaling=sa.scaling, **kwargs)
        a = a.reshape(Bt, T, Hd)
        a = a if a.is_contiguous() else a.contiguous()
        a_row_stride = T * Hd

    def rows_linear(layer, x, row_stride, act=0):
        w_s, b_s = plan.ensure(layer, ctx.token, bfr.STATE.seed, ctx.sample_base, ctx.lp_buf)
        y = ops.gemm_nt_rows(x, w_s, b_s, S, M, layer.out_features, layer.in_features, M * row_stride, row_stride, act)
        layer._lp_view, layer._lp_dirty = ctx.slot(layer), True
        return y

    ln1, ln2 = so.LayerNorm, down.LayerNorm
    y = rows_linear(so.dense, a, a_row_stride)
    y = ops.add_layernorm_rows(y, h, T * Hd, ln1.weight, ln1.bias, ln1.eps)  # residual: the [CLS] rows of the layer's input
    z = rows_linear(up, y, Hd, 1)
    z = rows_linear(down.dense, z, up.out_features)
    z = ops.add_layernorm(z, y, ln2.weight, ln2.bias, ln2.eps)
    return z.view(Bt, 1, Hd)


def _install_pooled_last_layer(inner: torch.nn.Module) -> bool:
    """A BertForSequenceClassification (BertModel with a pooler under a head that reads pooler_output alone): its forward and
    its last encoder layer's get the per-call narrow path.  Any other model is left as it is."""
    for head in inner.modules():
        bert = getattr(head, "bert", None)
        if (type(head).__name__ != "BertForSequenceClassification" or type(bert).__name__ != "BertModel"
                or getattr(bert, "pooler", None) is None or hasattr(head, "_bf_plain_forward")):
            continue
        layers = getattr(getattr(bert, "encoder", None), "layer", None)
        if not layers or type(layers[-1]).__name__ != "BertLayer":
            continue
        last = layers[-1]
        last._bf_plain_layer_forward = last.forward
        last.forward = types.MethodType(_pooled_last_layer_forward, last)
        head._bf_plain_forward = head.forward
        head.forward = types.MethodType(_pooled_head_forward, head)
        return True
    return False


_DECODER_LAYERS = {"LlamaDecoderLayer": "LlamaAttention", "MistralDecoderLayer": "MistralAttention",
                   "Qwen2DecoderLayer": "Qwen2Attention"}


def _records_grad(x, *modules) -> bool:
    """Would autograd record an op on x under these modules' parameters?"""
    return torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for m in modules for p in m.parameters()))


def _is_rmsnorm(m) -> bool:
    return (isinstance(m, torch.nn.Module) and type(m).__name__.endswith("RMSNorm")
            and isinstance(getattr(m, "weight", None), torch.Tensor) and m.weight.dim() == 1
            and isinstance(getattr(m, "variance_epsilon", None), (int, float)))


def _is_silu(fn) -> bool:
    return isinstance(fn, torch.nn.SiLU) or type(fn).__name__ == "SiLUActivation"


def _blocks_backward(module) -> bool:
    """Did fuse_decoder_blocks(backward=True) rewrite this module?  Then its fast form also runs under recorded gradients
    and in training mode, through the autograd functions over the backward kernels."""
    return getattr(module, "_bf_blocks_backward", False)


def _norm_eps(norm) -> float:
    return norm.eps if hasattr(norm, "eps") else norm.variance_epsilon


def _add_norm(gemma: bool, rec: bool, x, residual, norm, want_sum: bool = True):
    """(x + residual, its norm under `norm`) by bf_norm_add_rmsnorm with Gemma's (1 + weight) convention, or by
    bf_add_rmsnorm; rec: through the autograd function over both directions (which returns the norm alone without a
    residual, and always writes the sum)."""
    from . import ops

    if gemma:
        if rec:
            return ops.NormAddRMSNormFn.apply(x, None, residual, norm.weight, 0.0, _norm_eps(norm), 1)
        return ops.norm_add_rmsnorm(x, None, residual, norm.weight, 0.0, _norm_eps(norm), 1, want_sum=want_sum)
    if rec:
        return ops.AddRMSNormFn.apply(x, residual, norm.weight, _norm_eps(norm))
    return ops.add_rmsnorm(x, residual, norm.weight, _norm_eps(norm), want_sum=want_sum)


def _norm_module_forward(self, hidden_states, gemma: bool):
    """forward of an HF `*RMSNorm` on bf_add_rmsnorm, or (gemma) of a Gemma*RMSNorm on bf_norm_add_rmsnorm without a first
    norm or residual, offset 1.  A hidden state that the fused layer in front of this norm produced
    carries this norm's output already (`_bf_normed`, computed in that layer's residual pass): it is handed out as it is.
    Under recorded gradients the module's own forward runs unless the norm was rewritten with the backward on; then the
    attached tensor is the second output of the autograd
    function whose first output is the hidden state; it is taken only when it carries a grad_fn — whatever this forward
    returns under recorded gradients must be part of the graph, and reentrant checkpointing or layers run under no_grad
    hand out graph-less ones — and it stays attached, so a recomputation of this forward sees what the first run saw."""
    from . import ops

    x = hidden_states
    rec = isinstance(x, torch.Tensor) and _records_grad(x, self)
    if (not isinstance(x, torch.Tensor) or (rec and not _blocks_backward(self)) or not ops.rmsnorm_supported(x, None, self)):
        return self._bf_plain_rmsnorm_forward(hidden_states)
    ready = x.__dict__.get("_bf_normed") if rec else x.__dict__.pop("_bf_normed", None)
    if ready is not None and ready[1] is self and not (rec and ready[0].grad_fn is None):
        return ready[0]
    return _add_norm(gemma, True, x, None, self) if rec else _add_norm(gemma, False, x, None, self, want_sum=False)[1]


def _rmsnorm_forward(self, hidden_states):
    """_norm_module_forward for Llama's convention: counts in ops.BLOCK_CALLS["rmsnorm"], backward through ops.AddRMSNormFn."""
    return _norm_module_forward(self, hidden_states, False)


def _gemma_rmsnorm_forward(self, hidden_states):
    """_norm_module_forward for Gemma's (1 + weight) convention, backward through ops.NormAddRMSNormFn."""
    return _norm_module_forward(self, hidden_states, True)


def _two_norm_layer_forward(self, gemma, hidden_states, attention_mask=None, position_ids=None, past_key_values=None,
                            use_cache=False, position_embeddings=None, **kwargs):
    """forward of an HF Llama / Mistral / Qwen2 / Qwen3 decoder layer or (gemma) of a GemmaDecoderLayer with its two residual
    adds folded into the RMSNorm that follows each (bf_add_rmsnorm, or bf_norm_add_rmsnorm with the (1 + weight)
    convention, writes the sum and the normalised row in one pass): the second add feeds the NEXT
    layer's input norm (or the model's final norm), whose output travels on the returned hidden state as `_bf_normed`.
    The returned tensor is always the true hidden state.  Tensors off the device, a hook on the norm whose forward is
    skipped: the module's own forward; gradients recorded or training mode as well, unless the layer was rewritten with
    the backward on — then the two passes run through ops.AddRMSNormFn / ops.NormAddRMSNormFn, whose backward is
    bf_add_rmsnorm_bwd / bf_norm_add_rmsnorm_bwd."""
    from . import ops

    h = hidden_states
    post, nxt = self.post_attention_layernorm, self._bf_next_norm[0]
    rec = isinstance(h, torch.Tensor) and _records_grad(h, self, nxt)
    if (not isinstance(h, torch.Tensor) or _hooked(post) or not ops.rmsnorm_supported(h, None, post)
            or not ops.rmsnorm_supported(h, None, nxt) or ((self.training or rec) and not _blocks_backward(self))):
        return self._bf_plain_layer_forward(hidden_states, attention_mask=attention_mask, position_ids=position_ids,
                                            past_key_values=past_key_values, use_cache=use_cache,
                                            position_embeddings=position_embeddings, **kwargs)
    a, _ = self.self_attn(hidden_states=self.input_layernorm(h), attention_mask=attention_mask, position_ids=position_ids,
                          past_key_values=past_key_values, use_cache=use_cache, position_embeddings=position_embeddings,
                          **kwargs)
    if ops.rmsnorm_supported(a, h, post):
        h1, y1 = _add_norm(gemma, rec, a, h, post)
    else:
        h1 = h + a
        y1 = post(h1)
    m = self.mlp(y1)
    if not ops.rmsnorm_supported(m, h1, nxt):
        return h1 + m
    h2, y2 = _add_norm(gemma, rec, m, h1, nxt)
    h2._bf_normed = (y2, nxt)
    return h2


def _decoder_layer_forward(self, hidden_states, attention_mask=None, position_ids=None, past_key_values=None,
                           use_cache=False, position_embeddings=None, **kwargs):
    """_two_norm_layer_forward on bf_add_rmsnorm (Llama, Mistral, Qwen2, Qwen3)."""
    return _two_norm_layer_forward(self, False, hidden_states, attention_mask, position_ids, past_key_values, use_cache,
                                   position_embeddings, **kwargs)


def _gemma_layer_forward(self, hidden_states, attention_mask=None, position_ids=None, past_key_values=None,
                         use_cache=False, position_embeddings=None, **kwargs):
    """_two_norm_layer_forward on bf_norm_add_rmsnorm with the (1 + weight) convention (Gemma 1)."""
    return _two_norm_layer_forward(self, True, hidden_states, attention_mask, position_ids, past_key_values, use_cache,
                                   position_embeddings, **kwargs)


def _decoder_attention_forward(self, hidden_states, position_embeddings=None, attention_mask=None, past_key_values=None,
                               **kwargs):
    """forward of an HF Llama / Mistral / Qwen2 attention module with apply_rotary_pos_emb as one launch (bf_rope_qk), in
    place on the projections' outputs in the [B, T, heads * head_dim] layout the attention kernels read through strides.
    The cache update, the attention interface lookup and o_proj are the module's own code path.  Rewritten with
    backward=True it also runs under recorded gradients and in training mode (unless attention dropout would be active):
    out of place through ops.RopeQKFn, whose outputs have the same [B, T, heads, head_dim] layout."""
    import sys

    from . import ops

    x = hidden_states
    pe = position_embeddings
    rec = isinstance(x, torch.Tensor) and _records_grad(x, self)
    fast = (pe is not None and isinstance(x, torch.Tensor) and x.is_cuda and x.dim() == 3 and x.dtype in ops._TORCH2BF
            and self.head_dim in (64, 128) and (_blocks_backward(self) or not (self.training or rec))
            and not (self.training and self.attention_dropout > 0))
    if fast:
        cos, sin = pe
        fast = (cos.dim() == 3 and sin.shape == cos.shape and cos.shape[-1] == self.head_dim and cos.shape[1] == x.shape[1]
                and cos.shape[0] in (1, x.shape[0]))
    if not fast:
        return self._bf_plain_attn_forward(hidden_states, position_embeddings=position_embeddings,
                                           attention_mask=attention_mask, past_key_values=past_key_values, **kwargs)
    mod = sys.modules[type(self).__module__]
    input_shape = x.shape[:-1]
    hidden_shape = (*input_shape, -1, self.head_dim)
    query_states = self.q_proj(x).view(hidden_shape).transpose(1, 2)
    key_states = self.k_proj(x).view(hidden_shape).transpose(1, 2)
    value_states = self.v_proj(x).view(hidden_shape).transpose(1, 2)
    cos, sin = (t if t.is_contiguous() else t.contiguous() for t in (cos, sin))
    if ops.rope_supported(query_states, key_states, cos, sin):
        if rec:  # the in-place form would overwrite what the projections' backward reads
            query_states, key_states = ops.RopeQKFn.apply(query_states, key_states, cos, sin)
        else:
            query_states, key_states = ops.rope_qk(query_states, key_states, cos, sin, inplace=True)
    else:  # a projection that came back in another dtype or layout: the framework's ops on what is already computed
        query_states, key_states = mod.apply_rotary_pos_emb(query_states, key_states, cos, sin)
    if past_key_values is not None:
        key_states, value_states = past_key_values.update(key_states, value_states, self.layer_idx)
    attention_interface = mod.ALL_ATTENTION_FUNCTIONS.get_interface(self.config._attn_implementation,
                                                                    mod.eager_attention_forward)
    name = type(self).__name__  # (the one difference between the three classes' forwards)
    if name == "MistralAttention":
        kwargs = dict(kwargs, sliding_window=getattr(self.config, "sliding_window", None))
    elif name == "Qwen2Attention":
        kwargs = dict(kwargs, sliding_window=self.sliding_window)
    attn_output, attn_weights = attention_interface(self, query_states, key_states, value_states, attention_mask,
                                                    dropout=0.0 if not self.training else self.attention_dropout,
                                                    scaling=self.scaling, **kwargs)
    attn_output = attn_output.reshape(*input_shape, -1).contiguous()
    return self.o_proj(attn_output), attn_weights


def _glu_mlp_forward(self, x, gemma: bool):
    """forward of an HF Llama- or (gemma) Gemma-style MLP — down_proj(act_fn(gate_proj(x)) * up_proj(x)) — with the SiLU or
    tanh-GELU and the product as one launch (bf_swiglu / bf_geglu); rewritten with the backward on, under recorded gradients
    and in training mode too, through ops.SwiGLUFn / ops.GeGLUFn."""
    from . import ops

    rec = isinstance(x, torch.Tensor) and _records_grad(x, self)
    if (not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype not in ops._TORCH2BF or _hooked(self.act_fn)
            or ((self.training or rec) and not _blocks_backward(self))):
        return self._bf_plain_mlp_forward(x)
    gate, up = self.gate_proj(x), self.up_proj(x)
    if not ops.swiglu_supported(gate, up):
        return self.down_proj(self.act_fn(gate) * up)
    if gemma:
        return self.down_proj(ops.GeGLUFn.apply(gate, up) if rec else ops.geglu(gate, up))
    return self.down_proj(ops.SwiGLUFn.apply(gate, up) if rec else ops.swiglu(gate, up))


def _swiglu_mlp_forward(self, x):
    """_glu_mlp_forward on bf_swiglu / ops.SwiGLUFn (Llama, Mistral, Qwen2, Qwen3)."""
    return _glu_mlp_forward(self, x, False)


def _geglu_mlp_forward(self, x):
    """_glu_mlp_forward on bf_geglu / ops.GeGLUFn (Gemma 1 / 2 / 3)."""
    return _glu_mlp_forward(self, x, True)


# ---- the Gemma 1 / 2 / 3 and Qwen3 families (fuse_decoder_blocks(families=...)): inference-time forwards, and with
# backward="all" the training-time ones through ops.NormAddRMSNormFn / QKNormRopeFn / GeGLUFn
# family -> (decoder layer class, attention class, weight offset of its norms, has q / k norms, sandwich of four norms)
_FAMILY_LAYERS = {"qwen3": ("Qwen3DecoderLayer", "Qwen3Attention", 0, True, False),
                  "gemma": ("GemmaDecoderLayer", "GemmaAttention", 1, False, False),
                  "gemma2": ("Gemma2DecoderLayer", "Gemma2Attention", 1, False, True),
                  "gemma3": ("Gemma3DecoderLayer", "Gemma3Attention", 1, True, True)}
_DEFAULT_FAMILIES = ("llama", "mistral", "qwen2")
_CLASSIC_FAMILIES = {"llama": "LlamaDecoderLayer", "mistral": "MistralDecoderLayer", "qwen2": "Qwen2DecoderLayer"}


def _is_gemma_rmsnorm(m) -> bool:
    """An HF Gemma*RMSNorm: `weight` [N] and `eps`, y = x rsqrt(mean(x^2) + eps) (1 + weight) rounded once."""
    return (isinstance(m, torch.nn.Module) and type(m).__name__.endswith("RMSNorm") and type(m).__name__.startswith("Gemma")
            and isinstance(getattr(m, "weight", None), torch.Tensor) and m.weight.dim() == 1
            and isinstance(getattr(m, "eps", None), (int, float)) and not hasattr(m, "variance_epsilon"))


def _is_gelu_tanh(fn) -> bool:
    if isinstance(fn, torch.nn.GELU):
        return fn.approximate == "tanh"
    return type(fn).__name__ in ("GELUTanh", "PytorchGELUTanh")


def _sandwich_layer_forward(self, hidden_states, position_embeddings=None, attention_mask=None, position_ids=None,
                            past_key_values=None, **kwargs):
    """forward of an HF Gemma2DecoderLayer / Gemma3DecoderLayer, whose four norms sandwich the two residual adds:
        (h1, y1) = K(attn_out, post_attention_layernorm, h, pre_feedforward_layernorm)
        (h2, y2) = K(mlp_out, post_feedforward_layernorm, h1, the next layer's input_layernorm or the final norm)
    with K = bf_norm_add_rmsnorm: norm, add, norm in one launch each, so a layer makes four launches with its rotary and
    GeGLU ones.  y2 travels on the returned hidden state as `_bf_normed`; the returned tensor is always the true hidden
    state.  Tensors off the device or a hook on one of the three norms whose forward is skipped send the layer to its own
    forward; gradients recorded or training mode as well, unless the layer was rewritten with backward="all" — then K is
    ops.NormAddRMSNormFn, whose backward is one bf_norm_add_rmsnorm_bwd for both norms and the add."""
    from . import ops

    h = hidden_states
    post, pre_ff, post_ff = self.post_attention_layernorm, self.pre_feedforward_layernorm, self.post_feedforward_layernorm
    nxt = self._bf_next_norm[0]
    rec = isinstance(h, torch.Tensor) and _records_grad(h, self, nxt)
    if (not isinstance(h, torch.Tensor) or ((self.training or rec) and not _blocks_backward(self))
            or _hooked(post) or _hooked(pre_ff) or _hooked(post_ff)
            or not ops.norm_add_rmsnorm_supported(h, post, h, pre_ff)
            or not ops.norm_add_rmsnorm_supported(h, post_ff, h, nxt)):
        return self._bf_plain_layer_forward(hidden_states, position_embeddings=position_embeddings,
                                            attention_mask=attention_mask, position_ids=position_ids,
                                            past_key_values=past_key_values, **kwargs)
    a, _ = self.self_attn(hidden_states=self.input_layernorm(h), position_embeddings=position_embeddings,
                          attention_mask=attention_mask, position_ids=position_ids, past_key_values=past_key_values,
                          **kwargs)
    norm_add_rmsnorm = ops.NormAddRMSNormFn.apply if rec else ops.norm_add_rmsnorm
    if ops.norm_add_rmsnorm_supported(a, post, h, pre_ff):
        h1, y1 = norm_add_rmsnorm(a, post.weight, h, pre_ff.weight, post.eps, pre_ff.eps, 1)
    else:  # an attention output in another dtype: the framework's ops on what is already computed
        h1 = h + post(a)
        y1 = pre_ff(h1)
    m = self.mlp(y1)
    if not ops.norm_add_rmsnorm_supported(m, post_ff, h1, nxt):
        return h1 + post_ff(m)
    h2, y2 = norm_add_rmsnorm(m, post_ff.weight, h1, nxt.weight, post_ff.eps, nxt.eps, 1)
    h2._bf_normed = (y2, nxt)
    return h2


def _family_attention_forward(self, hidden_states, position_embeddings=None, attention_mask=None, past_key_values=None,
                              **kwargs):
    """forward of an HF Qwen3 / Gemma / Gemma2 / Gemma3 attention module with the per-head q_norm / k_norm (Qwen3, Gemma 3)
    and apply_rotary_pos_emb as one launch (bf_qknorm_rope: head size 64, 128 or 256), in place on the projections' outputs
    in the [B, T, heads * head_dim] layout the attention kernels read through strides.  The cache update, the attention
    interface lookup and o_proj are the module's own code path, and the interface gets exactly the keyword arguments that
    class's own forward passes.  Tensors off the device or a hook on q_norm / k_norm send the module to its own forward;
    gradients recorded or training mode as well, unless it was rewritten with backward="all": then it runs out of place
    through ops.QKNormRopeFn (unless attention dropout would be active), whose outputs have the same layout."""
    import sys

    from . import ops

    x = hidden_states
    pe = position_embeddings
    name = type(self).__name__
    offset, has_qk = self._bf_family[0], self._bf_family[1]
    qn, kn = (self.q_norm, self.k_norm) if has_qk else (None, None)
    rec = isinstance(x, torch.Tensor) and _records_grad(x, self)
    fast = (pe is not None and isinstance(x, torch.Tensor) and x.is_cuda and x.dim() == 3 and x.dtype in ops._TORCH2BF
            and self.head_dim in (64, 128, 256) and (_blocks_backward(self) or not (self.training or rec))
            and not (self.training and self.attention_dropout > 0)
            and not (has_qk and (_hooked(qn) or _hooked(kn))))
    if fast:
        cos, sin = pe
        fast = (cos.dim() == 3 and sin.shape == cos.shape and cos.shape[-1] == self.head_dim and cos.shape[1] == x.shape[1]
                and cos.shape[0] in (1, x.shape[0]))
    if not fast:
        return self._bf_plain_attn_forward(hidden_states, position_embeddings=position_embeddings,
                                           attention_mask=attention_mask, past_key_values=past_key_values, **kwargs)
    mod = sys.modules[type(self).__module__]
    input_shape = x.shape[:-1]
    hidden_shape = (*input_shape, -1, self.head_dim)
    query_states = self.q_proj(x).view(hidden_shape).transpose(1, 2)
    key_states = self.k_proj(x).view(hidden_shape).transpose(1, 2)
    value_states = self.v_proj(x).view(hidden_shape).transpose(1, 2)
    cos, sin = (t if t.is_contiguous() else t.contiguous() for t in (cos, sin))
    gq, gk = (qn.weight, kn.weight) if has_qk else (None, None)
    if ops.qknorm_rope_supported(query_states, key_states, cos, sin, gq, gk):
        eps = _norm_eps(qn) if has_qk else 0.0
        if rec:  # the in-place form would overwrite what the projections' backward reads
            query_states, key_states = ops.QKNormRopeFn.apply(query_states, key_states, cos, sin, gq, gk, eps, offset)
        else:
            query_states, key_states = ops.qknorm_rope(query_states, key_states, cos, sin, gq, gk, eps=eps,
                                                       weight_offset=offset, inplace=True)
    else:  # a projection that came back in another dtype or layout: the framework's ops on what is already computed
        if has_qk:
            query_states, key_states = qn(query_states), kn(key_states)
        query_states, key_states = mod.apply_rotary_pos_emb(query_states, key_states, cos, sin)
    if past_key_values is not None:
        key_states, value_states = past_key_values.update(key_states, value_states, self.layer_idx)
    attention_interface = mod.ALL_ATTENTION_FUNCTIONS.get_interface(self.config._attn_implementation,
                                                                    mod.eager_attention_forward)
    # what each class's own forward hands the interface (transformers' modeling_qwen3 / gemma / gemma2 / gemma3)
    if name == "Gemma2Attention":
        kwargs = dict(sliding_window=self.sliding_window, softcap=self.attn_logit_softcapping, **kwargs)
    elif name in ("Gemma3Attention", "Qwen3Attention"):
        kwargs = dict(sliding_window=self.sliding_window, **kwargs)
    attn_output, attn_weights = attention_interface(self, query_states, key_states, value_states, attention_mask,
                                                    dropout=self.attention_dropout if self.training else 0.0,
                                                    scaling=self.scaling, **kwargs)
    attn_output = attn_output.reshape(*input_shape, -1).contiguous()
    return self.o_proj(attn_output), attn_weights


def _fuse_family_layer(layer, nxt, family) -> bool:
    """Rewrite one layer of a family of _FAMILY_LAYERS; False (and nothing changed) when it lacks the attribute shape."""
    layer_cls, attn_cls, offset, has_qk, sandwich = _FAMILY_LAYERS[family]
    attn, mlp = getattr(layer, "self_attn", None), getattr(layer, "mlp", None)
    is_norm = _is_gemma_rmsnorm if offset else _is_rmsnorm
    norms = ["input_layernorm", "post_attention_layernorm"] + (["pre_feedforward_layernorm", "post_feedforward_layernorm"]
                                                               if sandwich else [])
    act = getattr(mlp, "act_fn", None)
    if (type(attn).__name__ != attn_cls or not all(is_norm(getattr(layer, n, None)) for n in norms) or not is_norm(nxt)
            or not all(isinstance(getattr(mlp, n, None), torch.nn.Module) for n in ("gate_proj", "up_proj", "down_proj"))
            or not (_is_gelu_tanh(act) if offset else _is_silu(act))
            or not all(isinstance(getattr(attn, n, None), torch.nn.Module) for n in ("q_proj", "k_proj", "v_proj", "o_proj"))
            or getattr(attn, "head_dim", None) not in (64, 128, 256)
            or (has_qk and not (is_norm(getattr(attn, "q_norm", None)) and is_norm(getattr(attn, "k_norm", None))))):
        return False
    layer._bf_next_norm = (nxt,)  # (in a tuple: not a child module of this layer)
    layer._bf_plain_layer_forward = layer.forward
    layer.forward = types.MethodType(_sandwich_layer_forward if sandwich else _gemma_layer_forward if offset
                                     else _decoder_layer_forward, layer)
    attn._bf_family = (offset, has_qk)
    attn._bf_plain_attn_forward = attn.forward
    attn.forward = types.MethodType(_family_attention_forward, attn)
    mlp._bf_plain_mlp_forward = mlp.forward
    mlp.forward = types.MethodType(_geglu_mlp_forward if offset else _swiglu_mlp_forward, mlp)
    for norm in (layer.input_layernorm, nxt):
        if not hasattr(norm, "_bf_plain_rmsnorm_forward"):
            norm._bf_plain_rmsnorm_forward = norm.forward
            norm.forward = types.MethodType(_gemma_rmsnorm_forward if offset else _rmsnorm_forward, norm)
    return True


def fuse_decoder_blocks(model: torch.nn.Module, backward: Union[bool, str] = False, families=_DEFAULT_FAMILIES) -> int:
    """Run the memory-bound ops of HuggingFace Llama, Mistral and Qwen2 decoder layers — the two RMSNorms with the
    residual adds in front of them, the rotary embedding of q and k, SiLU(gate) * up — as four launches per layer
    (bf_add_rmsnorm twice, bf_rope_qk, bf_swiglu) instead of the framework's thirty or so elementwise kernels.  A layer is
    rewritten when its class is exactly LlamaDecoderLayer, MistralDecoderLayer or Qwen2DecoderLayer with the attribute
    shape those have (RMSNorm modules with `weight` and `variance_epsilon`, an MLP of gate / up / down projections around
    a SiLU, an attention module with q / k / v / o projections and head_dim 64 or 128); with the default `families`, Qwen3
    (q / k norms), Gemma (1 + weight), OLMo and mixture-of-experts decoder layers keep their own norms, RoPE and glue (the
    experts of such a layer are converted by to_bayesian(experts=True) and run on the bf_moe_* kernels).  By default an inference-time
    rewrite like the other fuse_* functions: with gradients recorded, in training mode, off the device or on shapes the
    kernels refuse, the modules' own forwards run.  backward=True: the fast forms also run under recorded gradients and in
    training mode, through autograd functions whose backward is one launch each (bf_add_rmsnorm_bwd, bf_rope_qk_bwd,
    bf_swiglu_bwd) — a training step's decoder glue on the kernels in both directions; an attention module whose dropout
    would be active still runs its own forward.

    families: the model families whose layers are rewritten, a name or an iterable of names out of "llama", "mistral",
    "qwen2" (the default three), "qwen3", "gemma", "gemma2", "gemma3" (Gemma3 text decoder layers), or "all".  The four
    further families are opt-in and matched by exact class name as well:
      qwen3   the layer and the MLP as above (bf_add_rmsnorm, bf_swiglu); the attention module's q_norm, k_norm and
              rotary embedding are one launch (bf_qknorm_rope).
      gemma   Llama's structure with the (1 + weight) norms (bf_norm_add_rmsnorm), the rotary embedding at head size
              256 (bf_qknorm_rope without gammas) and gelu_tanh(gate) * up (bf_geglu).
      gemma2, gemma3   the four norms around the two residual adds as two norm -> add -> norm launches
              (bf_norm_add_rmsnorm), bf_qknorm_rope (with Gemma 3's q_norm / k_norm), bf_geglu: four launches a layer.
              A Gemma whose activation is not the tanh GELU is declined.
    For these four backward=True sets no backward flag: under recorded gradients or in training mode the modules' own
    forwards run.  backward="all" turns the backward on for them as well as for the default three: the fast forms then run
    under recorded gradients and in training mode through autograd functions whose backward is bf_norm_add_rmsnorm_bwd (one
    launch for a norm -> add -> norm, and a small one for the two weights' gradients), bf_qknorm_rope_bwd and bf_geglu_bwd
    (Qwen3's layer and MLP: bf_add_rmsnorm_bwd, bf_swiglu_bwd).  A hook on a module whose forward a fast form skips (the
    three further norms, q_norm, k_norm, act_fn) sends that module, or its layer, to its own forward.

    Returns the number of layers rewritten; calling it again rewrites nothing twice (a second call with backward=True
    turns the backward on for the Llama / Mistral / Qwen2 layers already rewritten, one with backward="all" for the layers
    of every family, and counts none of them).  Any other value of `backward` that is no bool is a ValueError."""
    if not isinstance(backward, bool) and backward != "all":
        raise ValueError(f"fuse_decoder_blocks: backward={backward!r} must be False, True or 'all'")
    names = (families,) if isinstance(families, str) else tuple(families)
    if "all" in names:
        names = tuple(_CLASSIC_FAMILIES) + tuple(_FAMILY_LAYERS)
    unknown = [n for n in names if n not in _CLASSIC_FAMILIES and n not in _FAMILY_LAYERS]
    if unknown:
        raise ValueError(f"fuse_decoder_blocks: unknown families {unknown}; known: "
                         f"{sorted(_CLASSIC_FAMILIES) + sorted(_FAMILY_LAYERS)} and 'all'")
    classic = {_CLASSIC_FAMILIES[n] for n in names if n in _CLASSIC_FAMILIES}
    further = {_FAMILY_LAYERS[n][0]: n for n in names if n in _FAMILY_LAYERS}
    fused = 0
    for parent in model.modules():
        layers, final = getattr(parent, "layers", None), getattr(parent, "norm", None)
        if not isinstance(layers, torch.nn.ModuleList) or not (_is_rmsnorm(final) or _is_gemma_rmsnorm(final)):
            continue
        for i, layer in enumerate(layers):
            attn, mlp = getattr(layer, "self_attn", None), getattr(layer, "mlp", None)
            nxt = getattr(layers[i + 1], "input_layernorm", None) if i + 1 < len(layers) else final
            cls = type(layer).__name__
            if cls in further:
                if not hasattr(layer, "_bf_plain_layer_forward") and _fuse_family_layer(layer, nxt, further[cls]):
                    fused += 1
                if backward == "all" and hasattr(layer, "_bf_plain_layer_forward"):
                    for m in (layer, attn, mlp, layer.input_layernorm, nxt):
                        m._bf_blocks_backward = True
                continue
            if backward and hasattr(layer, "_bf_plain_layer_forward") and cls in _DECODER_LAYERS:
                for m in (layer, attn, mlp, layer.input_layernorm, nxt):
                    m._bf_blocks_backward = True
            if (cls not in _DECODER_LAYERS or cls not in classic or hasattr(layer, "_bf_plain_layer_forward")
                    or type(attn).__name__ != _DECODER_LAYERS[cls]
                    or not _is_rmsnorm(getattr(layer, "input_layernorm", None))
                    or not _is_rmsnorm(getattr(layer, "post_attention_layernorm", None)) or not _is_rmsnorm(nxt)
                    or not all(isinstance(getattr(mlp, n, None), torch.nn.Module) for n in ("gate_proj", "up_proj", "down_proj"))
                    or not _is_silu(getattr(mlp, "act_fn", None))
                    or not all(isinstance(getattr(attn, n, None), torch.nn.Module) for n in ("q_proj", "k_proj", "v_proj", "o_proj"))
                    or getattr(attn, "head_dim", None) not in (64, 128)):
                continue
            layer._bf_next_norm = (nxt,)  # (in a tuple: not a child module of this layer)
            layer._bf_plain_layer_forward = layer.forward
            layer.forward = types.MethodType(_decoder_layer_forward, layer)
            attn._bf_plain_attn_forward = attn.forward
            attn.forward = types.MethodType(_decoder_attention_forward, attn)
            mlp._bf_plain_mlp_forward = mlp.forward
            mlp.forward = types.MethodType(_swiglu_mlp_forward, mlp)
            for norm in (layer.input_layernorm, nxt):
                if not hasattr(norm, "_bf_plain_rmsnorm_forward"):
                    norm._bf_plain_rmsnorm_forward = norm.forward
                    norm.forward = types.MethodType(_rmsnorm_forward, norm)
            if backward:
                for m in (layer, attn, mlp, layer.input_layernorm, nxt):
                    m._bf_blocks_backward = True
            fused += 1
    return fused
