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
from .ops import invalidate_caches  # noqa: F401
from .plan import kept_weight_bytes, kv_cache_bytes  # noqa: F401
from .random import (get_compute_dtype, manual_seed, set_compute_dtype, set_kl_gradient,  # noqa: F401
                     use_device_counter)

__all__ = ["to_bayesian", "to_bayesian_lora", "lora_state_dict", "invalidate_caches", "fuse_activations", "fuse_residual_layernorm", "fuse_shared_inputs", "fuse_ffn_pairs", "fuse_attention", "fuse_embeddings", "fuse_decoder_blocks", "enable_embedding", "nn", "manual_seed", "set_compute_dtype", "get_compute_dtype",
           "use_device_counter", "set_kl_gradient", "kept_weight_bytes", "kv_cache_bytes", "local_reparameterization"]


def to_bayesian(model: torch.nn.Module, initialization: Optional[Initialization] = DEFAULT_UNIFORM,
                prior: Optional[Parameter] = DEFAULT_SCALED_GAUSSIAN_MIXTURE, delta: float = None,
                freeze: bool = False) -> Model:
    """Deep-copy `model`, swap every layer whose exact class is in TORCH2BAYE for its Bayesian equivalent
    (`from_frequentist(layer, initialization, prior, delta, freeze)`, children visited in `named_children` order,
    depth first) and wrap the result in `bnn.Model`.

    Arguments / keyword arguments are the reference's: `delta` not None selects MOPED initialisation from the
    pretrained weights (Krishnan et al., arXiv:1906.05323), `freeze` freezes the posterior means."""

    def swap(module):
        for name, child in module.named_children():
            bayesian_cls = TORCH2BAYE.get(child.__class__)
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


_ATTENTION_NAME = "bayeformers_amd"


def _attention_interface(module, query, key, value, attention_mask, dropout: float = 0.0, scaling=None, **kwargs):
    """Attention function in the HuggingFace `AttentionInterface` convention: query/key/value [B, H, T, D], returns
    ([B, T, H, D], None).  Runs bf_attention_fwd (with bf_attention_bwd as its backward when a gradient is needed) when
    it applies (head size 64, T a multiple of 128, no mask or a key-padding mask; attention_probs_dropout runs inside the
    kernels on the Philox keep-mask of csrc/bf_philox.h); anything else goes to the
    framework's scaled-dot-product attention.  Causal calls (decoders) go to `_causal_attention`, whose kernels take any
    sequence length; the T % 128 limit here is the encoder kernels' alone, and `encoder_ragged_attention()` (off by default)
    lifts it: other lengths then run bf_attention_fwd_any / bf_attention_bwd_any, the same kernels' tail forms."""
    from transformers.integrations.sdpa_attention import sdpa_attention_forward

    from . import ops

    if getattr(key, "_bf_ring", None) is not None:  # a ring-buffer cache (kv_cache.RingStaticLayer), 16-bit or e4m3 rows
        return _ring_attention(module, query, key, value, attention_mask, dropout, scaling, **kwargs)
    if getattr(key, "_bf_kv8_scale", None) is not None:  # an FP8 cache (kv_cache.Fp8StaticLayer): key / value are e4m3 rows
        return _kv8_attention(module, query, key, value, attention_mask, dropout, scaling, **kwargs)
    need_grad = torch.is_grad_enabled() and (query.requires_grad or key.requires_grad or value.requires_grad)
    # causal: a mask _padding_mask_interface marked causal (the mask itself carries the structure), else what the caller
    # says with is_causal, else — with no mask — the module's own flag (HF decoders set module.is_causal and pass no mask
    # when nothing is padded); an explicit is_causal wins over the module flag, as in the framework's sdpa_attention_forward
    explicit = kwargs.get("is_causal", None)
    causal = bool(getattr(attention_mask, "_bf_causal", False) or getattr(attention_mask, "_bf_decode", False)
                  or getattr(attention_mask, "_bf_window", None) is not None
                  or getattr(attention_mask, "_bf_band", None) is not None) or (
        bool(explicit) if explicit is not None else (attention_mask is None and bool(getattr(module, "is_causal", False))))
    if causal:
        return _causal_attention(module, query, key, value, attention_mask, dropout, scaling, need_grad, **kwargs)
    # attention_probs_dropout (training mode) runs inside the kernels, forward and backward, for any supported length
    usable = ops.attention_supported(query, key, value)
    # under encoder_ragged_attention() (off by default): a length the kernels above refuse runs their tail forms
    # (bf_attention_fwd_any and its siblings) — the same masks, the same dropout contract, inference and training alike
    any_length = (not usable and encoder_ragged_attention_enabled() and ops.attention_any_supported(query, key, value))
    usable = usable or any_length
    key_mask = mask_off = None
    ready = getattr(attention_mask, "_bf_key_mask", None) if attention_mask is not None else None
    if usable and ready is not None and ready.shape == (query.shape[0], query.shape[2]):
        # built once per forward by _padding_mask_interface: additive fp32 [B, T] + the device flag "hides nothing"
        key_mask, mask_off = ready, attention_mask._bf_mask_off
    elif usable and attention_mask is not None:
        m = attention_mask
        B, H, T, _ = query.shape
        # a padding mask: [B, 1, 1 or T (broadcast), T]; per-query structure is not handled here
        if m.dim() == 4 and m.shape[0] == B and m.shape[1] == 1 and m.shape[3] == T and (m.shape[2] == 1 or m.stride(2) == 0):
            row = m[:, 0, 0, :]
            if row.dtype == torch.bool:
                key_mask = torch.where(row, 0.0, float("-inf")).to(torch.float32)
            else:
                key_mask = row.to(torch.float32).contiguous()
        else:
            usable = False
    if not usable:
        if attention_mask is not None and attention_mask.dtype not in (torch.bool, query.dtype):
            attention_mask = attention_mask.to(query.dtype)  # the framework's kernels want bool or the query's dtype
        return sdpa_attention_forward(module, query, key, value, attention_mask, dropout=dropout, scaling=scaling, **kwargs)
    scale = scaling if scaling is not None else query.shape[-1] ** -0.5
    drop = ops.Dropout(dropout, bfr.STATE.seed, bfr.dropout_call(), bfr.dropout_site(module), bfr.dropout_origin(),
                       bfr.dropout_counter()) if dropout > 0.0 else None
    if any_length:
        if need_grad:
            return ops.AttentionAnyFn.apply(query, key, value, key_mask, mask_off, scale, drop), None
        return ops.attention_forward_any(query, key, value, key_mask, scale, mask_off, drop=drop), None
    if need_grad:  # training: the same kernel, with bf_attention_bwd behind it
        return ops.AttentionFn.apply(query, key, value, key_mask, mask_off, scale, drop), None
    return ops.attention_forward(query, key, value, key_mask, scale, mask_off, drop=drop), None


def _ring_attention(module, query, key, value, attention_mask, dropout, scaling, **kwargs):
    """_attention_interface for a call against a ring-buffer cache: `key` and `value` are the [N, Hkv, ring_slots, D] tensors
    of a kv_cache.RingStaticLayer (Fp8RingStaticLayer: e4m3 rows with `_bf_kv8_scale`), marked `_bf_ring = (ring_slots,
    capacity)`, the key with sequence index j in row j % ring_slots.  A decode step — the mask carries the fill `_bf_kv_len`
    and the window `_bf_window`, at most 16 queries, no gradient, no dropout, no attention sinks, no key mask or a
    [N, capacity] one, the module's `sliding_window` agreeing with the mask's, a soft-cap only under `softcap_attention()` —
    runs bf_attention_decode_gqa_ring (bf_attention_decode_gqa_ring_kv8 on e4m3 rows).  ops.decode_kernel_wins is not
    consulted: nothing else can read a ring.  Every other call raises RuntimeError with the reason: the framework's
    attention would read the rows as if they lay in sequence order and be silently wrong."""
    from . import ops

    def refuse(why):
        raise RuntimeError("bayeformers_amd: the keys of this call are a ring-buffer cache (sliding_cache=\"ring\"), which only "
                           f"the ring decode kernels read, and {why}")

    slots, capacity = key._bf_ring
    if getattr(value, "_bf_ring", None) != key._bf_ring:
        refuse("its values are not the same ring's")
    k_scale, v_scale = getattr(key, "_bf_kv8_scale", None), getattr(value, "_bf_kv8_scale", None)
    if (k_scale is None) != (v_scale is None):
        refuse("only one of its keys and values carries FP8 scales")
    marked = attention_mask is not None
    kv_len = getattr(attention_mask, "_bf_kv_len", None) if marked else None
    window = getattr(attention_mask, "_bf_window", None) if marked else None
    key_mask = getattr(attention_mask, "_bf_key_mask", None) if marked else None
    softcap = kwargs.get("softcap", None)
    Tq = query.shape[2]
    if Tq > ops.DECODE_MAX_QUERIES:
        refuse(f"it carries {Tq} queries: a step takes at most {ops.DECODE_MAX_QUERIES} (a ring of window + "
               f"{ops.DECODE_MAX_QUERIES - 1} slots holds no more live keys; prefill_chunk is not supported)")
    if kv_len is None or window is None:
        refuse("its mask is not the sliding-window mask of a fixed-capacity cache (no `_bf_kv_len` or no `_bf_window`)")
    if torch.is_grad_enabled() and query.requires_grad:
        refuse("it needs a gradient")
    if dropout != 0.0:
        refuse(f"it carries attention dropout ({dropout})")
    if kwargs.get("s_aux", None) is not None:
        refuse("it carries attention sinks (s_aux)")
    if softcap is not None and not softcap_attention_enabled():
        refuse("it carries a logit soft-cap with softcap_attention() off")
    if "sliding_window" in kwargs and kwargs["sliding_window"] != window:
        refuse(f"the module's sliding_window={kwargs['sliding_window']!r} disagrees with the mask's window {window}")
    if window + Tq - 1 > slots:
        refuse(f"window {window} with {Tq} queries needs {window + Tq - 1} slots, the ring has {slots}")
    if key_mask is not None and tuple(key_mask.shape) != (query.shape[0], capacity):
        refuse(f"its key mask is {tuple(key_mask.shape)}, not [N, capacity] = {(query.shape[0], capacity)}")
    scale = scaling if scaling is not None else query.shape[-1] ** -0.5
    mask_off = getattr(attention_mask, "_bf_mask_off", None) if key_mask is not None else None
    cap = float(softcap) if softcap is not None else None
    if k_scale is not None:
        if not ops.attention_decode_kv8_supported(query, key, value):
            refuse("bf_attention_decode_gqa_ring_kv8 does not take its shapes, dtypes or strides")
        return ops.attention_forward_decode_ring_kv8(query, key, value, k_scale, v_scale, kv_len, key_mask, scale, mask_off,
                                                     None, window, slots, capacity, softcap=cap), None
    if not ops.attention_decode_supported(query, key, value):
        refuse("bf_attention_decode_gqa_ring does not take its shapes, dtypes or strides")
    return ops.attention_forward_decode_ring(query, key, value, kv_len, key_mask, scale, mask_off, None, window, slots,
                                             capacity, softcap=cap), None


def _kv8_attention(module, query, key, value, attention_mask, dropout, scaling, **kwargs):
    """_attention_interface for a call against an FP8 cache: `key` and `value` are the uint8 e4m3 rows of a
    kv_cache.Fp8StaticLayer, carrying their fp32 row scales as `_bf_kv8_scale`.  A decode step — the mask carries the fill
    `_bf_kv_len`, at most 16 queries, no gradient, no dropout, no attention sinks, no key mask or a [B, capacity] one, the
    module's `sliding_window` agreeing with the mask's — runs bf_attention_decode_gqa_kv8 on the rows as they are, with the
    mask's window and, under `softcap_attention()`, the call's soft-cap.  ops.decode_kernel_wins is not consulted: the FP8
    cache is a memory option and no other attention reads it.  Under `chunked_attention()` a cached chunk of more than 16
    queries (`_cached_chunk`) runs bf_attention_chunk_gqa_kv8 on the rows as they are, likewise.  Every other call dequantises the cache into bf16 first
    (ops.kv8_dequantize, the whole capacity: correct but slow) and then takes the path the bf16 tensors would have taken;
    the framework never sees the uint8 tensors."""
    from . import ops

    k_scale, v_scale = key._bf_kv8_scale, getattr(value, "_bf_kv8_scale", None)
    if v_scale is None:
        raise ValueError("bayeformers_amd: the keys of this call are FP8 cache rows but its values carry no scales")
    marked = attention_mask is not None
    kv_len = getattr(attention_mask, "_bf_kv_len", None) if marked else None
    window = getattr(attention_mask, "_bf_window", None) if marked else None
    key_mask = getattr(attention_mask, "_bf_key_mask", None) if marked else None
    softcap = kwargs.get("softcap", None)
    need_grad = torch.is_grad_enabled() and query.requires_grad
    if (kv_len is not None and query.shape[2] <= ops.DECODE_MAX_QUERIES and not need_grad and dropout == 0.0
            and kwargs.get("s_aux", None) is None
            and not (window is not None and "sliding_window" in kwargs and kwargs["sliding_window"] != window)
            and (softcap is None or softcap_attention_enabled())
            and (key_mask is None or tuple(key_mask.shape) == (query.shape[0], key.shape[2]))
            and ops.attention_decode_kv8_supported(query, key, value)):
        scale = scaling if scaling is not None else query.shape[-1] ** -0.5
        mask_off = getattr(attention_mask, "_bf_mask_off", None) if key_mask is not None else None
        return ops.attention_forward_decode_kv8(query, key, value, k_scale, v_scale, kv_len, key_mask, scale, mask_off,
                                                window=window,
                                                softcap=float(softcap) if softcap is not None else None), None
    if (_cached_chunk(query, key, attention_mask, need_grad, dropout, kwargs)
            and (softcap is None or softcap_attention_enabled()) and ops.attention_chunk_kv8_supported(query, key, value)):
        # a chunk of the chunked prefill: the rows as they are, no capacity-wide dequantise
        scale = scaling if scaling is not None else query.shape[-1] ** -0.5
        mask_off = getattr(attention_mask, "_bf_mask_off", None) if key_mask is not None else None
        return ops.attention_forward_chunk_kv8(query, key, value, k_scale, v_scale, kv_len, key_mask, scale, mask_off,
                                               window=window, softcap=float(softcap) if softcap is not None else None,
                                               key_origin=getattr(attention_mask, "_bf_key_origin", 0)), None
    return _attention_interface(module, query, ops.kv8_dequantize(key, k_scale), ops.kv8_dequantize(value, v_scale),
                                attention_mask, dropout, scaling, **kwargs)


def _cached_chunk(query, key, attention_mask, need_grad, dropout, kwargs) -> bool:
    """Whether a call is a cached chunk for the chunk entries (bf_attention_chunk_gqa and its kv8 sibling), under
    `chunked_attention()`: more than 16 new queries (fewer run the decode kernels) and no more than the keys, no gradient,
    no dropout, no attention sinks, one of _padding_mask_interface's cached-step masks (`_bf_decode`, or `_bf_kv_len` on a
    fixed-capacity cache — the first chunk into a static cache included) whose window, if any, the module's
    `sliding_window` agrees with, and no key mask or a [N, Tk] one.  The callers read the mask's fields themselves."""
    from . import ops

    if not chunked_attention_enabled() or attention_mask is None or need_grad or dropout != 0.0 \
            or kwargs.get("s_aux", None) is not None:
        return False
    if not ops.DECODE_MAX_QUERIES < query.shape[2] <= key.shape[2]:
        return False
    if not (bool(getattr(attention_mask, "_bf_decode", False)) or getattr(attention_mask, "_bf_kv_len", None) is not None):
        return False
    window = getattr(attention_mask, "_bf_window", None)
    if window is not None and "sliding_window" in kwargs and kwargs["sliding_window"] != window:
        return False
    key_mask = getattr(attention_mask, "_bf_key_mask", None)
    return key_mask is None or tuple(key_mask.shape) == (query.shape[0], key.shape[2])


def _causal_attention(module, query, key, value, attention_mask, dropout, scaling, need_grad, **kwargs):
    """The causal half of _attention_interface: bf_attention_fwd_gqa (bf_attention_bwd_gqa behind it) for equal query and
    key lengths — any length: one that is no multiple of 128 runs the kernels' tail forms, unless `ragged_attention(False)`
    or BF_NO_RAGGED_ATTENTION sends it to the framework — with no mask or _padding_mask_interface's causal mask; a decode
    step against a KV cache (fewer than 17 new queries, no gradient, no dropout) on bf_attention_decode_gqa, or on
    bf_attention_decode_gqa_len when the cache has
    a fixed capacity (the mask carries the filled length `_bf_kv_len`); other masks, longer cached chunks and attention
    dropout go to the framework's scaled-dot-product attention.  A sliding-window mask (`_bf_window`) takes the window
    siblings of the same entries, unless the module's own `sliding_window` argument disagrees with it.  A call that carries
    attention sinks (`s_aux`), which the kernels do not apply, goes to the framework with or without a window, on the
    prefill, decode and fixed-capacity paths alike.  Logit soft-capping (`softcap`, Gemma 2) takes the soft-cap entries
    (`_softcap_attention`) when `softcap_attention()` is on; with the switch off (the default) such a call goes to the
    framework's scaled-dot-product attention too, which does NOT apply the cap.  Head size 256 (Gemma): a full-attention
    forward without gradients and without a mask stays on the framework's attention too, whose is_causal form measured
    faster (ops.prefill_kernel_wins).  Under `chunked_attention()` (off by default) a cached chunk of more than 16 queries
    (`_cached_chunk`) runs bf_attention_chunk_gqa instead of the framework's attention, on a dynamic or a fixed-capacity
    cache, with or without a window."""
    from transformers.integrations.sdpa_attention import sdpa_attention_forward

    from . import ops

    band = getattr(attention_mask, "_bf_band", None) if attention_mask is not None else None
    if band is not None and kwargs.get("softcap", None) is None:
        return _packed_attention(module, query, key, value, attention_mask, dropout, scaling, need_grad, band, **kwargs)
    window = getattr(attention_mask, "_bf_window", None) if attention_mask is not None else None
    if (window is not None and "sliding_window" in kwargs and kwargs["sliding_window"] != window) \
            or kwargs.get("s_aux", None) is not None \
            or (kwargs.get("softcap", None) is not None and not softcap_attention_enabled()):
        return sdpa_attention_forward(module, query, key, value, attention_mask, dropout=dropout, scaling=scaling, **kwargs)
    if kwargs.get("softcap", None) is not None:
        return _softcap_attention(module, query, key, value, attention_mask, dropout, scaling, need_grad, window,
                                  float(kwargs["softcap"]), **{k: v for k, v in kwargs.items() if k != "softcap"})
    kv_len = getattr(attention_mask, "_bf_kv_len", None) if attention_mask is not None else None
    if _cached_chunk(query, key, attention_mask, need_grad, dropout, kwargs) \
            and ops.attention_chunk_supported(query, key, value) \
            and ops.chunk_kernel_wins(query.shape[1], key.shape[1], query.shape[2], key.shape[2], query.shape[3], window):
        # a chunk of the chunked prefill (chunked_attention(), off by default): bf_attention_chunk_gqa
        key_mask = getattr(attention_mask, "_bf_key_mask", None)
        mask_off = getattr(attention_mask, "_bf_mask_off", None) if key_mask is not None else None
        scale = scaling if scaling is not None else query.shape[-1] ** -0.5
        return ops.attention_forward_chunk(query, key, value, kv_len, key_mask, scale, mask_off, window=window,
                                           key_origin=getattr(attention_mask, "_bf_key_origin", 0)), None
    # the keys a decode step reads: all Tk, or with a window the ~W + Tq - 1 some query sees (decode_kernel_wins' Tk)
    read = key.shape[2] if window is None else min(key.shape[2], window + query.shape[2] - 1)
    if kv_len is not None:  # a step against a fixed-capacity cache: _padding_mask_interface's mask carries the fill
        key_mask = getattr(attention_mask, "_bf_key_mask", None)
        if (query.shape[2] < key.shape[2] and not need_grad and dropout == 0.0
                and ops.attention_decode_supported(query, key, value)
                and ops.decode_kernel_wins(query.shape[1], key.shape[1], query.shape[2], read, query.shape[3])
                and (key_mask is None or tuple(key_mask.shape) == (query.shape[0], key.shape[2]))):
            scale = scaling if scaling is not None else query.shape[-1] ** -0.5
            return ops.attention_forward_decode_len(query, key, value, kv_len, key_mask, scale,
                                                    getattr(attention_mask, "_bf_mask_off", None), window=window), None
        # (the bool mask hides the keys past the fill: the framework's attention over the whole capacity is exact)
        return sdpa_attention_forward(module, query, key, value, attention_mask, dropout=dropout, scaling=scaling, **kwargs)
    if (query.shape[2] < key.shape[2] and not need_grad and dropout == 0.0
            and ops.attention_decode_supported(query, key, value)
            and ops.decode_kernel_wins(query.shape[1], key.shape[1], query.shape[2], read, query.shape[3])):
        # no mask: nothing padded (a one-query step sees every cached key); else only the mask _padding_mask_interface built
        ready = attention_mask is None or bool(getattr(attention_mask, "_bf_decode", False))
        key_mask = getattr(attention_mask, "_bf_key_mask", None) if attention_mask is not None else None
        if ready and (key_mask is None or tuple(key_mask.shape) == (query.shape[0], key.shape[2])):
            mask_off = getattr(attention_mask, "_bf_mask_off", None) if key_mask is not None else None
            scale = scaling if scaling is not None else query.shape[-1] ** -0.5
            return ops.attention_forward_decode(query, key, value, key_mask, scale, mask_off, window=window), None
    key_mask = mask_off = None
    usable = (dropout == 0.0 and query.shape[2] == key.shape[2]
              and (query.shape[2] % 128 == 0 or ragged_attention_enabled())
              and ops.attention_supported(query, key, value, causal=True, kv_heads=key.shape[1])
              and ops.prefill_kernel_wins(query.shape[1], key.shape[1], query.shape[2], query.shape[3], need_grad, window,
                                          masked=attention_mask is not None))
    if usable and window is not None:  # the sliding mask of the cache-free sequence (key mask None: nothing padded)
        key_mask = getattr(attention_mask, "_bf_key_mask", None)
        usable = key_mask is None or tuple(key_mask.shape) == (query.shape[0], key.shape[2])
        mask_off = getattr(attention_mask, "_bf_mask_off", None) if key_mask is not None else None
    elif usable and attention_mask is not None:
        key_mask = getattr(attention_mask, "_bf_key_mask", None)
        usable = getattr(attention_mask, "_bf_causal", False) and key_mask is not None and \
            tuple(key_mask.shape) == (query.shape[0], key.shape[2])
        mask_off = getattr(attention_mask, "_bf_mask_off", None)
    if not usable:
        if attention_mask is not None and attention_mask.dtype not in (torch.bool, query.dtype):
            attention_mask = attention_mask.to(query.dtype)
        return sdpa_attention_forward(module, query, key, value, attention_mask, dropout=dropout, scaling=scaling, **kwargs)
    scale = scaling if scaling is not None else query.shape[-1] ** -0.5
    if window is not None:
        if need_grad:
            return ops.AttentionGqaFn.apply(query, key, value, key_mask, mask_off, scale, True, window), None
        return ops.attention_forward_gqa(query, key, value, key_mask, scale, True, mask_off, window=window), None
    if need_grad:
        return ops.AttentionGqaFn.apply(query, key, value, key_mask, mask_off, scale, True), None
    return ops.attention_forward_gqa(query, key, value, key_mask, scale, True, mask_off), None


def _packed_attention(module, query, key, value, attention_mask, dropout, scaling, need_grad, band, **kwargs):
    """_causal_attention for a packed-sequence mask (`_bf_band = (lo, hi)`, `_bf_band_window`: `_packed_mask`), without
    soft-capping: bf_attention_fwd_gqa_band (bf_attention_bwd_gqa_band behind it when a gradient is needed) under
    `packed_attention()`, for equal query and key lengths of any size (subject to `ragged_attention`) and the shapes
    ops.attention_supported takes.  Attention sinks (`s_aux`), a `sliding_window` argument that disagrees with the mask's
    window, attention dropout, unsupported shapes and the classes ops.prefill_kernel_wins sends there run the framework's
    scaled-dot-product attention over the dense mask, as every such call did before."""
    from transformers.integrations.sdpa_attention import sdpa_attention_forward

    from . import ops

    window = getattr(attention_mask, "_bf_band_window", None)
    B, H, T, D = query.shape
    usable = (packed_attention_enabled() and kwargs.get("s_aux", None) is None
              and not ("sliding_window" in kwargs and kwargs["sliding_window"] != window)
              and dropout == 0.0 and T == key.shape[2] and (T % 128 == 0 or ragged_attention_enabled())
              and ops.attention_supported(query, key, value, causal=True, kv_heads=key.shape[1])
              and tuple(band[0].shape) == (B, T) and tuple(band[1].shape) == (B, T)
              and ops.prefill_kernel_wins(H, key.shape[1], T, D, need_grad, window, masked=True))
    if not usable:
        return sdpa_attention_forward(module, query, key, value, attention_mask, dropout=dropout, scaling=scaling, **kwargs)
    scale = scaling if scaling is not None else D ** -0.5
    if need_grad:
        return ops.AttentionGqaBandFn.apply(query, key, value, band[0], band[1], scale), None
    return ops.attention_forward_gqa_band(query, key, value, band[0], scale), None


def _softcap_attention(module, query, key, value, attention_mask, dropout, scaling, need_grad, window, softcap, **kwargs):
    """_causal_attention for a call with logit soft-capping (HF Gemma2Attention: softcap = attn_logit_softcapping), under
    `softcap_attention()`: the same cases on the soft-cap entries — bf_attention_fwd_gqa_softcap (with
    bf_attention_bwd_gqa_softcap behind it) for prefill and training at any length (subject to `ragged_attention`),
    bf_attention_decode_gqa_softcap for a step against a cache, with the fill `_bf_kv_len` when its capacity is fixed, each
    with or without a window and a padding key mask.  The dispatch rules that weigh the kernels against the framework's
    attention are not consulted: that attention does not compute this function.  What the kernels do not take (attention
    dropout, a cached chunk of more than 16 queries, other masks, unsupported shapes or dtypes) runs `_softcap_eager`,
    never the framework's scaled-dot-product attention.  Under `chunked_attention()` such a cached chunk (`_cached_chunk`)
    runs bf_attention_chunk_gqa with the cap instead."""
    from . import ops

    scale = scaling if scaling is not None else query.shape[-1] ** -0.5
    Tq, Tk = query.shape[2], key.shape[2]
    marked = attention_mask is not None
    key_mask = getattr(attention_mask, "_bf_key_mask", None) if marked else None
    mask_off = getattr(attention_mask, "_bf_mask_off", None) if key_mask is not None else None
    keys_ok = key_mask is None or tuple(key_mask.shape) == (query.shape[0], Tk)
    kv_len = getattr(attention_mask, "_bf_kv_len", None) if marked else None
    plain = not need_grad and dropout == 0.0 and keys_ok
    if _cached_chunk(query, key, attention_mask, need_grad, dropout, kwargs) \
            and ops.attention_chunk_supported(query, key, value):
        # a chunk of the chunked prefill (chunked_attention()): bf_attention_chunk_gqa with the cap (kwargs: the call's other
        # arguments, for the sinks and the module's own window, which _causal_attention sends to the framework before this)
        return ops.attention_forward_chunk(query, key, value, kv_len, key_mask, scale, mask_off, window=window,
                                           softcap=softcap, key_origin=getattr(attention_mask, "_bf_key_origin", 0)), None
    if kv_len is not None:  # a step against a fixed-capacity cache
        if Tq < Tk and plain and ops.attention_decode_supported(query, key, value):
            return ops.attention_forward_decode_len(query, key, value, kv_len, key_mask, scale, mask_off, window=window,
                                                    softcap=softcap), None
    elif Tq < Tk:  # a step against a cache: no mask (one query, nothing padded) or _padding_mask_interface's
        if plain and ops.attention_decode_supported(query, key, value) \
                and (not marked or bool(getattr(attention_mask, "_bf_decode", False))):
            return ops.attention_forward_decode(query, key, value, key_mask, scale, mask_off, window=window,
                                                softcap=softcap), None
    elif (dropout == 0.0 and Tq == Tk and keys_ok and (Tq % 128 == 0 or ragged_attention_enabled())
          and ops.attention_supported(query, key, value, causal=True, kv_heads=key.shape[1])
          # no mask, the sliding mask (key mask None: nothing padded) or the causal padding mask
          and (not marked or window is not None or (getattr(attention_mask, "_bf_causal", False) and key_mask is not None))):
        if need_grad:
            return ops.AttentionGqaFn.apply(query, key, value, key_mask, mask_off, scale, True, window, softcap), None
        return ops.attention_forward_gqa(query, key, value, key_mask, scale, True, mask_off, window=window,
                                         softcap=softcap), None
    return _softcap_eager(module, query, key, value, attention_mask, dropout, scale, softcap), None


def _softcap_eager(module, query, key, value, attention_mask, dropout, scaling, softcap):
    """The fallback of `_softcap_attention`: the model's own eager chain (transformers' gemma2 eager_attention_forward:
    repeat_kv, matmul, `/ softcap`, tanh, `* softcap`, `+ mask`, fp32 softmax, dropout, matmul) in plain torch.  The mask
    arrives in the SDPA format (bool, True = visible) and is turned into the additive one the chain adds; no mask means
    causal, bottom-right aligned (the module's is_causal).  Returns [B, Tq, H, D]."""
    B, H, Tq, D = query.shape
    Tk, rep = key.shape[2], H // key.shape[1]
    if rep > 1:
        key = key[:, :, None].expand(B, key.shape[1], rep, Tk, D).reshape(B, H, Tk, D)
        value = value[:, :, None].expand(B, value.shape[1], rep, Tk, D).reshape(B, H, Tk, D)
    w = torch.matmul(query, key.transpose(2, 3)) * scaling
    w = torch.tanh(w / softcap) * softcap
    lowest = torch.finfo(w.dtype).min
    if attention_mask is None:
        if Tq > 1:
            seen = torch.ones((Tq, Tk), dtype=torch.bool, device=w.device).tril(Tk - Tq)
            w = w + torch.where(seen, 0.0, lowest).to(w.dtype)
    elif attention_mask.dtype == torch.bool:
        w = w + torch.where(attention_mask, 0.0, lowest).to(w.dtype)
    else:
        w = w + attention_mask.to(w.dtype)
    w = torch.nn.functional.softmax(w, dim=-1, dtype=torch.float32).to(query.dtype)
    w = torch.nn.functional.dropout(w, p=dropout, training=bool(getattr(module, "training", False)))
    return torch.matmul(w, value).transpose(1, 2).contiguous()


def _closure_cell(fn, name):
    """What the closure of `fn` holds under the free variable `name` (None: not a closure over it)."""
    code = getattr(fn, "__code__", None)
    if code is None or name not in code.co_freevars or fn.__closure__ is None:
        return None
    return fn.__closure__[code.co_freevars.index(name)].cell_contents


def _packed_sequence_of(mask_function):
    """(ids, W) when mask_function is exactly the composition transformers builds for packed sequences
    (masking_utils._preprocess_mask_arguments: position_ids that restart, no attention mask) — and_masks(f,
    packed_sequence_mask_function(ids)) over exactly two functions, f being causal_mask_function (W = None) or
    sliding_window_causal_mask_function(W) — else None.  `ids` is the [B, T] tensor of document indices, non-decreasing
    along T as find_packed_sequence_indices returns it (a cumulative sum)."""
    from transformers import masking_utils as mu

    if getattr(mask_function, "__code__", None) is not mu.and_masks(mu.causal_mask_function).__code__:
        return None
    fns = _closure_cell(mask_function, "mask_functions")
    if not isinstance(fns, tuple) or len(fns) != 2:
        return None
    if getattr(fns[1], "__code__", None) is not mu.packed_sequence_mask_function(None).__code__:
        return None
    ids = _closure_cell(fns[1], "packed_sequence_mask")
    if not isinstance(ids, torch.Tensor) or ids.dim() != 2 or ids.dtype.is_floating_point or ids.dtype == torch.bool:
        return None
    if fns[0] is mu.causal_mask_function:
        return ids, None
    window = _sliding_window_of(fns[0])
    return (ids, window) if window is not None else None


def _packed_mask(batch_size, q_length, kv_length, q_offset, kv_offset, ids, window, attention_mask, **kwargs):
    """The packed-sequence mask _padding_mask_interface builds on the device (NotImplemented: not the case it takes): the
    cache-free sequence, no padding mask, ids [batch_size, kv_length].  Query i sees key j iff j <= i, both lie in one
    document and — with a window — i - j < window: sdpa_mask's [B, 1, T, T] bool mask, carrying the bounds of banded
    causal attention `_bf_band = (lo, hi)` (ops.band_bounds) and `_bf_band_window` for the band entries."""
    from . import ops

    local_size = kwargs.get("local_size", None)
    if (kwargs.get("use_vmap", False) or attention_mask is not None or q_length is None or q_length != kv_length
            or not (isinstance(q_offset, int) and isinstance(kv_offset, int) and q_offset == 0 and kv_offset == 0)
            or tuple(ids.shape) != (batch_size, kv_length)
            or (local_size is not None and local_size != window)):
        return NotImplemented
    pos = torch.arange(kv_length, device=ids.device)
    seen = (pos[None, :] <= pos[:, None])[None, :, :] & (ids[:, :, None] == ids[:, None, :])
    if window is not None:
        seen = seen & (pos[None, :] > pos[:, None] - window)[None, :, :]
    out = seen[:, None, :, :]
    out._bf_band = ops.band_bounds(ids, window)
    out._bf_band_window = window
    return out


def _sliding_window_of(mask_function):
    """W when mask_function is exactly transformers' sliding_window_causal_mask_function(W) — and_masks over the two
    functions (sliding_window_overlay(W)'s inner function, causal_mask_function) and nothing else — else None."""
    from transformers import masking_utils as mu

    cell = _closure_cell
    if getattr(mask_function, "__code__", None) is not mu.and_masks(mu.causal_mask_function).__code__:
        return None
    fns = cell(mask_function, "mask_functions")
    if not isinstance(fns, tuple) or len(fns) != 2 or fns[1] is not mu.causal_mask_function:
        return None
    if getattr(fns[0], "__code__", None) is not mu.sliding_window_overlay(1).__code__:
        return None
    w = cell(fns[0], "sliding_window")
    return w if isinstance(w, int) and not isinstance(w, bool) and w >= 1 else None


def _sliding_mask(batch_size, q_length, kv_length, q_offset, kv_offset, window, attention_mask, **kwargs):
    """The three sliding-window causal masks _padding_mask_interface builds on the device (NotImplemented: not one of
    them; None: sdpa_mask's answer when the window hides nothing and nothing is padded).
    Query i (index q_offset + i) sees key j (index kv_offset + j) iff q_offset + i - window < kv_offset + j <= q_offset + i
    and the key is not padding — sdpa_mask's [B, 1, Tq, Tk] bool mask, carrying `_bf_window` and the key mask."""
    local_size = kwargs.get("local_size", None)
    if kwargs.get("use_vmap", False) or (local_size is not None and local_size != window) or q_length is None \
            or kv_length is None or not 0 < q_length <= kv_length:
        return NotImplemented
    if isinstance(q_offset, torch.Tensor):  # a fixed-capacity cache (see the causal case below): q_offset is its fill
        if kv_offset != 0 or not (attention_mask is None or (attention_mask.dim() == 2
                                                              and attention_mask.shape == (batch_size, kv_length))):
            return NotImplemented
        device = q_offset.device
        keys = torch.arange(kv_length, device=device)
        last = q_offset.reshape(()) + torch.arange(q_length, device=device)  # each query's own index
        tri = (keys[None, :] <= last[:, None]) & (keys[None, :] > last[:, None] - window)
        visible = None if attention_mask is None else (attention_mask if attention_mask.dtype == torch.bool
                                                       else attention_mask != 0)
        out = _with_keys(tri, visible, batch_size, q_length, kv_length)
        out._bf_decode = True
        out._bf_kv_len = (q_offset.reshape(()) + q_length).reshape(1)
        out._bf_window = window
        return out
    if not (isinstance(q_offset, int) and isinstance(kv_offset, int) and kv_offset >= 0
            and q_offset - kv_offset == kv_length - q_length):
        return NotImplemented
    if attention_mask is not None and not (attention_mask.dim() == 2
                                           and attention_mask.shape == (batch_size, kv_offset + kv_length)):
        return NotImplemented
    if attention_mask is None and kwargs.get("allow_is_causal_skip", True) and kv_length < window \
            and (q_length == 1 or q_length == kv_length):
        return None  # as sdpa_mask answers: the window hides nothing, module.is_causal routes the call
    device = attention_mask.device if attention_mask is not None else kwargs.get("device", "cpu")
    keys = torch.arange(kv_offset, kv_offset + kv_length, device=device)
    last = torch.arange(q_offset, q_offset + q_length, device=device)
    tri = (keys[None, :] <= last[:, None]) & (keys[None, :] > last[:, None] - window)
    visible = None
    if attention_mask is not None:
        visible = attention_mask[:, kv_offset:kv_offset + kv_length]
        visible = visible if visible.dtype == torch.bool else visible != 0
    out = _with_keys(tri, visible, batch_size, q_length, kv_length)
    if q_length < kv_length:
        out._bf_decode = True  # a step against a cache (bottom-right aligned)
    out._bf_window = window
    out._bf_key_origin = kv_offset  # the sequence index of key 0 (a sliding cache kept its last keys): the chunk entries' tile grid
    return out


def _with_keys(tri, visible, batch_size, q_length, kv_length):
    """tri [Tq, Tk] & the padding key mask visible [B, Tk] (None: nothing padded) as [B, 1, Tq, Tk], carrying the
    additive fp32 key mask and the device flag "nothing is hidden" (both None without padding)."""
    if visible is None:
        out = tri[None, None, :, :].expand(batch_size, 1, q_length, kv_length)
        out._bf_key_mask = out._bf_mask_off = None
        return out
    out = tri[None, None, :, :] & visible[:, None, None, :]
    out._bf_key_mask = torch.where(visible, 0.0, float("-inf")).to(torch.float32)
    out._bf_mask_off = visible.all().reshape(1)
    return out


def _padding_mask_interface(batch_size, q_length=None, kv_length=None, q_offset=0, kv_offset=0, mask_function=None,
                            attention_mask=None, **kwargs):
    """Mask function in the HuggingFace `AttentionMaskInterface` convention for models routed through
    `_attention_interface`.  A plain bidirectional padding mask [B, T] becomes, ONCE per forward and without a host
    round trip, the additive fp32 key mask bf_attention_fwd reads plus a one-byte device flag "nothing is hidden" that
    lets the kernel skip the mask (the framework's own function answers that question with `mask.all()` on the host —
    a device synchronisation in every forward, and a different code path under HIP-graph capture).  The 4-D tensor
    returned ([B, 1, 1, T] additive) is what the framework's attention takes when the kernel does not apply.
    A decoder's causal mask for a step against a KV cache (q_offset = kv_length - q_length, a 2-D padding mask or none)
    is built on the device too: the [B, 1, Tq, Tk] bool mask the framework's attention takes, carrying the key mask and
    the causal marker `_bf_decode` for bf_attention_decode_gqa (None for one query and no padding mask, as the framework answers).
    A step against a fixed-capacity cache (q_offset a device tensor: the fill of a transformers StaticCache, kv_length its
    capacity) gets the [B, 1, Tq, capacity] bool mask built on the device (causal from q_offset, the keys past the fill
    hidden) with the key mask and a snapshot of the fill after this step, `_bf_kv_len`, for bf_attention_decode_gqa_len.
    A sliding-window causal mask (exactly transformers' sliding_window_causal_mask_function(W)) is built the same three
    ways — the cache-free sequence, a step against a cache (a DynamicSlidingWindowLayer's kv_offset > 0 included: its
    key mask is the 2-D mask's slice at kv_offset) and a fixed-capacity cache — and carries `_bf_window = W` for the
    window entries; it is never None when the window hides something.
    Packed sequences (exactly and_masks(causal_mask_function or sliding_window_causal_mask_function(W),
    packed_sequence_mask_function(ids)), the cache-free sequence, no padding mask: `_packed_mask`) get the same dense bool
    mask carrying `_bf_band = (lo, hi)` and `_bf_band_window` for the band entries — and none of the other markers.
    Anything else (4-D masks, extra mask functions, other offsets) goes to the framework's scaled-dot-product mask."""
    from transformers.masking_utils import bidirectional_mask_function, causal_mask_function, sdpa_mask

    window = _sliding_window_of(mask_function) if mask_function is not causal_mask_function else None
    packed = _packed_sequence_of(mask_function) if mask_function is not causal_mask_function and window is None else None
    if packed is not None:
        out = _packed_mask(batch_size, q_length, kv_length, q_offset, kv_offset, packed[0], packed[1], attention_mask,
                           **kwargs)
        if out is not NotImplemented:
            return out
    if window is not None:
        out = _sliding_mask(batch_size, q_length, kv_length, q_offset, kv_offset, window, attention_mask, **kwargs)
        if out is not NotImplemented:
            return out

    if (mask_function is causal_mask_function and isinstance(q_offset, torch.Tensor) and kv_offset == 0
            and q_length is not None and kv_length is not None and 0 < q_length <= kv_length
            and not kwargs.get("use_vmap", False)
            and (attention_mask is None or (attention_mask.dim() == 2 and attention_mask.shape == (batch_size, kv_length)))):
        # a fixed-capacity cache (transformers' StaticLayer: q_offset is its fill count, a device tensor, and kv_length its
        # capacity).  Tested before the comparisons below: on a tensor they synchronise with the host (or fail a capture).
        # Query i sees keys 0 .. q_offset + i, which hides the keys past the fill; the snapshot kv_len is the fill after
        # this forward's update (the cache bumps its counter in place during the forward)
        device = q_offset.device
        kv_len = (q_offset.reshape(()) + q_length).reshape(1)
        keys = torch.arange(kv_length, device=device)
        tri = keys[None, :] <= (q_offset.reshape(()) + torch.arange(q_length, device=device))[:, None]
        if attention_mask is None:
            out = tri[None, None, :, :].expand(batch_size, 1, q_length, kv_length)
            out._bf_key_mask = out._bf_mask_off = None
        else:
            visible = attention_mask if attention_mask.dtype == torch.bool else attention_mask != 0
            out = tri[None, None, :, :] & visible[:, None, None, :]
            out._bf_key_mask = torch.where(visible, 0.0, float("-inf")).to(torch.float32)
            out._bf_mask_off = visible.all().reshape(1)
        out._bf_decode = True
        out._bf_kv_len = kv_len
        return out

    if (mask_function is causal_mask_function and kv_offset == 0 and q_length is not None and kv_length is not None
            and 0 < q_length < kv_length and q_offset == kv_length - q_length and not kwargs.get("use_vmap", False)
            and (attention_mask is None or (attention_mask.dim() == 2 and attention_mask.shape == (batch_size, kv_length)))):
        if attention_mask is None and q_length == 1:
            return None  # the new query sees every cached key: module.is_causal routes the call
        device = attention_mask.device if attention_mask is not None else kwargs.get("device", "cpu")
        keys = torch.arange(kv_length, device=device)
        tri = keys[None, :] <= torch.arange(q_offset, kv_length, device=device)[:, None]  # query i sees 0 .. q_offset + i
        if attention_mask is None:
            out = tri[None, None, :, :].expand(batch_size, 1, q_length, kv_length)
            out._bf_key_mask = out._bf_mask_off = None
        else:
            visible = attention_mask if attention_mask.dtype == torch.bool else attention_mask != 0
            out = tri[None, None, :, :] & visible[:, None, None, :]
            out._bf_key_mask = torch.where(visible, 0.0, float("-inf")).to(torch.float32)
            out._bf_mask_off = visible.all().reshape(1)
        out._bf_decode = True  # causal, bottom-right aligned (_bf_causal stays the cache-free marker)
        return out

    if (mask_function is causal_mask_function and q_offset == 0 and kv_offset == 0 and q_length == kv_length
            and not kwargs.get("use_vmap", False)
            and (attention_mask is None or (attention_mask.dim() == 2 and attention_mask.shape == (batch_size, kv_length)))):
        # a decoder's causal mask over the cache-free sequence: None when nothing is padded (the framework's answer too:
        # the attention is then causal by module.is_causal); with a padding mask, sdpa_mask's [B, 1, T, T] bool mask built
        # on the device without a host round trip, carrying the key mask and "causal" for bf_attention_fwd_gqa
        if attention_mask is None:
            return None
        visible = attention_mask if attention_mask.dtype == torch.bool else attention_mask != 0
        additive = torch.where(visible, 0.0, float("-inf")).to(torch.float32)
        tri = torch.ones((q_length, kv_length), dtype=torch.bool, device=visible.device).tril()
        out = tri[None, None, :, :] & visible[:, None, None, :]
        out._bf_key_mask = additive
        out._bf_mask_off = visible.all().reshape(1)
        out._bf_causal = True
        return out
    plain = (attention_mask is not None and attention_mask.dim() == 2 and mask_function is bidirectional_mask_function
             and not kwargs.get("use_vmap", False) and q_offset == 0 and kv_offset == 0
             and attention_mask.shape == (batch_size, kv_length))
    if attention_mask is None and mask_function is bidirectional_mask_function:
        return None
    if not plain:
        return sdpa_mask(batch_size=batch_size, q_length=q_length, kv_length=kv_length, q_offset=q_offset,
                         kv_offset=kv_offset, mask_function=mask_function, attention_mask=attention_mask, **kwargs)
    visible = attention_mask if attention_mask.dtype == torch.bool else attention_mask != 0
    additive = torch.where(visible, 0.0, float("-inf")).to(torch.float32)  # one launch (fp32 already: .to is a no-op)
    out = additive[:, None, None, :]
    out._bf_key_mask = additive
    out._bf_mask_off = visible.all().reshape(1)  # stays on the device
    return out


_RAGGED_ATTENTION = [True]


def ragged_attention(enable: bool = True) -> None:
    """Switch the causal attention kernels for sequence lengths that are no multiple of 128 (the tail forms of
    bf_attention_fwd_gqa / bf_attention_bwd_gqa and their window siblings) on or off for this process;
    BF_NO_RAGGED_ATTENTION in the environment switches them off too.  Off: such a prefill or training step runs the
    framework's scaled-dot-product attention, as every length but the multiples of 128 did before.  The switch is part of
    what a captured forward bakes in (graphs.baked_state): a replayed forward is captured again after a flip."""
    _RAGGED_ATTENTION[0] = bool(enable)


def ragged_attention_enabled() -> bool:
    return _RAGGED_ATTENTION[0] and os.environ.get("BF_NO_RAGGED_ATTENTION") is None


_PACKED_ATTENTION = [True]


def packed_attention(enable: bool = True) -> None:
    """Switch the band attention kernels for packed sequences (bf_attention_fwd_gqa_band / bf_attention_bwd_gqa_band:
    position ids that restart at each document, no attention mask) on or off for this process; BF_NO_PACKED_ATTENTION in
    the environment switches them off too.  Off: such a prefill or training step runs the framework's scaled-dot-product
    attention over the dense [B, 1, T, T] mask, as it did before.  The switch is part of what a captured forward bakes in
    (graphs.baked_state): a replayed forward is captured again after a flip."""
    _PACKED_ATTENTION[0] = bool(enable)


def packed_attention_enabled() -> bool:
    return _PACKED_ATTENTION[0] and os.environ.get("BF_NO_PACKED_ATTENTION") is None


_SOFTCAP_ATTENTION = [False]


def softcap_attention(enable: bool = True) -> None:
    """Switch the soft-cap attention kernels (bf_attention_fwd_gqa_softcap / bf_attention_bwd_gqa_softcap /
    bf_attention_decode_gqa_softcap) on or off for this process; BF_SOFTCAP_ATTENTION in the environment switches them on
    too.  OFF by default.  On: a causal attention call that carries `softcap` (HF Gemma 2: attn_logit_softcapping) runs
    them — prefill, training, cached decode and fixed-capacity decode — and what they do not take runs the model's eager
    chain with the cap.  Off: such a call goes to the framework's scaled-dot-product attention, which ignores `softcap`:
    the result is then NOT the model's function (keep such a model on its `eager` attention, or switch this on).  The
    switch is part of what a captured forward bakes in (graphs.baked_state): a replayed forward is captured again after a
    flip."""
    _SOFTCAP_ATTENTION[0] = bool(enable)


def softcap_attention_enabled() -> bool:
    return _SOFTCAP_ATTENTION[0] or os.environ.get("BF_SOFTCAP_ATTENTION") is not None


_CHUNKED_ATTENTION = [False]


def chunked_attention(enable: bool = True) -> None:
    """Switch the cached-chunk attention kernels (bf_attention_chunk_gqa / bf_attention_chunk_gqa_kv8) on or off for this
    process; BF_CHUNKED_ATTENTION in the environment switches them on too.  OFF by default.  On: a forward of more than 16
    new tokens against a KV cache — a chunk of a chunked prefill — without gradient, dropout or attention sinks runs them
    (`_cached_chunk`): on a dynamic cache, on a fixed-capacity one (the fill is a device scalar), on an FP8 cache without
    dequantising it, with a sliding window, and with soft-capping under `softcap_attention()`.  Off: such a call goes
    where it always went — the framework's scaled-dot-product attention over the dense mask, the capped eager chain, or a
    capacity-wide dequantise first.  `sample_generate(prefill_chunk=...)` turns it on for its prefill and restores it."""
    _CHUNKED_ATTENTION[0] = bool(enable)


def chunked_attention_enabled() -> bool:
    return _CHUNKED_ATTENTION[0] or os.environ.get("BF_CHUNKED_ATTENTION") is not None


_ENCODER_RAGGED_ATTENTION = [False]


def encoder_ragged_attention(enable: bool = True) -> None:
    """Switch the any-length encoder attention kernels (bf_attention_fwd_any / bf_attention_bwd_any and their dropout and
    rows siblings: the tail forms of the encoder kernels) on or off for this process; BF_ENCODER_RAGGED_ATTENTION in the
    environment switches them on too.  OFF by default.  On: a non-causal attention call of head size 64 whose length is
    no multiple of 128 (a batch padded to its longest sentence, a ViT's 197 tokens) runs them — inference, training with
    attention_probs_dropout on the Philox keep-masks (the dropout contract of csrc/bf_philox.h then holds at every
    length), and the [CLS] row of a pooled head's last layer — with the masks `_attention_interface` takes.  Off: such
    a call runs the framework's scaled-dot-product attention over the dense mask, dropout from the framework's generator.
    The switch is part of what a captured forward bakes in (graphs.baked_state): a replayed forward is captured again
    after a flip.  profiles/encoder_ragged_attention.md says when it pays."""
    _ENCODER_RAGGED_ATTENTION[0] = bool(enable)


def encoder_ragged_attention_enabled() -> bool:
    return _ENCODER_RAGGED_ATTENTION[0] or os.environ.get("BF_ENCODER_RAGGED_ATTENTION") is not None


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
        ready = getattr(attention_mask, "_bf_key_mask", None)
        if ready is not None and ready.shape == (Bt, T):
            key_mask, mask_off = ready, attention_mask._bf_mask_off
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


def _rmsnorm_forward(self, hidden_states):
    """forward of an HF `*RMSNorm` on bf_add_rmsnorm.  A hidden state that the fused layer in front of this norm produced
    carries this norm's output already (`_bf_normed`, computed in that layer's residual pass): it is handed out as it is.
    Under recorded gradients (fuse_decoder_blocks(backward=True)) the attached tensor is the second output of the autograd
    function whose first output is the hidden state; it is taken only when it carries a grad_fn — whatever this forward
    returns under recorded gradients must be part of the graph, and reentrant checkpointing or layers run under no_grad
    hand out graph-less ones — and it stays attached, so a recomputation of this forward sees what the first run saw."""
    from . import ops

    x = hidden_states
    rec = _records_grad(x, self)
    if not ops.rmsnorm_supported(x, None, self) or (rec and not _blocks_backward(self)):
        return self._bf_plain_rmsnorm_forward(hidden_states)
    ready = x.__dict__.get("_bf_normed") if rec else x.__dict__.pop("_bf_normed", None)
    if ready is not None and ready[1] is self and not (rec and ready[0].grad_fn is None):
        return ready[0]
    if rec:
        return ops.AddRMSNormFn.apply(x, None, self.weight, self.variance_epsilon)
    return ops.add_rmsnorm(x, None, self.weight, self.variance_epsilon, want_sum=False)[1]


def _decoder_layer_forward(self, hidden_states, attention_mask=None, position_ids=None, past_key_values=None,
                           use_cache=False, position_embeddings=None, **kwargs):
    """forward of an HF Llama / Mistral / Qwen2 decoder layer with its two residual adds folded into the RMSNorm that
    follows each (bf_add_rmsnorm writes the sum and the normalised row in one pass): the second add feeds the NEXT
    layer's input norm (or the model's final norm), whose output travels on the returned hidden state as `_bf_normed`.
    The returned tensor is always the true hidden state.  Tensors off the device, a hook on the norm whose forward is
    skipped: the module's own forward; gradients recorded or training mode as well, unless the layer was rewritten with
    backward=True — then the two passes run through ops.AddRMSNormFn, whose backward is bf_add_rmsnorm_bwd."""
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
    add_rmsnorm = ops.AddRMSNormFn.apply if rec else ops.add_rmsnorm
    if ops.rmsnorm_supported(a, h, post):
        h1, y1 = add_rmsnorm(a, h, post.weight, post.variance_epsilon)
    else:
        h1 = h + a
        y1 = post(h1)
    m = self.mlp(y1)
    if not ops.rmsnorm_supported(m, h1, nxt):
        return h1 + m
    h2, y2 = add_rmsnorm(m, h1, nxt.weight, nxt.variance_epsilon)
    h2._bf_normed = (y2, nxt)
    return h2


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


def _swiglu_mlp_forward(self, x):
    """forward of an HF Llama-style MLP — down_proj(act_fn(gate_proj(x)) * up_proj(x)) — with the SiLU and the product as
    one launch (bf_swiglu); rewritten with backward=True, under recorded gradients and in training mode too, through
    ops.SwiGLUFn."""
    from . import ops

    rec = isinstance(x, torch.Tensor) and _records_grad(x, self)
    if (not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype not in ops._TORCH2BF or _hooked(self.act_fn)
            or ((self.training or rec) and not _blocks_backward(self))):
        return self._bf_plain_mlp_forward(x)
    gate, up = self.gate_proj(x), self.up_proj(x)
    if not ops.swiglu_supported(gate, up):
        return self.down_proj(self.act_fn(gate) * up)
    return self.down_proj(ops.SwiGLUFn.apply(gate, up) if rec else ops.swiglu(gate, up))


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


def _norm_eps(norm) -> float:
    return norm.eps if hasattr(norm, "eps") else norm.variance_epsilon


def _gemma_rmsnorm_forward(self, hidden_states):
    """forward of an HF Gemma*RMSNorm on bf_norm_add_rmsnorm (no first norm, no residual, offset 1).  A hidden state that
    the fused layer in front of this norm produced carries this norm's output already (`_bf_normed`, as _rmsnorm_forward
    describes): it is handed out as it is.  Under recorded gradients the module's own forward runs, unless the norm was
    rewritten with backward="all": then _rmsnorm_forward's rules for the attached tensor hold and the norm runs through
    ops.NormAddRMSNormFn."""
    from . import ops

    x = hidden_states
    rec = isinstance(x, torch.Tensor) and _records_grad(x, self)
    if (not isinstance(x, torch.Tensor) or (rec and not _blocks_backward(self)) or not x.is_cuda
            or not ops.norm_add_rmsnorm_supported(x, None, None, self)):
        return self._bf_plain_rmsnorm_forward(hidden_states)
    ready = x.__dict__.get("_bf_normed") if rec else x.__dict__.pop("_bf_normed", None)
    if ready is not None and ready[1] is self and not (rec and ready[0].grad_fn is None):
        return ready[0]
    if rec:
        return ops.NormAddRMSNormFn.apply(x, None, None, self.weight, 0.0, self.eps, 1)
    return ops.norm_add_rmsnorm(x, None, None, self.weight, 0.0, self.eps, 1, want_sum=False)[1]


def _gemma_layer_forward(self, hidden_states, attention_mask=None, position_ids=None, past_key_values=None,
                         use_cache=False, position_embeddings=None, **kwargs):
    """forward of an HF GemmaDecoderLayer: _decoder_layer_forward's structure (each residual add folded into the norm that
    follows it, the second one's output travelling on the hidden state as `_bf_normed`) through bf_norm_add_rmsnorm with the
    (1 + weight) convention.  Tensors off the device or a hook on the norm whose forward is skipped send the layer to its
    own forward; gradients recorded or training mode as well, unless the layer was rewritten with backward="all" — then the
    two passes run through ops.NormAddRMSNormFn, whose backward is bf_norm_add_rmsnorm_bwd."""
    from . import ops

    h = hidden_states
    post, nxt = self.post_attention_layernorm, self._bf_next_norm[0]
    rec = isinstance(h, torch.Tensor) and _records_grad(h, self, nxt)
    if (not isinstance(h, torch.Tensor) or ((self.training or rec) and not _blocks_backward(self)) or _hooked(post)
            or not ops.norm_add_rmsnorm_supported(h, None, None, post)
            or not ops.norm_add_rmsnorm_supported(h, None, None, nxt)):
        return self._bf_plain_layer_forward(hidden_states, attention_mask=attention_mask, position_ids=position_ids,
                                            past_key_values=past_key_values, use_cache=use_cache,
                                            position_embeddings=position_embeddings, **kwargs)
    a, _ = self.self_attn(hidden_states=self.input_layernorm(h), attention_mask=attention_mask, position_ids=position_ids,
                          past_key_values=past_key_values, use_cache=use_cache, position_embeddings=position_embeddings,
                          **kwargs)
    norm_add_rmsnorm = ops.NormAddRMSNormFn.apply if rec else ops.norm_add_rmsnorm
    if ops.norm_add_rmsnorm_supported(a, None, h, post):
        h1, y1 = norm_add_rmsnorm(a, None, h, post.weight, 0.0, post.eps, 1)
    else:
        h1 = h + a
        y1 = post(h1)
    m = self.mlp(y1)
    if not ops.norm_add_rmsnorm_supported(m, None, h1, nxt):
        return h1 + m
    h2, y2 = norm_add_rmsnorm(m, None, h1, nxt.weight, 0.0, nxt.eps, 1)
    h2._bf_normed = (y2, nxt)
    return h2


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


def _geglu_mlp_forward(self, x):
    """forward of an HF Gemma-style MLP — down_proj(gelu_tanh(gate_proj(x)) * up_proj(x)) — with the activation and the
    product as one launch (bf_geglu); rewritten with backward="all", under recorded gradients and in training mode too,
    through ops.GeGLUFn."""
    from . import ops

    rec = isinstance(x, torch.Tensor) and _records_grad(x, self)
    if (not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype not in ops._TORCH2BF or _hooked(self.act_fn)
            or ((self.training or rec) and not _blocks_backward(self))):
        return self._bf_plain_mlp_forward(x)
    gate, up = self.gate_proj(x), self.up_proj(x)
    if not ops.geglu_supported(gate, up):
        return self.down_proj(self.act_fn(gate) * up)
    return self.down_proj(ops.GeGLUFn.apply(gate, up) if rec else ops.geglu(gate, up))


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
    (q / k norms), Gemma (1 + weight), OLMo and mixture-of-experts layers are left alone.  By default an inference-time
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


def fuse_attention(model: torch.nn.Module) -> bool:
    """Route the wrapped HuggingFace model's attention through bf_attention_fwd: registers an attention function in
    transformers' AttentionInterface (mask format: the scaled-dot-product one) and selects it in the model's config.
    The function falls back to the framework's attention for anything it does not take.  A decoder's causal attention
    (Llama, Mistral, Qwen2, Gemma: grouped heads, sliding windows, head size 64, 128 or 256) runs bf_attention_fwd_gqa
    at any sequence length (`ragged_attention(False)` or BF_NO_RAGGED_ATTENTION: at multiples of 128 only); a call with
    attention sinks (gpt-oss) goes to the framework.  Logit soft-capping (Gemma 2) runs the soft-cap entries
    (bf_attention_fwd_gqa_softcap and its backward and decode siblings) once `softcap_attention()` or BF_SOFTCAP_ATTENTION
    switches them on; with that switch off, the default, such a call goes to the framework's scaled-dot-product attention,
    which ignores the cap — the model then computes another function than its `eager` attention.  Packed sequences
    (position ids that restart at each document, no attention mask, no cache) run the band entries
    (bf_attention_fwd_gqa_band / bf_attention_bwd_gqa_band) unless `packed_attention(False)` or BF_NO_PACKED_ATTENTION
    sends them to the framework's attention over the dense mask.  The ops around the
    attention of those families (norms, rotary embedding, gate) are fuse_decoder_blocks's, opt-in by its `families`.  Returns False (and changes
    nothing) when the model has no HuggingFace config or transformers lacks the interface.
    A BertForSequenceClassification also gets the narrow last encoder layer (`_pooled_last_layer_forward`): in evaluation
    forwards that ask for neither hidden states nor attentions, everything behind the last layer's key / value
    projections runs on the [CLS] rows alone (`pooled_last_layer(False)` or BF_NO_POOLED_LAST_LAYER: on every row)."""
    try:
        from transformers import AttentionInterface
        from transformers.masking_utils import AttentionMaskInterface, sdpa_mask
    except ImportError:
        return False
    inner = model.model if isinstance(model, Model) and model.model is not None else model
    config = getattr(inner, "config", None)
    if config is None or not hasattr(config, "_attn_implementation"):
        return False
    AttentionInterface.register(_ATTENTION_NAME, _attention_interface)
    AttentionMaskInterface.register(_ATTENTION_NAME, _padding_mask_interface)
    for m in inner.modules():
        c = getattr(m, "config", None)
        if c is not None and hasattr(c, "_attn_implementation"):
            c._attn_implementation = _ATTENTION_NAME
    _install_pooled_last_layer(inner)
    return True
