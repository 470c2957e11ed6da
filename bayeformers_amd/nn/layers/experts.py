# -*- coding: utf-8 -*-
"""bayeformers_amd.nn.layers.experts

The experts of a mixture-of-experts decoder block (transformers' `MixtralExperts` / `Qwen3MoeExperts`: two 3-D parameters,
gate_up_proj [E, 2I, H] and down_proj [E, H, I]) with a Gaussian posterior on both, include/bayeformers_amd_moe.h:

    W_s      = mu + softplus(rho) * eps(seed, sample_base + s, stream 2 * layer_id + {0, 1}, e)      for both tensors
    h[r, j]  = act(x[r] Wg^T) * (x[r] Wu^T)      [Wg; Wu] = gate_up_s[e], e = top_k_index[r, j], s = the row's sample
    out[r]   = sum_j top_k_weights[r, j] * (h[r, j] down_s[e]^T)
    {log_prior, log_variational_posterior}[s] of both draws

One bf_sample_logprob launch draws both tensors for all S samples; the products are bf_moe_route / bf_moe_gate_up /
bf_moe_down / bf_moe_combine — a grouped GEMM over the S * E (sample, expert) pairs laid out on the device, so a decode step
with such a layer can be graph-captured.  What ops.moe_supported refuses (fp32 compute, another activation, odd shapes) runs
the framework's loop per (sample, expert) on the same draws; that loop waits for the device and cannot be captured.  The
backward runs the same loop under autograd (backward kernels: not yet).  The router stays the framework's and
deterministic.  Not a bnn.Linear: the cross-layer sampling plan, the deferred gradient table and local_reparameterization
never see it.
"""
from typing import Optional

import torch
from torch import Size, Tensor
from torch.nn import Module

from ... import ops
from ... import random as bfr
from ..parameters.base import Parameter
from ..parameters.gaussian import DEFAULT_SCALED_GAUSSIAN_MIXTURE, Gaussian
from ..parameters.initializations import DEFAULT_UNIFORM, Initialization
from .base import KernelLayer
from .linear import _moped


class _ExpertsFn(torch.autograd.Function):
    """Autograd node of Experts.forward.  Backward = the reference's graph for sampled weights: gradients through the
    framework composite on the saved x, the draws and the routing, W = mu + eps * softplus(rho) with eps regenerated from the
    Philox counter and the log-prob scalars detached.  The routing weights get their gradient: the router trains through it."""

    @staticmethod
    def forward(ctx, x, wts, mu_gu, rho_gu, mu_d, rho_d, idx, layer, S, seed, base, lp_out, kept, need_grad):
        ctx.layer, ctx.S, ctx.seed, ctx.base = layer, S, seed, base
        ctx.counter = bfr.counter_snapshot(need_grad)
        # (kept: pinned_samples(keep_weights=True) — the block's first forward drew them, and their log-probs)
        w_gu, w_d = kept if kept is not None else layer.sample_weights(S, seed, base, lp_out, x.dtype)
        out = ops.moe_forward(x, idx, wts, w_gu, w_d, S, layer.act_fn)
        if need_grad:
            ctx.save_for_backward(x, wts, idx, w_gu, w_d)
        return out

    @staticmethod
    def backward(ctx, grad):
        x, wts, idx, w_gu, w_d = ctx.saved_tensors
        layer, S = ctx.layer, ctx.S
        need = ctx.needs_input_grad
        need_w = any(need[2:6])
        dx, dwts, dgu, dd = ops.moe_backward(x, grad, idx, wts, w_gu, w_d, S, layer.act_fn, need[0], need[1], need_w)
        grads = [None] * 4
        if need_w:
            with bfr.counter_override(ctx.counter):
                for i, (dw, gauss, sid) in enumerate(((dgu, layer.gate_up_proj, 2 * layer.layer_id),
                                                      (dd, layer.down_proj, 2 * layer.layer_id + 1))):
                    if need[2 + 2 * i] or need[3 + 2 * i]:
                        dmu, drho = ops.reduce_param_grad(dw, gauss, sid, S, ctx.seed, ctx.base, need[2 + 2 * i])
                        grads[2 * i], grads[2 * i + 1] = dmu, (drho if need[3 + 2 * i] else None)
        return (dx, dwts, *grads, None, None, None, None, None, None, None, None)


class Experts(KernelLayer):
    """Bayesian experts of a mixture-of-experts block.

    Attributes: num_experts, hidden_dim, intermediate_dim, act_fn (the framework module's); gate_up_proj (Gaussian
    [E, 2I, H], fp32 mu / rho) with gate_up_proj_prior; down_proj (Gaussian [E, H, I]) with down_proj_prior; log_prior,
    log_variational_posterior (of both); layer_id, compute_dtype, log_prob_samples as bnn.Linear."""

    def __init__(self, num_experts: int, hidden_dim: int, intermediate_dim: int, act_fn=None,
                 initialization: Optional[Initialization] = DEFAULT_UNIFORM,
                 prior: Optional[Parameter] = DEFAULT_SCALED_GAUSSIAN_MIXTURE) -> None:
        super(Experts, self).__init__()
        self.num_experts, self.hidden_dim, self.intermediate_dim = num_experts, hidden_dim, intermediate_dim
        self.act_fn = act_fn if act_fn is not None else torch.nn.SiLU()
        self.initialization = initialization
        self.gate_up_proj = Gaussian(Size((num_experts, 2 * intermediate_dim, hidden_dim)), self.initialization)
        self.gate_up_proj_prior = prior
        self.down_proj = Gaussian(Size((num_experts, hidden_dim, intermediate_dim)), self.initialization)
        self.down_proj_prior = prior
        self._init_kernel_layer()

    def extra_repr(self) -> str:
        return (f"num_experts={self.num_experts}, hidden_dim={self.hidden_dim}, intermediate_dim={self.intermediate_dim}")

    def gaussians(self):
        yield self.gate_up_proj, self.gate_up_proj_prior, 2 * self.layer_id
        yield self.down_proj, self.down_proj_prior, 2 * self.layer_id + 1

    def sample_weights(self, S: int, seed: int, base: int, lp_out: Optional[Tensor], x_dtype: torch.dtype):
        """(gate_up_s [S, E, 2I, H], down_s [S, E, H, I]) in the compute dtype (16-bit) or fp32 from ONE sampling launch, with
        {log_prior, log_q} per sample, summed over the two tensors, into lp_out."""
        cdt = self.compute_dtype or bfr.get_compute_dtype()
        wdt = cdt if (cdt != torch.float32 and x_dtype == cdt) else torch.float32
        (w_gu, w_d), lp = ops.sample_logprob([self.gate_up_proj, self.down_proj],
                                             [self.gate_up_proj_prior, self.down_proj_prior],
                                             [2 * self.layer_id, 2 * self.layer_id + 1], S, seed, base, out_dtype=wdt)
        ops.MOE_CALLS["sample"] += 1
        if lp_out is not None:
            lp_out.copy_(lp)
        return w_gu, w_d

    def forward(self, hidden_states: Tensor, top_k_index: Tensor, top_k_weights: Tensor) -> Tensor:
        """The framework module's forward on sampled weights.  hidden_states: [R, H]; top_k_index, top_k_weights: [R, k] as the
        block's router returns them (an index equal to num_experts is a dropped slot).  Inside `bnn.Model` with S samples in
        flight the rows are sample-major ([S*B*T, H]) and slab s meets the s-th draw; otherwise S = 1."""
        if bfr.STATE.ctx is None:
            again = bfr.recompute_context()
            if again is not None:  # a checkpointed block recomputed during backward: the forward's own epsilon
                with again.replay():
                    return self.forward(hidden_states, top_k_index, top_k_weights)
        ctx, base, S, slot = self._begin(hidden_states.device)
        x2 = hidden_states.reshape(-1, self.hidden_dim)
        if x2.shape[0] == 0:
            self.sample_weights(S, bfr.STATE.seed, base, slot, x2.dtype)
            self._end(ctx, slot)
            return torch.zeros_like(hidden_states)
        if x2.shape[0] % S:
            raise ValueError(f"Experts: input rows ({x2.shape[0]}) are not a multiple of the sample count S={S}")
        idx = top_k_index.reshape(x2.shape[0], -1)
        wts = top_k_weights.reshape(x2.shape[0], -1)
        params = (self.gate_up_proj.mu, self.gate_up_proj.rho, self.down_proj.mu, self.down_proj.rho)
        need_grad = torch.is_grad_enabled() and any(t.requires_grad for t in (x2, wts) + params)
        kept_w = None
        kept = ctx.kept if ctx is not None else None
        if kept is not None:
            kept_w = kept.experts_sample(self, S, bfr.STATE.seed, base, slot, x2.dtype)
        out = _ExpertsFn.apply(x2, wts, *params, idx, self, S, bfr.STATE.seed, base, slot, kept_w, need_grad)
        self._end(ctx, slot)
        return out.view(hidden_states.shape)

    @classmethod
    def from_frequentist(cls, experts: Module, initialization: Optional[Initialization] = DEFAULT_UNIFORM,
                         prior: Optional[Parameter] = DEFAULT_SCALED_GAUSSIAN_MIXTURE, delta: float = None,
                         freeze: bool = False) -> "Experts":
        """Bayesian experts from a framework experts module (`is_experts_module`), the arguments as bnn.Linear's: with `delta`
        (MOPED) mu <- the pretrained tensor (shares storage), rho <- log(exp(delta |w|) - 1), mu frozen if `freeze`, prior
        <- Gaussian(mu = w, rho = 1), for both tensors; without it mu and rho keep the initialization's draw.  As there,
        `initialization` is not forwarded to the constructor."""
        E, I2, H = experts.gate_up_proj.shape
        baye = cls(E, H, I2 // 2, experts.act_fn, prior=prior)
        if delta is not None:
            baye.gate_up_proj_prior = _moped(baye.gate_up_proj, experts.gate_up_proj, delta, freeze)
            baye.down_proj_prior = _moped(baye.down_proj, experts.down_proj, delta, freeze)
        return baye


def is_experts_module(module: Module) -> bool:
    """Does `module` look like transformers' gated experts (MixtralExperts, Qwen3MoeExperts, ...) by structure: 3-D
    parameters gate_up_proj [E, 2I, H] and down_proj [E, H, I], `num_experts` and `act_fn` attributes, and no other parameter
    of its own (gpt-oss's experts carry biases: left alone)."""
    if isinstance(module, Experts):
        return False
    own = dict(module.named_parameters(recurse=False))
    if set(own) != {"gate_up_proj", "down_proj"} or not hasattr(module, "num_experts") or not hasattr(module, "act_fn"):
        return False
    gu, d = own["gate_up_proj"], own["down_proj"]
    if gu.dim() != 3 or d.dim() != 3:
        return False
    E, I2, H = gu.shape
    return E == module.num_experts and I2 % 2 == 0 and tuple(d.shape) == (E, H, I2 // 2)
