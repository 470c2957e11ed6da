# -*- coding: utf-8 -*-
"""bayeformers_amd.nn.layers.lora

A frozen nn.Linear with a Bayesian low-rank adapter (the BLoB formulation: a Gaussian posterior on the LoRA A factor only,
a deterministic B factor), include/bayeformers_amd_lora.h:

    A_s  = mu_A + softplus(rho_A) * eps(seed, sample_base + s, stream 2 * layer_id, e)
    y[s] = x[s] W0^T + b0 + (alpha / r) * (x[s] A_s^T) B^T
    {log_prior, log_variational_posterior}[s] of A_s

The base product is ONE GEMM over all samples' rows (W0 is shared), the rank-r terms are bf_lora_fwd / bf_lora_bwd, A_s and
its log-probs come from bf_sample_logprob.  Not a bnn.Linear: the cross-layer sampling plan and the deferred gradient table
never see it.
"""
import math
from typing import Optional

import torch
import torch.nn as nn
from torch import Size, Tensor
from torch.nn import Module

from ... import ops
from ... import random as bfr
from ..parameters.base import Parameter
from ..parameters.gaussian import DEFAULT_SCALED_GAUSSIAN_MIXTURE, Gaussian
from ..parameters.initializations import DEFAULT_UNIFORM, Initialization
from .base import KernelLayer


class _LoRAFn(torch.autograd.Function):
    """Autograd node of LoRALinear.forward.  Backward = the reference's graph for a sampled factor: gradients through
    x W0^T + scale * (x A_s^T) B^T with A_s = mu + eps * softplus(rho), eps regenerated from the Philox counter and the
    log-prob scalars detached; nothing flows to W0."""

    @staticmethod
    def forward(ctx, x, mu, rho, b, layer, S, seed, base, lp_out, a_kept, need_grad):
        ctx.layer, ctx.S, ctx.seed, ctx.base = layer, S, seed, base
        ctx.counter = bfr.counter_snapshot(need_grad)
        if a_kept is not None:
            a_s = a_kept  # pinned_samples(keep_weights=...): the block's first forward drew it (and its log-probs)
        else:
            a_s = layer.sample_a(S, seed, base, lp_out, x.dtype)
        y, h = ops.lora_forward(x, a_s, b, layer.base_weight, layer.base_bias, layer.scale, S, layer._bias32())
        if need_grad:
            ctx.save_for_backward(x, a_s, h, b)
        return y

    @staticmethod
    def backward(ctx, grad):
        x, a_s, h, b = ctx.saved_tensors
        layer, S = ctx.layer, ctx.S
        need_x, need_mu, need_rho, need_b = ctx.needs_input_grad[:4]
        dx, da, db = ops.lora_backward(x, grad, a_s, b, h, layer.base_weight, layer.scale, S, need_x, need_b)
        dmu = drho = None
        if need_mu or need_rho:
            with bfr.counter_override(ctx.counter):
                dmu, drho = ops.lora_reduce_da(da, layer.lora_A, 2 * layer.layer_id, S, ctx.seed, ctx.base, need_mu)
        return dx, dmu, drho if need_rho else None, db, None, None, None, None, None, None, None


class LoRALinear(KernelLayer):
    """Frozen base projection with a Bayesian rank-r adapter.

    Attributes: in_features, out_features, r, alpha, scale = alpha / r; base_weight [N, K] and base_bias [N] or None (frozen,
    the model's dtype); lora_A (Gaussian [r, K], fp32 mu / rho) with lora_A_prior; lora_B (fp32 nn.Parameter [N, r], zero at
    construction, deterministic); log_prior, log_variational_posterior (of lora_A); layer_id, compute_dtype,
    log_prob_samples as bnn.Linear."""

    def __init__(self, in_features: int, out_features: int, r: int = 16, alpha: float = 32, bias: Optional[bool] = True,
                 initialization: Optional[Initialization] = DEFAULT_UNIFORM,
                 prior: Optional[Parameter] = DEFAULT_SCALED_GAUSSIAN_MIXTURE) -> None:
        super(LoRALinear, self).__init__()
        if isinstance(r, bool) or not isinstance(r, int) or r < 1:
            raise ValueError(f"LoRALinear: r={r!r} (a positive int)")
        self.in_features, self.out_features = in_features, out_features
        self.r, self.alpha, self.scale = r, alpha, float(alpha) / r
        self.initialization = initialization

        self.base_weight = nn.Parameter(torch.zeros(out_features, in_features), requires_grad=False)
        if bias:
            self.base_bias = nn.Parameter(torch.zeros(out_features), requires_grad=False)
        else:
            self.register_parameter("base_bias", None)
        # rho from the initialization's range; mu as nn.Linear and PEFT initialise the A factor
        self.lora_A = Gaussian(Size((r, in_features)), self.initialization)
        with torch.no_grad():
            nn.init.kaiming_uniform_(self.lora_A.mu, a=math.sqrt(5))
        self.lora_A_prior = prior
        self.lora_B = nn.Parameter(torch.zeros(out_features, r, dtype=torch.float32))
        self._init_kernel_layer()
        self._b32 = None

    def extra_repr(self) -> str:
        return (f"in_features={self.in_features}, out_features={self.out_features}, r={self.r}, alpha={self.alpha}, "
                f"bias={self.base_bias is not None}")

    def _apply(self, fn, recurse=True):
        """`.to(torch.bfloat16)` / `.half()` change the frozen base's precision, never lora_B's: it is an fp32 master like
        mu and rho (the kernels round it in registers)."""
        master = self._parameters.get("lora_B")

        def keep_master(t):
            moved = fn(t)
            if master is not None and (t is master or t is master.grad) and moved.dtype != t.dtype:
                moved = t.to(device=moved.device)
            return moved

        return super(LoRALinear, self)._apply(keep_master, recurse)

    def gaussians(self):
        yield self.lora_A, self.lora_A_prior, 2 * self.layer_id

    def _bias32(self) -> Optional[Tensor]:
        """The base bias as the GEMM epilogue reads it ([1, N] fp32), converted once per state of the parameter."""
        b0 = self.base_bias
        if b0 is None:
            return None
        key = (b0.data_ptr(), b0._version, b0.device)
        if self._b32 is None or self._b32[0] != key:
            with torch.inference_mode(False), torch.no_grad():
                self._b32 = (key, b0.detach().float().view(1, -1).clone())
        return self._b32[1]

    def sample_a(self, S: int, seed: int, base: int, lp_out: Optional[Tensor], x_dtype: torch.dtype) -> Tensor:
        """A_s [S, r, K] in the compute dtype (16-bit) or fp32, with {log_prior, log_q} per sample into lp_out."""
        cdt = self.compute_dtype or bfr.get_compute_dtype()
        adt = cdt if (cdt != torch.float32 and x_dtype == cdt) else torch.float32
        (a_s,), lp = ops.sample_logprob([self.lora_A], [self.lora_A_prior], [2 * self.layer_id], S, seed, base, out_dtype=adt)
        if lp_out is not None:
            lp_out.copy_(lp)
        return a_s

    def forward(self, input: Tensor) -> Tensor:
        """y = x W0^T + b0 + scale * (x A_s^T) B^T with A ~ N(mu_A, softplus(rho_A)).  Inside `bnn.Model` with S samples in
        flight the input is [S*B, ..., in_features] (sample-major) and slab s meets A_s; otherwise S = 1."""
        if bfr.STATE.ctx is None:
            again = bfr.recompute_context()
            if again is not None:  # a checkpointed block recomputed during backward: the forward's own epsilon
                with again.replay():
                    return self.forward(input)
        ctx, base, S, slot = self._begin(input.device)
        x2 = input.reshape(-1, self.in_features)
        if x2.shape[0] == 0:
            self.sample_a(S, bfr.STATE.seed, base, slot, x2.dtype)
            self._end(ctx, slot)
            return input.new_empty(*input.shape[:-1], self.out_features)
        if x2.shape[0] % S:
            raise ValueError(f"LoRALinear: input rows ({x2.shape[0]}) are not a multiple of the sample count S={S}")
        need_grad = torch.is_grad_enabled() and any(
            t.requires_grad for t in (x2, self.lora_A.mu, self.lora_A.rho, self.lora_B))
        a_kept = None
        kept = ctx.kept if ctx is not None else None
        if kept is not None:
            a_kept = kept.lora_sample(self, S, bfr.STATE.seed, base, slot, x2.dtype)
        y = _LoRAFn.apply(x2, self.lora_A.mu, self.lora_A.rho, self.lora_B, self, S, bfr.STATE.seed, base, slot, a_kept,
                          need_grad)
        self._end(ctx, slot)
        return y.view(*input.shape[:-1], self.out_features)

    @classmethod
    def from_frequentist(cls, linear: Module, r: int = 16, alpha: float = 32,
                         initialization: Optional[Initialization] = DEFAULT_UNIFORM,
                         prior: Optional[Parameter] = DEFAULT_SCALED_GAUSSIAN_MIXTURE) -> "LoRALinear":
        """Adapter on a pretrained nn.Linear: the base takes over its weight and bias (shared storage, frozen), B = 0, so the
        converted layer computes the pretrained function until it is trained."""
        layer = cls(linear.in_features, linear.out_features, r, alpha, linear.bias is not None, initialization, prior)
        layer.base_weight.data = linear.weight.data
        if linear.bias is not None:
            layer.base_bias.data = linear.bias.data
        dev = linear.weight.device
        if dev.type != "cpu":
            layer.lora_A.to(dev)
            layer.lora_B.data = layer.lora_B.data.to(dev)
        return layer
