# -*- coding: utf-8 -*-
"""bayeformers_amd.nn.model

Wrapper that turns any module containing Bayesian children into a Bayesian model — same surface as
/root/reference/bayeformers/nn/model.py (is_module_bayesian :16-28, Model :31-89).

Additions for the MI355X path (all optional; with S = 1 the behaviour is the reference's):
  * `with model.monte_carlo(S): out = model(**inputs_repeated_S_times)` runs S Monte-Carlo samples in ONE forward:
    every bnn.Linear sees [S*B, ...] (sample-major), multiplies slab s by W_s and leaves per-sample log-probs;
  * the per-layer {log_prior, log_q} land in one [L, S, 2] float64 buffer, so `log_prior()` is one reduction
    instead of 74 scalar adds; `log_prior_samples()` / `log_variational_posterior_samples()` return the [S] values;
  * all layers of one forward share the same reserved Monte-Carlo sample indices (bayeformers_amd.random).
"""
import contextlib
import itertools
import warnings
from typing import Any, Iterator, List, Optional, Union

import torch
from torch import Tensor
from torch.nn import Module

from .. import ops
from .. import random as bfr
from ..graphs import GraphCache, auto_forward
from ..plan import SamplePlan
from .layers.base import KernelLayer
from .layers.linear import Linear


def is_module_bayesian(module: Module) -> bool:
    """A module is Bayesian if it exposes log_prior and log_variational_posterior (model.py:16-28)."""
    log_prior = hasattr(module, "log_prior")
    log_variational_posterior = hasattr(module, "log_variational_posterior")
    return log_prior and log_variational_posterior


_TOKENS = itertools.count(1)


class _ForwardContext:
    """What the Bayesian layers of one Model.forward share: the reserved sample indices, their log-prob slots and
    (when every layer is plannable) the cross-layer sampling plan."""

    def __init__(self, sample_base: int, S: int, slots: dict, plan=None, lp_buf=None, shard_start: int = 0, dropping: bool = True,
                 drop_sites=None):
        self.sample_base, self.S, self._slots = sample_base, S, slots
        self.plan, self.lp_buf = plan, lp_buf
        self.token = next(_TOKENS)
        self.shared_out = {}  # id(first layer of a stacked run) -> (input identity, [L, S, M, N] outputs)
        # device-counter mode: the counter value this forward's kernels added — what `replay` needs, i.e. only a forward
        # that records gradients (the copy is a kernel launch)
        self.counter = bfr.counter_snapshot(torch.is_grad_enabled())
        if self.counter is not None:  # ... and the layers' autograd nodes share it (counter_snapshot's per-forward cache)
            self._counter_snap = (bfr.STATE.device_counter, bfr.STATE.counter_moves, self.counter)
        self.graph_tasks = set()  # ids of the backward passes that reached this forward's outputs (bfr.remember_context)
        # the `call` of every dropout applied inside this forward; `shard_start` (the first global sample of this process's
        # shard within the step) is where the kernels start numbering their dropout groups (ops.Dropout.first_group): a
        # sample's masks are a function of its GLOBAL index, so S-sharded training draws the single-process masks
        self.drop_call = bfr.reserve_dropout_call()
        self.drop_counter = bfr.reserve_dropout_counter(needed=dropping)  # device-counter mode: this forward's copy of it
        self.shard_start = int(shard_start)
        self.drop_sites = drop_sites  # the owning model's [next free dropout site number] (random.dropout_site)
        self.kept = None  # the _KeptWeights of a pinned_samples(keep_weights=True) block (then plan = its plan)

    @contextlib.contextmanager
    def replay(self):
        """Run layer forwards again under this (finished) forward's sample indices: the recomputation of a checkpointed
        block during backward (bayeformers_amd.random.recompute_context).  Sampled weights still resident in the plan's
        arenas are reused; overwritten ones are drawn again from the same counters."""
        prev = bfr.STATE.ctx
        bfr.STATE.ctx = self
        self._replaying = True
        try:
            with bfr.counter_override(self.counter):
                yield self
        finally:
            self._replaying = False
            bfr.STATE.ctx = prev
            if self.plan is not None and prev is None:
                self.plan.pending.clear()  # the log-probs of these samples were reduced when the forward ended

    def slot(self, layer) -> Optional[Tensor]:
        return self._slots.get(id(layer))


class _KeptWeights:
    """The sampled weights of a `pinned_samples(keep_weights=True)` block: every bnn.Linear of the model in ONE SamplePlan with
    one arena per group (plan.SamplePlan keep=True), sampled by one launch in the block's first forward and read by every
    later one.  Belongs to the block: Model._plan and its rebuilds never see it."""

    mode = "keep_weights=True"
    fp8 = False

    def __init__(self, S: int, cdt: torch.dtype):
        self.S, self.cdt = S, cdt
        self.plan: Optional[SamplePlan] = None
        self.watch = []  # (tensor, data_ptr, _version) of every mu / rho the samples were drawn from
        self.ready = False  # the block's first forward has run prepare()
        self.lora = {}  # id(bnn.LoRALinear) -> its 16-bit A_s [S, r, K], drawn by the layer's first forward of the block
        self.experts = {}  # id(bnn.Experts) -> its two draws ([S, E, 2I, H], [S, E, H, I]), likewise

    def prepare(self, model, layers, ctx) -> SamplePlan:
        """The plan of the block; in its first forward also the one sampling launch over all groups."""
        S, cdt = ctx.S, bfr.get_compute_dtype()
        if (S, cdt) != (self.S, self.cdt):
            raise RuntimeError(f"pinned_samples({self.mode}): entered for S={self.S} at {self.cdt}, a forward runs "
                               f"with S={S} at {cdt}")
        if torch.is_grad_enabled() or model.training:
            raise RuntimeError(f"pinned_samples({self.mode}): forwards inside must run in eval mode without gradients")
        if self.ready:
            for t, ptr, ver in self.watch:
                if t.data_ptr() != ptr or t._version != ver:
                    raise RuntimeError(f"pinned_samples({self.mode}): a posterior mu / rho changed inside the block; "
                                       "the kept samples no longer match it (leave the block to draw new ones)")
            return self.plan
        linears = [(i, l) for i, l in enumerate(layers) if isinstance(l, Linear)]
        pl = [l for _, l in linears]
        shared = tuple(sorted({id(l._shared_input): l._shared_input for l in pl
                               if l._shared_input is not None}.values(), key=lambda t: t[0].layer_id))
        self.ready = True
        if not pl:  # only LoRA / Experts layers are Bayesian: nothing to plan, each keeps its own draws (lora_sample, ...)
            return None
        self.plan = self._draw(pl, [i for i, _ in linears], shared, ctx)
        from .parameters.gaussian import Gaussian

        for l in pl:
            for g in (l.weight, l.bias):
                if isinstance(g, Gaussian):
                    self.watch += [(t, t.data_ptr(), t._version) for t in (g.mu, g.rho)]
        return self.plan

    def lora_sample(self, layer, S: int, seed: int, base: int, slot: Tensor, x_dtype: torch.dtype) -> Tensor:
        """The kept A_s of a bnn.LoRALinear: drawn (with its log-probs, into `slot`) at the layer's first forward of the block,
        read by every later one.  Always the 16-bit (or fp32-compute) draw, never FP8: the tensor is tiny."""
        a_s = self.lora.get(id(layer))
        if a_s is None:
            a_s = self.lora[id(layer)] = layer.sample_a(S, seed, base, slot, x_dtype)
            self.watch += [(t, t.data_ptr(), t._version) for t in (layer.lora_A.mu, layer.lora_A.rho)]
        return a_s

    def experts_sample(self, layer, S: int, seed: int, base: int, slot: Tensor, x_dtype: torch.dtype):
        """The kept draws of a bnn.Experts: both tensors drawn by one launch (with their log-probs, into `slot`) at the layer's
        first forward of the block, read by every later one.  Always the 16-bit (or fp32-compute) draws, never FP8."""
        w = self.experts.get(id(layer))
        if w is None:
            w = self.experts[id(layer)] = layer.sample_weights(S, seed, base, slot, x_dtype)
            self.watch += [(t, t.data_ptr(), t._version) for g in (layer.gate_up_proj, layer.down_proj) for t in (g.mu, g.rho)]
        return w

    def _draw(self, pl, index, shared, ctx) -> SamplePlan:
        plan = SamplePlan(pl, self.S, self.cdt, pl[0].weight.mu.device, index=index, shared=shared, keep=True)
        plan._sample_groups(0, len(plan.groups) - 1, ctx.token, bfr.STATE.seed, ctx.sample_base)
        return plan


class _KeptFp8Weights(_KeptWeights):
    """The sampled weights of a `pinned_samples(keep_weights="fp8")` block as centred FP8 rows
    (include/bayeformers_amd_fp8.h): per layer one bf16 copy of the posterior mean shared by the S samples, and per sample
    the draw's deviation from it in e4m3 with a power-of-two scale per output row (and the fp32 biases as they are).  The
    plan is an ordinary ring plan: the block's first forward samples it a ringful of groups at a time and quantises each
    into the store, so the 16-bit draws never exist all at once; later the ring only holds the dequantised weights W^ of
    the groups whose layers run a GEMM that reads 16-bit weights."""
    mode = 'keep_weights="fp8"'
    fp8 = True

    def __init__(self, S: int, cdt: torch.dtype):
        super().__init__(S, cdt)
        self.store = {}     # id(layer) -> (center [N, K] bf16, q [S, N, K] uint8, scale [S, N] fp32, bias [S, N] fp32 or None)
        self.resident = []  # per ring arena: the group whose W^ (and biases) it holds

    def _draw(self, pl, index, shared, ctx) -> SamplePlan:
        S, dev = self.S, pl[0].weight.mu.device
        plan = SamplePlan(pl, S, self.cdt, dev, index=index, shared=shared)
        for l in pl:
            N, K = l.out_features, l.in_features
            _, b_s = plan.views[id(l)]
            self.store[id(l)] = (l.weight.mu.detach().to(torch.bfloat16, copy=True).contiguous(),  # (a copy even of a bf16 mu)
                                 torch.empty((S, N, K), dtype=torch.uint8, device=dev),
                                 torch.empty((S, N), dtype=torch.float32, device=dev),
                                 torch.empty((S, N), dtype=torch.float32, device=dev) if b_s is not None else None)
        ring, first = len(plan.arenas), 0
        while first < len(plan.groups):  # everything runs on one stream: a launch overwrites an arena after its quantisation
            last = min(len(plan.groups), first + ring) - 1
            plan._sample_groups(first, last, ctx.token, bfr.STATE.seed, ctx.sample_base)
            for gi in range(first, last + 1):
                for l in plan.groups[gi]:
                    center, q, scale, bias = self.store[id(l)]
                    w_s, b_s = plan.views[id(l)]
                    ops.quantize_rows_fp8(w_s, center, q, scale)
                    if bias is not None:
                        bias.copy_(b_s)
            first = last + 1
        # the arenas hold unrounded draws now: no layer may read them as they are
        plan.arena_owner = [None] * ring
        self.resident = [None] * ring
        return plan

    def store_bytes(self) -> int:
        return sum(t.numel() * t.element_size() for entry in self.store.values() for t in entry if t is not None)

    def weights16(self, layer):
        """(W^ [S, N, K] bf16, bias) of `layer` in the ring: its group is dequantised unless the arena still holds it."""
        plan = self.plan
        gi = plan.group_of[id(layer)]
        slot = gi % len(plan.arenas)
        if self.resident[slot] != gi:
            for l in plan.groups[gi]:
                center, q, scale, bias = self.store[id(l)]
                w_s, b_s = plan.views[id(l)]
                ops.dequantize_rows_fp8(q, scale, center, out=w_s)
                if bias is not None:
                    b_s.copy_(bias)
            self.resident[slot] = gi
        return plan.views[id(layer)]


class _MeanForward:
    """What the bnn.Linear layers of a forward inside `Model.posterior_mean()` share: the model, and through it the centre
    copies of an enclosing pinned_samples(keep_weights="fp8") block."""

    def __init__(self, model: "Model"):
        self.model = model

    def center(self, layer, cdt: torch.dtype) -> Optional[Tensor]:
        """The bf16 posterior mean [N, K] the enclosing keep_weights="fp8" block holds for `layer`, once its first forward
        has made it; None otherwise (the layer then keeps a copy of its own)."""
        kept = self.model.__dict__.get("_kept")
        if kept is None or not kept.fp8 or not kept.ready or cdt != torch.bfloat16:
            return None
        entry = kept.store.get(id(layer))
        return entry[0] if entry is not None else None


class _KLFn(torch.autograd.Function):
    """[S, 2] per-sample {log_prior, log_q} of the model as a differentiable function of every layer's mu and rho
    (opt-in, bayeformers_amd.set_kl_gradient).  Backward = one bf_kl_grad launch per parameter tensor."""

    @staticmethod
    def forward(ctx, lp, model, S, seed, base, counter, *params):
        ctx.model, ctx.S, ctx.seed, ctx.base, ctx.counter = model, S, seed, base, counter
        return lp.clone()

    @staticmethod
    def backward(ctx, g):
        from .. import ops

        g = g.to(torch.float64).contiguous()
        grads = []
        with bfr.counter_override(ctx.counter):
            for layer in ctx.model.fused_children():
                for gauss, prior, sid in layer.gaussians():
                    dmu, drho = ops.kl_grad(gauss, prior, sid, ctx.S, ctx.seed, ctx.base, g, gauss.mu.requires_grad)
                    grads += [dmu, drho if gauss.rho.requires_grad else None]
        return (None, None, None, None, None, None) + tuple(grads)


class Model(Module):
    """Wrapper gathering log_prior and log_variational_posterior from Bayesian children.

    Attributes:
        model (Optional[nn.Module]): wrapped module (None when subclassed with its own forward)
    """

    def __init__(self, model: Optional[Module] = None) -> None:
        super(Model, self).__init__()
        self.model = model
        self._mc_samples = 1
        self._mc_span = (0, 1)  # (first global sample index of this process, indices every step consumes)
        self._fused: Optional[List[KernelLayer]] = None
        self._lp_buf: Optional[Tensor] = None
        self._last_base = None
        self._plan: Optional[SamplePlan] = None
        self.cross_layer_sampling = True  # one sampling launch per ~96 MB group of layers instead of one per layer
        # evaluation forwards (eval mode, no_grad, one sample per call: the reference's own caller loop,
        # /root/reference/examples/bert_glue.py:63-66) are replayed from a HIP graph from their third call on (graphs.py)
        self.graph_replay = True
        self._graphs = GraphCache()

    # ------------------------------------------------------------------------------------------ forward
    def forward(self, *args, **kwargs) -> Any:
        """Forward of the wrapped module (model.py:53-57)."""
        if self.model is not None:
            return self.model.forward(*args, **kwargs)
        raise NotImplementedError("Forward pass not implemented yet")

    def __call__(self, *args, **kwargs):
        if bfr.STATE.ctx is not None:  # nested bnn.Model: the outer forward owns the sample indices
            return super(Model, self).__call__(*args, **kwargs)
        if bfr.STATE.mean is not None:  # posterior_mean(): no sample indices, no log-prob slots, no plan, no replay
            return super(Model, self).__call__(*args, **kwargs)
        out = auto_forward(self, args, kwargs)  # an evaluation forward seen before: replayed from its HIP graph
        if out is not None:
            return out
        return self._eager_call(*args, **kwargs)

    def train(self, mode: bool = True):
        cache = self.__dict__.get("_graphs")
        if cache is not None:
            cache.refused.clear()  # signatures that were kept eager because of a child in training mode get another look
        return super(Model, self).train(mode)

    def _eager_call(self, *args, **kwargs):
        S = self._mc_samples
        layers = self.fused_children()
        if layers:
            # a kernel of an earlier forward may have found a prior's baked constants different from the tensors they were read
            # from (an in-place edit through .data: no version counter moved).  That forward's log-prior is NaN; from this
            # one on every cached copy is dropped and the priors are described again.
            ops.refresh_stale_epoch()
        ops._COLSUM_OFFERS.clear()  # (column sums a backward pass offered and nobody took)
        slots = {}
        if layers:
            dev = next(layers[0].gaussians())[0].mu.device
            buf = self._lp_buf
            if buf is None or buf.shape[0] != len(layers) or buf.shape[1] != S or buf.device != dev:
                with torch.inference_mode(False):  # (kept across forwards, written in place by forwards of any mode)
                    buf = self._lp_buf = torch.zeros((len(layers), S, 2), dtype=torch.float64, device=dev)
            slots = {id(l): buf[i] for i, l in enumerate(layers)}
        plan = None
        # (a layer under local reparameterisation draws no weights: it is never in the sampling plan)
        linears = [l for l in layers if isinstance(l, Linear) and not l.local]
        kept = self.__dict__.get("_kept")
        if kept is not None:
            pass  # the block's own plan (below, once the forward's context exists); Model._plan is left as it is
        elif linears and self.cross_layer_sampling and SamplePlan.plannable(linears):
            # layers seen with <= 64 rows per sample run the single fused kernel instead (Linear.forward marks them)
            planned = [(i, l) for i, l in enumerate(layers) if isinstance(l, Linear) and not l._small_m and not l.local]
            if planned:
                cdt = bfr.get_compute_dtype()
                pl = [l for _, l in planned]
                shared = tuple(sorted({id(l._shared_input): l._shared_input for l in pl
                                       if l._shared_input is not None}.values(), key=lambda t: t[0].layer_id))
                key = SamplePlan.make_key(pl, S, cdt, shared)
                if (self._plan is None or self._plan.key != key or not self._plan.alias_valid()
                        or self._plan.epoch != bfr.STATE.stale_epoch):
                    self._plan = SamplePlan(pl, S, cdt, pl[0].weight.mu.device, index=[i for i, _ in planned],
                                            shared=shared)
                plan = self._plan
        if plan is None and kept is None:
            self._plan = None  # (a plan of an earlier forward that no layer would use now: its arenas are released)
        # every rank reserves the GLOBAL sample indices of the step and runs its own contiguous slice of them; inside
        # pinned_samples() every forward runs on the one reservation made when it was entered
        start, total = self._mc_span
        pinned = self.__dict__.get("_pinned")
        if pinned is not None and (pinned[1], pinned[2]) != (start, total):
            raise RuntimeError(f"pinned_samples: entered for sample span {pinned[1:]}, a forward runs with {(start, total)}")
        base = pinned[0] + start if pinned is not None else bfr.reserve_samples(total) + start
        self._last_base, self._last_seed, self._last_S = base, bfr.STATE.seed, S
        self._last_counter = bfr.counter_snapshot() if bfr.STATE.kl_gradient else None
        ctx = bfr.STATE.ctx = _ForwardContext(base, S, slots, plan, self._lp_buf, shard_start=start, dropping=self.training,
                                              drop_sites=self.__dict__.setdefault("_drop_sites", [1]))
        out = None
        try:
            if kept is not None:
                ctx.kept, ctx.plan = kept, kept.prepare(self, layers, ctx)
                plan = ctx.plan
            out = super(Model, self).__call__(*args, **kwargs)
            return out
        finally:
            if plan is not None:
                plan.finish(self._lp_buf)  # one log-prob reduction for all the groups this forward sampled
            if pinned is not None and self._lp_buf is not None:
                # the same indices draw the same weights: the log-probs of the block's first forward stand for all of them
                # (a later forward may reduce them on another kernel, in another summation order)
                kept = self.__dict__.get("_pinned_lp")
                if kept is None or kept.shape != self._lp_buf.shape:
                    with torch.inference_mode(False):
                        self._pinned_lp = self._lp_buf.clone()
                else:
                    self._lp_buf.copy_(kept)
            bfr.STATE.ctx = None
            # what a finished forward keeps is what a checkpointed block's recomputation needs (sample indices, slots,
            # plan, counter): NOT the stacked query/key/value outputs and their inputs — a replay re-keys on data_ptr and
            # computes them again anyway, and holding them would pin ~3 GB of a BERT-base step until the next forward
            ctx.shared_out = {}
            if torch.is_grad_enabled() and out is not None:
                bfr.remember_context(ctx, out)
            if pinned is None:
                bfr.commit_samples(total)

    @contextlib.contextmanager
    def monte_carlo(self, samples: int, shard=(0, 1), span=None):
        """Run forwards with `samples` Monte-Carlo samples folded into the batch axis (inputs repeated S times,
        sample-major: `x.repeat(S, 1, ...)`).  shard = (rank, world): this process runs `samples` of the
        `samples * world` global sample indices of each step (S-sharding over GPUs, sampling.sample_bayesian).
        span = (start, total) says it directly — this process runs the global indices [start, start + samples) of the
        `total` every step consumes — for shards of unequal size (S = 10 over 8 GPUs: sampling.shard_span)."""
        prev = (self._mc_samples, self._mc_span)
        S = int(samples)
        if span is None:
            span = (int(shard[0]) * S, S * int(shard[1]))
        start, total = int(span[0]), int(span[1])
        if S < 1 or start < 0 or start + S > total:
            raise ValueError(f"monte_carlo: samples={S} at offset {start} do not fit in the step's {total} sample indices")
        self._mc_samples, self._mc_span = S, (start, total)
        self._mc_harness = getattr(self, "_mc_harness", 0) + 1  # (inside a harness: no transparent graph replay, graphs.py)
        try:
            yield self
        finally:
            self._mc_samples, self._mc_span = prev
            self._mc_harness -= 1

    @contextlib.contextmanager
    def pinned_samples(self, keep_weights: Union[bool, str] = False, max_bytes: Optional[int] = None):
        """Run every forward inside on ONE reservation of Monte-Carlo sample indices: reserved when the block is entered
        (for the span of the `monte_carlo` setting in force then), committed once when it is left.  Each of the S samples
        is then one fixed draw of the weights across the forwards — e.g. the steps of a generation that reuse a KV cache
        — and log_prob_samples() is the same after every forward.  Works with the host counter and with the
        device-resident one (use_device_counter: the kernels add the counter, which moves once at the end).  Forwards
        inside are never replayed from a HIP graph.  Outside the block each forward reserves fresh indices, as always.

        keep_weights=True (eval mode, no gradient): the block's first forward samples the S weight draws of EVERY bnn.Linear in
        one launch and keeps them in device memory until the block is left; later forwards sample nothing.  Their layers with at
        most ops.SKINNY_ROWS rows per sample (decode steps) run bf_gemm_nt_skinny on the kept 16-bit weights, the others the
        tiled GEMM (fp32 compute: the fp32 GEMM).  The draws and log-probs are the bits the cross-layer plan gives.  Costs
        plan.kept_weight_bytes(model, S, compute dtype) bytes — S * P * 2 in bf16 for P Linear weights — checked before
        anything is allocated against max_bytes (default plan.ARENA_BYTES): above it, ValueError.  A forward after a
        posterior mu / rho was changed inside the block raises.  bnn.Embedding layers keep their own path.  A bnn.LoRALinear
        keeps its A_s and a bnn.Experts its two weight draws, each drawn at the layer's first forward of the block (the
        bf_moe_* kernels of later forwards read them: a decode step with experts samples nothing).

        keep_weights="fp8" (bf16 compute only): the same block on fewer bytes.  One bf16 copy of each layer's posterior mean is
        kept for all samples, and of each draw only its deviation from that mean, in e4m3 with a power-of-two scale per output
        row (include/bayeformers_amd_fp8.h) — plan.kept_weight_bytes(model, S, bfloat16, fp8=True) bytes, about (2 + S) * P
        instead of 2 * S * P, plus a transient 16-bit ring of at most plan.ARENA_BYTES.  Every forward of the block, prefill and
        decode alike, multiplies by the dequantised weights W^, which differ from the bf16 draws by 2^-4 of the DEVIATION (0.3 %
        of |mu| at MOPED delta = 0.05), not of the weight.  Decode steps run bf_gemm_nt_skinny_fp8 on the bytes; the other
        GEMMs read W^ dequantised into the ring.  log_prob_samples() is that of the unrounded draws, bitwise keep_weights=True's.
        A model with bnn.Experts layers is refused (ValueError naming them): their kept draws have no FP8 form."""
        if self.__dict__.get("_pinned") is not None:
            raise RuntimeError("pinned_samples: already pinned")
        if keep_weights != "fp8" and (isinstance(keep_weights, str) or keep_weights not in (True, False)):
            raise ValueError(f"pinned_samples: keep_weights={keep_weights!r} (False, True or \"fp8\")")
        kept = None
        if keep_weights:
            kept = self._keep_weights_check(max_bytes, fp8=keep_weights == "fp8")
        elif max_bytes is not None:
            raise ValueError("pinned_samples: max_bytes is the budget of keep_weights=True")
        start, total = self._mc_span
        self._pinned = (bfr.reserve_samples(total), start, total)
        self._pinned_lp = None
        self._kept = kept
        try:
            yield self
        finally:
            self._pinned = self._pinned_lp = self._kept = None  # (the kept samples' arenas go with the last reference)
            bfr.commit_samples(total)

    @contextlib.contextmanager
    def posterior_mean(self):
        """Run every forward inside on the posterior MEAN of the weights: each bnn.Linear computes x mu_w^T + mu_b and draws
        nothing.  The input is ONE row block — [B, ...], not the [S*B, ...] of `monte_carlo(S)` — and the forward reserves
        no sample index, writes no log-probs (log_prob_samples() stays the last sampled forward's) and is never replayed
        from a HIP graph.  It nests inside `monte_carlo` / `pinned_samples` (keep_weights in any form) and leaves the
        pinned draws, the kept weights and the sample counter as they are: the sampled forward after it is bitwise what it
        would have been.  That is the draft model of sample_generate(speculative=...): the same network at 1/S of the weight
        traffic.

        Each layer multiplies a copy of mu_w in the compute dtype, made at its first mean forward and kept on the layer
        (Linear.mean_weights; dropped by a new mu, a later stale epoch or ops.invalidate_caches): plan.mean_weight_bytes(model,
        dtype) bytes, P * 2 in bf16 against the S * P * 2 of keep_weights=True.  Inside keep_weights="fp8" the block's own
        centre copies are read and nothing is added.  At most ops.SKINNY_ROWS rows run bf_gemm_nt_skinny with S = 1, more
        rows the tiled GEMM.  Inference only (no gradient); a model with a bnn.Embedding, a bnn.LoRALinear or a bnn.Experts,
        which have no mean form yet, is refused (ValueError naming the layer types)."""
        if bfr.STATE.ctx is not None:
            raise RuntimeError("posterior_mean: entered inside a running forward")
        if torch.is_grad_enabled():
            raise RuntimeError("posterior_mean is inference only: enter it under torch.no_grad()")
        other = sorted({type(l).__name__ for l in self.fused_children() if not isinstance(l, Linear)})
        if other:
            raise ValueError(f"posterior_mean: the model has {', '.join(other)} layers, which have no posterior-mean "
                             "forward (bnn.Linear only)")
        prev = bfr.STATE.mean
        bfr.STATE.mean = _MeanForward(self)
        try:
            yield self
        finally:
            bfr.STATE.mean = prev

    def _keep_weights_check(self, max_bytes: Optional[int], fp8: bool = False) -> "_KeptWeights":
        """Everything pinned_samples(keep_weights=True or "fp8") refuses, checked before anything is reserved or allocated."""
        from .. import plan as bplan

        mode = _KeptFp8Weights.mode if fp8 else _KeptWeights.mode
        if any(isinstance(l, Linear) and l.local for l in self.fused_children()):
            raise ValueError(f"pinned_samples({mode}) keeps one weight draw per sample; this model runs local "
                             "reparameterisation (local_reparameterization), which has no weight draw — switch it off first")
        if torch.is_grad_enabled():
            raise RuntimeError(f"pinned_samples({mode}) is inference only: enter it under torch.no_grad()")
        if self.training:
            raise RuntimeError(f"pinned_samples({mode}) is inference only: put the model in eval mode (model.eval())")
        S, cdt = self._mc_samples, bfr.get_compute_dtype()
        if fp8 and cdt != torch.bfloat16:
            raise ValueError(f"pinned_samples({mode}) needs bfloat16 compute (set_compute_dtype): at {cdt} the dequantised "
                             "weights are not the exact bf16 values the format defines")
        limit = bplan.ARENA_BYTES if max_bytes is None else int(max_bytes)
        need = bplan.kept_weight_bytes(self, S, cdt, fp8=fp8)
        if need > limit:
            raise ValueError(f"pinned_samples({mode}): the kept samples need {need} bytes (S={S}, {cdt}), "
                             f"above max_bytes={limit}")
        from .layers.experts import Experts
        from .layers.lora import LoRALinear

        if fp8 and any(isinstance(l, Experts) for l in self.fused_children()):
            raise ValueError(f"pinned_samples({mode}): the model has Experts layers, whose kept draws have no FP8 form "
                             "(bnn.Linear only) — use keep_weights=True")
        linears = [l for l in self.fused_children() if isinstance(l, Linear)]
        if not linears and not any(isinstance(l, (LoRALinear, Experts)) for l in self.fused_children()):
            raise ValueError(f"pinned_samples({mode}): the model has no Bayesian Linear layer")
        if linears and not SamplePlan.plannable(linears):
            raise ValueError(f"pinned_samples({mode}) needs every Bayesian Linear on one ROCm device, with built-in "
                             "priors and the global compute dtype (SamplePlan.plannable)")
        return (_KeptFp8Weights if fp8 else _KeptWeights)(S, cdt)

    def fused_children(self) -> List[KernelLayer]:
        """The kernel-backed children (bnn.Linear, bnn.Embedding, bnn.LoRALinear, bnn.Experts) in registration order; their
        layer_id (Philox stream) is that order, with the bnn.Experts layers numbered after all the others."""
        if self._fused is None:
            self._fused = [m for m in self.modules() if isinstance(m, KernelLayer)]
            # bnn.Experts layers (to_bayesian(experts=True)) are numbered after all the others: every other layer keeps the
            # stream, and so the draws, it has in the conversion without them
            from .layers.experts import Experts

            order = [l for l in self._fused if not isinstance(l, Experts)] + [l for l in self._fused if isinstance(l, Experts)]
            for i, l in enumerate(order):
                l.layer_id = i
        return self._fused

    def refresh(self) -> None:
        """Re-scan the children after the module tree was edited."""
        self._fused, self._lp_buf, self._plan = None, None, None
        self.__dict__.pop("_children_kept", None)
        cache = self.__dict__.get("_graphs")
        if cache is not None:
            cache.close()  # captured forwards hold the old layers' buffers

    # ------------------------------------------------------------------------------------------ log-probs
    @property
    def bayesian_children(self) -> Iterator[Module]:
        """All Bayesian children (duck-typed, model.py:59-68)."""
        children = filter(is_module_bayesian, self.modules())
        children = [c for c in children if c != self]
        return children

    def _only_fused(self) -> bool:
        return self._children()[1]

    def _children(self):
        """(Bayesian children, all of them kernel-backed?) — walked once and kept: the walk over a converted BERT-base's ~600
        modules is 1.5 ms, and the reference's caller loop asks twice per sample (log_prior(), log_variational_posterior():
        /root/reference/examples/bert_glue.py:65-66).  Like `fused_children()` the result stands until `refresh()`; a kept
        child that is no longer registered where it was found (a layer swapped out) makes it stale at once."""
        kept = self.__dict__.get("_children_kept")
        if kept is not None and all(parent._modules.get(name) is child for parent, name, child in kept[2]):
            return kept[0], kept[1]
        children = list(self.bayesian_children)
        where = []
        wanted = {id(c) for c in children}
        for parent in self.modules():
            for name, child in parent._modules.items():
                if id(child) in wanted:
                    where.append((parent, name, child))
        only = all(isinstance(c, KernelLayer) for c in children)
        self.__dict__["_children_kept"] = (children, only, where)
        return children, only

    def _sum(self, index: int, name: str):
        children, only_fused = self._children()
        if not len(children):
            warnings.warn("No Bayesian Child is present in this model")
        if len(children) and self._lp_buf is not None and only_fused:
            # one reduction over the [L, S, 2] buffer the kernels wrote: sum over layers, mean over samples
            if bfr.STATE.kl_gradient and torch.is_grad_enabled():
                return self.log_prob_samples()[:, index].mean().to(torch.float32)
            return self._lp_buf[:, :, index].sum(0).mean().to(torch.float32)
        value = 0.0
        for child in children:
            value += getattr(child, name)
        return value

    def log_prior(self) -> Tensor:
        """Sum of the children's log_prior (model.py:70-78); mean over the S samples of the last forward."""
        return self._sum(0, "log_prior")

    def log_variational_posterior(self) -> Tensor:
        """Sum of the children's log_variational_posterior (model.py:81-89); mean over the S samples."""
        return self._sum(1, "log_variational_posterior")

    def _kl_params(self):
        params = []
        for layer in self.fused_children():
            for gauss, _, _ in layer.gaussians():
                params += [gauss.mu, gauss.rho]
        return params

    def log_prob_samples(self) -> Tensor:
        """[S, 2] float64: per-sample {log_prior, log_variational_posterior} summed over the fused layers.

        Detached, as in the reference, unless bayeformers_amd.set_kl_gradient(True): then the result carries the
        Bayes-by-Backprop gradient w.r.t. every layer's mu and rho."""
        if self._lp_buf is None:
            raise RuntimeError("no forward has run yet")
        lp = self._lp_buf.sum(0)
        if bfr.STATE.kl_gradient and torch.is_grad_enabled() and self._only_fused():
            lp = _KLFn.apply(lp, self, self._last_S, self._last_seed, self._last_base, self._last_counter,
                             *self._kl_params())
        return lp

    def log_prior_samples(self) -> Tensor:
        return self.log_prob_samples()[:, 0]

    def log_variational_posterior_samples(self) -> Tensor:
        return self.log_prob_samples()[:, 1]
