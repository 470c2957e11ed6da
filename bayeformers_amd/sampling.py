"""The S-sample Monte-Carlo loop and the ELBO — the user-side harness of the reference, as one batched call.

Reference: `sample_bayesian` in /root/reference/examples/bert_glue.py:56-73 and examples/bert_squad.py:190-212,
the inline loop of examples/mlp_mnist.py:97-107 and README.md:58-72 — S serial forwards, then the mean over S of
the outputs and of the two log-prob scalars; the NLL is taken on the MEAN output and
`loss = (lvp - log_prior) / n_batches + nll` (bert_glue.py:234-235).

Here the S samples are folded into the batch axis of ONE forward (`Model.monte_carlo`), and optionally sharded
over the ranks of a torch.distributed group: rank r runs the global sample indices
[base + r*S/G, base + (r+1)*S/G), so per-sample results do not depend on the number of GPUs, and a single
all-reduce (RCCL over xGMI on MI355X) of the packed [sum of outputs | sum log_prior | sum lvp] buffer finishes the
step.  The message is KB-sized, i.e. latency-bound: one collective per step, on the compute stream.
"""
import math
import numbers
from dataclasses import dataclass, fields
from typing import Any, Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple, Union

import torch
import torch.distributed as dist
from torch import Tensor

from . import random as bfr
from .nn.model import Model


# Repeated inputs of the last two (tensor, S) pairs: a loop that feeds the SAME resident batch tensors again (the
# benchmark's fixed batch, an evaluation loop over a cached batch) does not pay the S-fold copies in every step.  An entry
# is valid only for the very same tensor object, unmodified (`_version`), whose repeated copy is unmodified too; it holds
# the source by weak reference, so a DataLoader loop (a new tensor every step) pins nothing but the last two copies.
_REPEAT_CACHE: Dict[int, tuple] = {}
_REPEAT_CACHE_SIZE = 2


def _repeat_cached(v: Tensor, samples: int) -> Tensor:
    import weakref

    if v.is_inference():  # no version counter to watch
        return v.repeat(samples, *([1] * (v.dim() - 1)))
    key = id(v)
    hit = _REPEAT_CACHE.get(key)
    if (hit is not None and hit[0]() is v and hit[1] == v._version and hit[2] == samples and hit[3] == v.data_ptr()
            and hit[4]._version == hit[5]):
        return hit[4]
    out = v.repeat(samples, *([1] * (v.dim() - 1)))
    # what it is made of (consumers that are the same for every copy use the original) — by WEAK reference, like the cache
    # entry: the copy must not keep its source alive
    out._bf_repeat = (samples, weakref.ref(v))
    if out.numel() * out.element_size() > (64 << 20):
        return out  # large inputs are not worth pinning
    if key not in _REPEAT_CACHE and len(_REPEAT_CACHE) >= _REPEAT_CACHE_SIZE:
        _REPEAT_CACHE.pop(next(iter(_REPEAT_CACHE)))
    _REPEAT_CACHE[key] = (weakref.ref(v), v._version, samples, v.data_ptr(), out, out._version)
    return out


def repeat_inputs(inputs: Union[Tensor, Dict[str, Any], Sequence[Any]], samples: int):
    """Repeat every tensor S times along dim 0, sample-major ([s0 batch | s1 batch | ...])."""
    def rep(v):
        if isinstance(v, Tensor) and v.dim() > 0:
            if samples == 1:
                return v
            # (integer / bool inputs carry no gradient: cached in training steps too)
            if not v.requires_grad and (not torch.is_grad_enabled() or not v.is_floating_point()):
                return _repeat_cached(v, samples)
            return v.repeat(samples, *([1] * (v.dim() - 1)))
        return v

    if isinstance(inputs, Tensor):
        return rep(inputs)
    if isinstance(inputs, dict):
        return {k: rep(v) for k, v in inputs.items()}
    return type(inputs)(rep(v) for v in inputs)


def _default_select(out):
    if isinstance(out, Tensor):
        return (out,)
    if hasattr(out, "start_logits") and hasattr(out, "end_logits"):  # HF question answering
        return (out.start_logits, out.end_logits)
    if hasattr(out, "logits"):
        return (out.logits,)
    raise TypeError("sample_bayesian: pass select= to pick the output tensor(s) of the model")


def _all_reduce_sum(t: Tensor, group) -> Tensor:
    """Sum over the ranks of the S-shard group.  With gradients recorded the result keeps THIS rank's part of the sum in
    the autograd graph (value = the global sum; d/d(local) = 1): a loss built on the all-reduced means then sends each
    rank the gradient of its own samples, and summing the ranks' parameter gradients (training.GradientBuckets) gives
    the gradient of the single-process step."""
    if torch.is_grad_enabled() and t.requires_grad:
        total = t.detach().clone()
        dist.all_reduce(total, op=dist.ReduceOp.SUM, group=group)
        return t + (total - t.detach())
    dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
    return t


def shard_span(samples: int, rank: int, world: int) -> Tuple[int, int]:
    """(first global sample index, number of samples) of rank `rank` when `samples` Monte-Carlo samples are sharded
    over `world` ranks: contiguous slices whose sizes differ by at most one (S = 10 over 8 GPUs: 2, 2, 1, 1, 1, 1, 1, 1 —
    BASELINE config 5's 8-GPU leg).  A rank past the last sample gets (samples, 0)."""
    q, r = divmod(int(samples), int(world))
    return rank * q + min(rank, r), q + (1 if rank < r else 0)


def _shard_group(group):
    """(distributed?, rank, world) of the S-shard group."""
    distributed = dist.is_available() and dist.is_initialized() and (group is not None or dist.get_world_size() > 1)
    world = dist.get_world_size(group) if distributed else 1
    rank = dist.get_rank(group) if distributed else 0
    return distributed, rank, world


def _local_step(model: Model, inputs, samples: int, select: Optional[Callable], rank: int, world: int, repeated: bool = False):
    """This rank's part of a step: the batched forward of its slice of the samples and the sums over them.  Returns
    (raw, sizes, local) — local is what the ranks add up: ONE packed fp64 buffer [sums of the outputs | sum log_prior |
    sum lvp] when the outputs are small, else (fp32 output sums, fp64 log-prob sums).  repeated: `inputs` are already
    the S_local-fold repeat."""
    if samples < 1:
        raise ValueError(f"samples={samples}: at least one Monte-Carlo sample")
    start, count = shard_span(samples, rank, world)
    idle = count == 0
    if idle:
        start, count = 0, 1
    s_local = count
    select = select or _default_select

    rep = inputs if repeated else repeat_inputs(inputs, s_local)
    with model.monte_carlo(s_local, span=(start, samples)):
        if isinstance(rep, dict):
            out = model(**rep)
        elif isinstance(rep, Tensor):
            out = model(rep)
        else:
            out = model(*rep)
    outs = select(out)
    raw = tuple(o.reshape(s_local, o.shape[0] // s_local, *o.shape[1:]) for o in outs)
    lp = model.log_prob_samples()  # [S_local, 2] float64

    # sums over this rank's samples: outputs in fp32 (fused convert-on-load, they can be large), the two log-prob
    # scalars in fp64; small outputs ride in the same fp64 buffer so that a distributed step is ONE collective
    sizes = [r[0].numel() for r in raw]
    one_buffer = sum(sizes) <= 65536
    acc_dt = torch.float64 if one_buffer else torch.float32
    sums = [r.sum(0, dtype=acc_dt).reshape(-1) for r in raw]
    if idle:  # this rank's forward only provided the shapes
        sums, lp, raw = [t * 0 for t in sums], lp * 0, tuple(r[:0] for r in raw)
    if one_buffer:
        local = (torch.cat(sums + [lp.sum(0)]),)
    else:
        local = (torch.cat(sums) if len(sums) > 1 else sums[0], lp.sum(0))
    return raw, sizes, local


def _finish_step(raw, sizes, local, samples: int, group, distributed: bool):
    """The step's collective(s) and the means over ALL samples: (means, log_prior, lvp)."""
    n_out = sum(sizes)
    if distributed:
        local = tuple(_all_reduce_sum(t, group) for t in local)
    if len(local) == 1:
        packed = local[0] / samples
        out_part, lp_part = packed[:n_out], packed[n_out:]
    else:
        out_part, lp_part = local[0] / samples, local[1] / samples
    means, off = [], 0
    for r, n in zip(raw, sizes):
        means.append(out_part[off:off + n].reshape(r.shape[1:]).to(r.dtype))
        off += n
    return means, lp_part[0], lp_part[1]


def sample_bayesian(model: Model, inputs, samples: int, select: Optional[Callable] = None,
                    group: Optional["dist.ProcessGroup"] = None, gather_raw: bool = False, graph: bool = False
                    ) -> Tuple[Tuple[Tensor, ...], Tuple[Tensor, ...], Tensor, Tensor]:
    """Run `samples` Monte-Carlo forwards of `model` as one batched forward.

    inputs: a tensor, a dict of tensors (HF style, called as model(**inputs)) or a sequence (model(*inputs)) for ONE
        batch; they are repeated S_local times here.
    select: maps the model output to a tuple of [S_local*B, ...] tensors to average (default: `.logits`,
        `(start_logits, end_logits)`, or the output itself).
    group: if torch.distributed is initialised (or a group is given) the samples are sharded over its ranks in
        contiguous slices whose sizes differ by at most one (`shard_span`); `samples` need not be a multiple of the
        world size.  (A rank left without a sample — more ranks than samples — still runs one forward, of the step's
        first sample, to learn the output shapes; it enters the reduction with weight zero.)

    Returns (raw, mean, log_prior, log_variational_posterior):
        raw   tuple of [S_local, B, ...] per-sample outputs of this rank, S_local = shard_span(...)[1] (all S if gather_raw),
        mean  tuple of [B, ...] means over ALL S samples,
        log_prior, log_variational_posterior: 0-d float64 means over ALL S samples.
    graph: evaluation loops — replay the step from a HIP graph (`GraphedSampler`, kept for the last two batch signatures of
        this model; results are the graph's buffers, valid until the next call with the same signature).  Needs no_grad /
        inference mode and a model in eval mode; not combined with gather_raw.
    """
    if graph:
        if gather_raw:
            raise ValueError("sample_bayesian: graph=True does not gather the ranks' raw outputs")
        if torch.is_grad_enabled():
            raise RuntimeError("sample_bayesian: graph=True replays a captured forward — call it under torch.no_grad()")
        return _graphed(model, inputs, samples, select, group)
    distributed, rank, world = _shard_group(group)
    raw, sizes, local = _local_step(model, inputs, samples, select, rank, world)
    means, log_prior, lvp = _finish_step(raw, sizes, local, samples, group, distributed)
    if distributed and gather_raw:
        # shards may differ by one sample: every rank sends ceil(S / world) slabs, the receiver keeps each rank's own
        s_max = -(-samples // world)
        counts = [shard_span(samples, r, world)[1] for r in range(world)]
        gathered = []
        for r in raw:
            send = r.contiguous()
            if send.shape[0] < s_max:
                send = torch.cat([send, send.new_zeros((s_max - send.shape[0],) + tuple(send.shape[1:]))], 0)
            parts = [torch.empty_like(send) for _ in range(world)]
            dist.all_gather(parts, send, group=group)
            gathered.append(torch.cat([part[:c] for part, c in zip(parts, counts)], 0))
        raw = tuple(gathered)
    return raw, tuple(means), log_prior, lvp


@dataclass
class Predictive:
    """Monte-Carlo predictive statistics of one output over the step's S samples (bf_mc_predictive_*).  Every field is a
    device tensor (reading one is the caller's synchronisation).  Row shapes are the output's without its sample and class
    axes ([B] for sequence classification, [B, T] for token classification; start/end logits: [B], the classes being the
    positions).

        probs                [..., C] fp32  Bayesian-model-average probabilities, mean over s of softmax(l_s)
        predictive_entropy   [...]   fp32  H(probs)                            (total uncertainty)
        expected_entropy     [...]   fp32  mean over s of H(softmax(l_s))     (aleatoric)
        mutual_information   [...]   fp32  max(0, predictive - expected)      (epistemic)
        prediction           [...]   int64 argmax probs (first index on ties)
    with labels (else None):
        correct_per_sample   [S]     int64 rows each sample classifies correctly (the reference's per-sample count)
        acc_std              0-d     fp64  population std of correct_per_sample (np.std, bert_glue.py:237)
        bma_correct          0-d     int64 rows `prediction` gets right
        log_likelihood       [...]   fp64  log mean over s of p_s(label); NaN on ignored rows
        nll                  0-d     fp64  -mean log_likelihood over the valid rows
        invalid_labels       0-d     int64 labels neither ignore_index nor in [0, C) (treated as ignored)
    from sample_predictive (else None): mean (the output's mean over S), log_prior, log_variational_posterior."""
    probs: Tensor
    predictive_entropy: Tensor
    expected_entropy: Tensor
    mutual_information: Tensor
    prediction: Tensor
    mean: Optional[Tensor] = None
    log_prior: Optional[Tensor] = None
    log_variational_posterior: Optional[Tensor] = None
    correct_per_sample: Optional[Tensor] = None
    acc_std: Optional[Tensor] = None
    bma_correct: Optional[Tensor] = None
    log_likelihood: Optional[Tensor] = None
    nll: Optional[Tensor] = None
    invalid_labels: Optional[Tensor] = None

    def clone(self) -> "Predictive":
        return Predictive(**{f.name: (None if getattr(self, f.name) is None else getattr(self, f.name).clone())
                             for f in fields(self)})


def _predictive_rows(raw: Tensor, labels: Optional[Tensor], what: str = "mc_predictive", idle: bool = False):
    """raw [S, B, ..., C] -> ([S, R, C] view, labels [R] int64 or None); shapes are checked before devices.  idle: raw is
    the empty [0, B, ..., C] of a rank without a sample (its view is then None)."""
    if not isinstance(raw, Tensor) or raw.dim() < 2:
        raise ValueError(f"{what}: expected per-sample outputs [S, B, ..., C], got {getattr(raw, 'shape', type(raw))}")
    S, C = raw.shape[0], raw.shape[-1]
    rows = tuple(raw.shape[1:-1])
    if (S < 1 and not idle) or C < 1 or any(n == 0 for n in rows):
        raise ValueError(f"{what}: empty outputs {tuple(raw.shape)}")
    if raw.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        raise TypeError(f"{what}: logits must be fp32, bf16 or fp16, not {raw.dtype}")
    if labels is not None:
        if not isinstance(labels, Tensor) or tuple(labels.shape) != rows:
            raise ValueError(f"{what}: labels must have the output's row shape {rows} (outputs {tuple(raw.shape)}), "
                             f"got {tuple(labels.shape) if isinstance(labels, Tensor) else type(labels)}")
        if labels.dtype.is_floating_point or labels.dtype == torch.bool:
            raise TypeError(f"{what}: labels must be integer class indices, not {labels.dtype}")
    from . import ops
    from ._C import BayeFormersAMDError

    ops._require_device(raw, f"{what} outputs")
    if labels is not None and labels.device != raw.device:
        raise BayeFormersAMDError(f"{what}: labels live on '{labels.device}', the outputs on '{raw.device}'")
    lab = None if labels is None else labels.reshape(-1).to(torch.int64).contiguous()
    if idle:
        return None, lab
    r3 = raw.reshape(S, -1, C)
    if C > 1 and r3.stride(2) != 1:
        r3 = r3.contiguous()
    return r3, lab


class _PredictiveItem(NamedTuple):
    """One output of a predictive step: its per-sample shape [..., C] without the sample axis, rows, classes, labels [R]
    (or None), and the packed partials with their fp32 and fp64 parts (views of `partial`)."""
    shape: tuple
    R: int
    C: int
    labels: Optional[Tensor]
    partial: Tensor
    f32: Tensor
    f64: Tensor


class _PredictiveStep:
    """The predictive statistics of one step's outputs: the partial launch of every output (this rank's samples), the
    partials' ride in the step's collective, and the finish launches.  ws: the kernels' workspace (default: the cached one
    of the current device and stream, ops.predictive_workspace)."""

    def __init__(self, raw, labels, ignore_index: int, samples: int, sample_base: int = 0, idle: bool = False,
                 ws: Optional[Tensor] = None, what: str = "sample_predictive"):
        from . import ops

        self.items: List[_PredictiveItem] = []
        self.samples, self.ignore_index, self.ws = int(samples), int(ignore_index), ws
        for r, lab in zip(raw, labels):
            r3, lab = _predictive_rows(r, lab, what, idle)
            C = r.shape[-1]
            R = int(torch.Size(r.shape[1:-1]).numel())
            nbytes, offs = ops.predictive_layout(R, C, samples, lab is not None)
            if self.ws is None:
                self.ws = ops.predictive_workspace(r.device, samples)
            partial = torch.empty(nbytes, dtype=torch.uint8, device=r.device)
            if idle:  # this rank ran no sample: it enters the sums with zeros
                partial.zero_()
            else:
                ops.predictive_partial(r3, lab, ignore_index, sample_base, samples, partial, self.ws)
            self.items.append(_PredictiveItem(tuple(r.shape[1:]), R, C, lab, partial, partial[:offs[2]].view(torch.float32),
                                              partial[offs[2]:offs[5]].view(torch.float64)))

    def pack(self, local):
        """The step's collective buffers with the partials appended: ONE fp64 buffer when the step has one (the fp32 sums
        ride as fp64), else (fp32 sums | fp32 partials, fp64 sums | fp64 partials)."""
        if len(local) == 1:
            return (torch.cat([local[0]] + [it.f32.double() for it in self.items] + [it.f64 for it in self.items]),)
        return (torch.cat([local[0]] + [it.f32 for it in self.items]), torch.cat([local[1]] + [it.f64 for it in self.items]))

    def unpack(self, packed, local):
        """Copy the reduced partials back; returns the step's own reduced buffers (shaped as `local`)."""
        if len(local) == 1:
            parts = [[it.f32 for it in self.items] + [it.f64 for it in self.items]]
        else:
            parts = [[it.f32 for it in self.items], [it.f64 for it in self.items]]
        out = []
        for buf, own, dsts in zip(packed, local, parts):
            off = own.numel()
            for t in dsts:
                t.copy_(buf[off:off + t.numel()])
                off += t.numel()
            out.append(buf[:own.numel()])
        return tuple(out)

    def finish(self, means=None, log_prior=None, lvp=None) -> List[Predictive]:
        from . import ops

        res = []
        for k, it in enumerate(self.items):
            has_labels = it.labels is not None
            o = ops.predictive_outputs(it.R, it.C, self.samples, has_labels, it.partial.device)
            ops.predictive_finish(it.partial, it.R, it.C, self.samples, it.labels, self.ignore_index, o, self.ws)
            rows = it.shape[:-1]
            p = Predictive(probs=o["probs"].view(it.shape), predictive_entropy=o["predictive_entropy"].view(rows),
                           expected_entropy=o["expected_entropy"].view(rows),
                           mutual_information=o["mutual_information"].view(rows), prediction=o["prediction"].view(rows),
                           mean=None if means is None else means[k], log_prior=log_prior, log_variational_posterior=lvp)
            if has_labels:
                p.correct_per_sample, p.log_likelihood = o["correct_per_sample"], o["log_likelihood"].view(rows)
                p.acc_std, p.nll = o["scalars"][0], o["scalars"][1]
                p.bma_correct, p.invalid_labels = o["counts"][0], o["counts"][1]
            res.append(p)
        return res


def mc_predictive(raw: Tensor, labels: Optional[Tensor] = None, ignore_index: int = -100) -> Predictive:
    """Predictive statistics of S per-sample outputs raw [S, B, ..., C] (e.g. `raw[0]` of sample_bayesian): the dims between
    the sample and class axes fold into rows (token classification [S, B, T, C]: R = B*T).  labels: integer [B, ...] or
    None.  Two launches, no host synchronisation; single process (an S-sharded step: sample_predictive).  A CPU tensor
    raises: the statistics run in HIP kernels only."""
    samples = raw.shape[0] if isinstance(raw, Tensor) and raw.dim() >= 2 else 0
    return _PredictiveStep((raw,), (labels,), ignore_index, samples, what="mc_predictive").finish()[0]


def _labels_per_output(labels, n_out: int):
    if labels is None:
        return (None,) * n_out
    if isinstance(labels, Tensor):
        labels = (labels,)
    labels = tuple(labels)
    if len(labels) != n_out:
        raise ValueError(f"sample_predictive: {len(labels)} label tensors for {n_out} selected outputs (question answering: "
                         "pass (start_positions, end_positions))")
    return labels


def _label_sig(labels):
    if labels is None:
        return None
    if isinstance(labels, Tensor):
        labels = (labels,)
    return tuple(None if t is None else (tuple(t.shape), t.dtype, t.device) for t in labels)


def sample_predictive(model: Model, inputs, samples: int, labels=None, select: Optional[Callable] = None,
                      group: Optional["dist.ProcessGroup"] = None, ignore_index: int = -100, graph: bool = False
                      ) -> Tuple[Predictive, ...]:
    """The step of `sample_bayesian` (same forward, same samples, same mean / log_prior / lvp) plus the predictive statistics
    of every selected output: one `Predictive` per output.  labels: an integer tensor of the output's row shape, or one per
    output (question answering: (start_positions, end_positions)), or None.

    Sharded over an S-shard group, each rank computes the partial sums of its samples and they ride in the step's own
    collective (ONE all-reduce when the outputs are small, as in sample_bayesian; two otherwise); there is no all-gather.
    graph=True replays the step and the statistics from a HIP graph (`GraphedSampler(predictive=True)`, cached as for
    sample_bayesian; the results are copies).  The results are detached: evaluation statistics."""
    if graph:
        if torch.is_grad_enabled():
            raise RuntimeError("sample_predictive: graph=True replays a captured forward — call it under torch.no_grad()")
        return _graphed(model, inputs, samples, select, group, predictive=True, labels=labels, ignore_index=ignore_index)
    distributed, rank, world = _shard_group(group)
    with torch.no_grad():
        raw, sizes, local = _local_step(model, inputs, samples, select, rank, world)
        start, count = shard_span(samples, rank, world)
        step = _PredictiveStep(raw, _labels_per_output(labels, len(raw)), ignore_index, samples, start, count == 0)
        if distributed:
            packed = step.pack(local)
            for t in packed:
                dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
            local = step.unpack(packed, local)
        means, log_prior, lvp = _finish_step(raw, sizes, local, samples, None, False)
        return tuple(step.finish(means, log_prior, lvp))


_GRAPHED_KEEP = 2  # GraphedSamplers kept per model by sample_bayesian(graph=True): the last two batch signatures


def graphed_samplers(model: Model) -> list:
    """[(key, GraphedSampler)], most recent last: the samplers `sample_bayesian(graph=True)` keeps for `model`.  They live in
    the model's graph cache (graphs.GraphCache: copies and pickles of the model start with an empty one); model -> cache ->
    sampler -> model is an ordinary reference cycle, so a dropped model is collected with its samplers, whose graphs are then
    released and whose hold on the device-resident sample counter ends (GraphCache.__del__)."""
    from .graphs import GraphCache

    cache = model.__dict__.get("_graphs")
    if cache is None:
        cache = model.__dict__["_graphs"] = GraphCache()
    return cache.samplers


_IMMUTABLE = (type(None), bool, int, float, str, bytes)


def _select_key(select):
    """Cache identity of a `select` callable, or None when two calls cannot be told to select the same thing (then nothing is
    cached: every call captures).  A lambda written at the call site is a new object on every call but the same code; it is
    the same selection only if what it captured is the same VALUE — closures over immutable scalars (and tuples of them) are
    compared by value, anything else (a list or tensor that may be mutated, an object whose id may be reused) is refused.
    A plain function without a closure and a bound method of a live object are themselves the key; a functools.partial is
    keyed by its function and (immutable) arguments."""
    import functools

    def frozen(v):
        if isinstance(v, _IMMUTABLE):
            return True
        return isinstance(v, tuple) and all(frozen(x) for x in v)

    if select is None:
        return ("default",)
    if isinstance(select, functools.partial):
        inner = _select_key(select.func)
        kw = tuple(sorted(select.keywords.items()))
        if inner is None or not frozen(select.args) or not frozen(tuple(v for _, v in kw)):
            return None
        return ("partial", inner, select.args, kw)
    code = getattr(select, "__code__", None)
    if code is None:
        return ("object", select)  # a callable object: held by the key, compared by identity (its default __eq__) or its own
    cells = []
    for c in select.__closure__ or ():
        try:
            v = c.cell_contents
        except ValueError:  # an empty cell
            return None
        if not frozen(v):
            return None
        cells.append(v)
    if not frozen(select.__defaults__ or ()):
        return None
    return ("function", code, select.__defaults__, tuple(cells), getattr(select, "__self__", None))


def _graphed(model: Model, inputs, samples: int, select, group, predictive: bool = False, labels=None,
             ignore_index: int = -100):
    cache = graphed_samplers(model)
    skey = _select_key(select)
    pkw = dict(predictive=True, labels=labels, ignore_index=ignore_index) if predictive else {}
    if skey is None:  # a selection that cannot be recognised again: capture for this call only
        sampler = GraphedSampler(model, inputs, samples, select=select, group=group, **pkw)
        try:
            if predictive:
                return tuple(p.clone() for p in sampler(inputs, labels))
            raw, means, log_prior, lvp = sampler(inputs)
            return tuple(r.clone() for r in raw), tuple(m.clone() for m in means), log_prior.clone(), lvp.clone()
        finally:
            sampler.close()
    key = (GraphedSampler._sig(inputs), int(samples), skey, group)
    if predictive:
        key = key + (("predictive", _label_sig(labels), int(ignore_index)),)
    sampler = None
    for i, (k, sm) in enumerate(cache):
        if k == key and sm.graph is not None:
            cache.append(cache.pop(i))
            sampler = sm
            break
    if sampler is None:
        while len(cache) >= _GRAPHED_KEEP:
            cache.pop(0)[1].close()
        sampler = GraphedSampler(model, inputs, samples, select=select, group=group, **pkw)
        cache.append((key, sampler))
    if predictive:  # copies, as for the means below
        return tuple(p.clone() for p in sampler(inputs, labels))
    raw, means, log_prior, lvp = sampler(inputs)
    # the convenience path hands out COPIES of the small results (an evaluation loop that collects `mean[0]` per batch
    # must not end up with the last batch in every entry); `raw` stays the graph's buffer, valid until the next call
    return raw, tuple(m.clone() for m in means), log_prior.clone(), lvp.clone()


def elbo(log_prior: Tensor, log_variational_posterior: Tensor, nll: Tensor, n_batches: int) -> Tensor:
    """loss = (lvp - log_prior) / n_batches + nll  (bert_glue.py:235, mlp_mnist.py:107, README.md:72)."""
    return torch.add(nll, log_variational_posterior - log_prior, alpha=1.0 / n_batches)


class GraphedSampler:
    """`sample_bayesian` for ONE batch signature, replayed from a HIP graph (inference / evaluation).

    A small step is bound by the host, not by the GPU: the forward of a BERT-base shard of 1-3 samples is ~2-3 ms of
    kernels behind 4-7 ms of Python and launch calls (what a strong-scaling shard of S = 10 over 8 GPUs runs, or a
    latency-bound evaluation with few samples).  This class runs the rank's part of the step — input repeat, the batched
    forward, the sampling plan's launches, the sums over the rank's samples, and on a single process the means too — once
    under `torch.cuda.graph` and replays it; the Monte-Carlo sample counter lives in device memory while it exists
    (`use_device_counter`), so replay k draws the epsilon the k-th eager step would have drawn.  With an S-shard group the
    step's one collective runs eagerly after the replay (RCCL on the compute stream), exactly as in `sample_bayesian`.

        sampler = GraphedSampler(bmodel, inputs, samples=10)
        raw, mean, log_prior, lvp = sampler()            # same batch, fresh epsilon
        raw, mean, log_prior, lvp = sampler(next_inputs)  # same shapes / dtypes: copied into the captured buffers

    The returned tensors are the graph's own buffers (`mean`, the log-probs: fresh tensors when a group reduces them): the
    next call overwrites them — clone what must outlive it.  Gradients are not recorded (training steps are not
    replayable: their dropout masks and autograd graphs are per step) and the model must be in eval mode.

    What a capture bakes in besides the shapes: the Philox SEED (a kernel argument), the compute dtype and the sampling
    plan (which priors are aliases of their frozen means, where the sampled weights live).  `__call__` compares them with
    the current state and captures again when one changed (`bf.manual_seed(other)`, `set_compute_dtype`, an edited prior),
    so a replay never draws from a stale key or dtype.  The capture's warm-up steps give their sample indices back:
    `manual_seed(s); GraphedSampler(...)()` equals the eager call from the same state, and replay k the k-th eager step.

    predictive=True captures the predictive statistics too (`sample_predictive`): a call returns one `Predictive` per
    output (the graph's buffers, like the rest).  labels: the labels of the first batch (a tensor, one per output, or None
    for the label-free statistics); they are copied into captured buffers, and `sampler(inputs, labels)` copies new ones
    in, so labels are never baked in by address.  With an S-shard group the partials ride in the step's collective after
    the replay, then the finish launches run."""

    def __init__(self, model: Model, inputs, samples: int, select: Optional[Callable] = None,
                 group: Optional["dist.ProcessGroup"] = None, warmup: int = 2, predictive: bool = False, labels=None,
                 ignore_index: int = -100) -> None:
        from . import graphs

        if model.training:
            raise RuntimeError("GraphedSampler: the model is in training mode (dropout masks are per step); call model.eval()")
        self.model, self.samples, self.select, self.group = model, int(samples), select, group
        self.distributed, self.rank, self.world = _shard_group(group)
        tensors = [v for v in self._leaves(inputs) if isinstance(v, Tensor)]
        if not tensors or not all(t.is_cuda for t in tensors):
            raise RuntimeError("GraphedSampler: the inputs must be tensors on the GPU the model runs on")
        self.device = tensors[0].device
        self._s_local = max(1, shard_span(self.samples, self.rank, self.world)[1])
        # the S_local-fold repeat of the batch is made ONCE, here: a new batch is copied into it (broadcast over the
        # sample axis) and the captured step starts at the model's forward
        self._signature = self._sig(inputs)
        with torch.inference_mode(False):  # (buffers that later calls write, in whatever mode they run: never inference tensors)
            self._rep = self._map(inputs, lambda v: v.repeat(self._s_local, *([1] * (v.dim() - 1))) if v.dim() > 0 else v.clone())
        self.predictive, self.ignore_index = bool(predictive), int(ignore_index)
        self._labels = None
        if labels is not None and not self.predictive:
            raise ValueError("GraphedSampler: labels are for predictive=True")
        if self.predictive:
            from . import ops

            if labels is not None:
                labels = (labels,) if isinstance(labels, Tensor) else tuple(labels)
                with torch.inference_mode(False):
                    self._labels = tuple(None if t is None else t.to(self.device, torch.int64).clone() for t in labels)
            # the predictive kernels' workspace is the sampler's own (zero-filled once; the kernels leave it zeroed)
            with torch.inference_mode(False):
                self._pws = torch.zeros(ops._C.lib().bf_mc_predictive_workspace_bytes(self.samples), dtype=torch.uint8,
                                        device=self.device)
        # the captured kernels hold the counter's ADDRESS: it must stay on the device until the last sampler is closed
        graphs.acquire_counter(self.device)
        self._open = True
        self.graph = self._static = None
        self._warmup = max(1, int(warmup))
        self.captures = 0
        try:
            self._capture()
        except BaseException:
            self.close()  # a failed capture leaves nothing behind (the counter goes back where it was)
            raise

    def _baked(self):
        """The host state a capture bakes into its launches."""
        from . import graphs

        return graphs.baked_state(self.model)

    def _capture(self) -> None:
        from . import random as bfr

        self.graph = self._static = None
        with torch.inference_mode(False), torch.no_grad(), torch.cuda.device(self.device):
            for _ in range(self._warmup):  # plans, workspaces and tile schedules are built outside the capture
                self._step()
            # the warm-up steps consumed sample indices the caller never saw: hand them back, so that the first replay
            # draws what the eager step from the caller's state would have drawn
            bfr.STATE.device_counter.sub_(self._warmup * self.samples)
            bfr.STATE.device_drop_counter.sub_(self._warmup)  # (one dropout call number per forward, used or not)
            bfr.STATE.counter_moves += 1
            torch.cuda.synchronize(self.device)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                self._static = self._step()
            self.graph = graph
        self._baked_state = self._baked()
        self.captures += 1

    def _still_valid(self) -> bool:
        from . import graphs

        return graphs.still_valid(self.model, self._baked_state)

    # ------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _leaves(inputs):
        if isinstance(inputs, Tensor):
            return [inputs]
        return list(inputs.values()) if isinstance(inputs, dict) else list(inputs)

    @staticmethod
    def _map(inputs, fn):
        f = lambda v: fn(v) if isinstance(v, Tensor) else v
        if isinstance(inputs, Tensor):
            return f(inputs)
        if isinstance(inputs, dict):
            return {k: f(v) for k, v in inputs.items()}
        return type(inputs)(f(v) for v in inputs)

    @classmethod
    def _sig(cls, inputs):
        keys = list(inputs.keys()) if isinstance(inputs, dict) else None
        return keys, [(tuple(v.shape), v.dtype, v.device) if isinstance(v, Tensor) else v for v in cls._leaves(inputs)]

    def _step(self):
        raw, sizes, local = _local_step(self.model, self._rep, self.samples, self.select, self.rank, self.world, repeated=True)
        pred = None
        if self.predictive:
            start, count = shard_span(self.samples, self.rank, self.world)
            labels = self._labels if self._labels is not None else _labels_per_output(None, len(raw))
            pred = _PredictiveStep(raw, _labels_per_output(labels, len(raw)), self.ignore_index, self.samples, start,
                                   count == 0, ws=self._pws)
        if self.distributed:
            return raw, sizes, local, None, pred
        done = _finish_step(raw, sizes, local, self.samples, None, False)
        if pred is not None:
            pred = pred.finish(*done)
        return raw, sizes, local, done, pred

    def load(self, inputs) -> None:
        """Copy a new batch (same structure, shapes, dtypes, device) into the captured input buffers."""
        if self._sig(inputs) != self._signature:
            raise ValueError("GraphedSampler: the batch differs from the captured one in structure, shape, dtype or device; "
                             "build another GraphedSampler for it")
        S = self._s_local
        for dst, src in zip(self._leaves(self._rep), self._leaves(inputs)):
            if isinstance(src, Tensor):
                (dst.view(S, *src.shape) if src.dim() > 0 else dst).copy_(src)

    def load_labels(self, labels) -> None:
        """Copy new labels (same shapes as the captured ones) into the captured label buffers."""
        if not self.predictive or self._labels is None:
            raise ValueError("GraphedSampler: labels need a sampler built with predictive=True and labels")
        labels = (labels,) if isinstance(labels, Tensor) else tuple(labels)
        if len(labels) != len(self._labels) or any(
                (a is None) != (b is None) or (a is not None and tuple(a.shape) != tuple(b.shape))
                for a, b in zip(self._labels, labels)):
            raise ValueError("GraphedSampler: the labels differ in number or shape from the captured ones")
        for dst, src in zip(self._labels, labels):
            if dst is not None:
                dst.copy_(src)

    def __call__(self, inputs=None, labels=None):
        if self.graph is None:
            raise RuntimeError("GraphedSampler: closed")
        if self.model.training:
            raise RuntimeError("GraphedSampler: the model was switched to training mode after the capture; the captured "
                               "forward is the evaluation one — call model.eval(), or build a new sampler")
        if not self._still_valid():  # another seed / compute dtype / plan than the captured launches carry
            self._capture()
        if inputs is not None:
            self.load(inputs)
        if labels is not None:
            self.load_labels(labels)
        self.graph.replay()
        raw, sizes, local, done, pred = self._static
        if pred is not None:
            if done is None:  # the collective (partials appended to the step's buffers), then the finish launches
                with torch.no_grad():
                    packed = pred.pack(local)
                    for t in packed:
                        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group)
                    done = _finish_step(raw, sizes, pred.unpack(packed, local), self.samples, None, False)
                    return tuple(pred.finish(*done))
            return tuple(pred)
        if done is None:  # the S-shard group's collective, on clones: the graph's buffers stay what the replay wrote
            with torch.no_grad():
                done = _finish_step(raw, sizes, tuple(t.clone() for t in local), self.samples, self.group, True)
        means, log_prior, lvp = done
        return raw, tuple(means), log_prior, lvp

    def close(self) -> None:
        """Drop the graph; when the last open sampler closes and the samplers had moved the sample counter to the device,
        it moves back to the host (advanced by what the replays consumed)."""
        from . import graphs

        self.graph = self._static = None
        if self._open:
            self._open = False
            graphs.release_counter()


@dataclass
class Generation:
    """What `sample_generate` returns; device tensors.  n = max_new_tokens.

        sequences                   [B, T0 + n] int64  the prompt and the generated tokens (pad_token_id past a row's EOS)
        predictive_entropy          [B, n] fp32  H of the model-average probabilities of each step (total uncertainty)
        expected_entropy            [B, n] fp32  mean over the samples of H(softmax(l_s))      (aleatoric)
        mutual_information          [B, n] fp32  max(0, predictive - expected)                 (epistemic)
        token_prob                  [B, n] fp32  the model-average probability of the token chosen
        lengths                     [B] int64    tokens generated, the EOS included
        log_prior                   [S] fp64     per-sample log prior of the pinned weight draws
        log_variational_posterior   [S] fp64     per-sample log q of the same draws
        speculation                 [3] int64    sample_generate(speculative=...) only, else None: {verify steps, draft
                                                 tokens proposed, draft tokens accepted}
    The statistics of a step after a row's EOS are 0."""
    sequences: Tensor
    predictive_entropy: Tensor
    expected_entropy: Tensor
    mutual_information: Tensor
    token_prob: Tensor
    lengths: Tensor
    log_prior: Tensor
    log_variational_posterior: Tensor
    # (an attribute with a default, deliberately not a dataclass field: fields(), the constructor, == and repr stay the
    # eight tensors every generation has, so code that walks the fields never meets a None)
    speculation = None


def sample_generate(model: Model, input_ids: Tensor, attention_mask: Optional[Tensor] = None, samples: int = 1,
                    max_new_tokens: int = 1, do_sample: bool = False, temperature: float = 1.0,
                    eos_token_id: Optional[int] = None, pad_token_id: Optional[int] = None,
                    generator: Optional[torch.Generator] = None, group: Optional["dist.ProcessGroup"] = None,
                    keep_weights: Union[bool, str] = False, max_bytes: Optional[int] = None, static_cache: bool = False,
                    graph: bool = False, top_k: Optional[int] = None, top_p: Optional[float] = None,
                    min_p: Optional[float] = None, repetition_penalty: Optional[float] = None,
                    no_repeat_ngram_size: Optional[int] = None, min_new_tokens: Optional[int] = None,
                    kv_cache: Optional[str] = None, prefill_chunk: Optional[int] = None,
                    sliding_cache: Optional[str] = None, speculative: Optional[int] = None) -> Generation:
    """Generate with a Bayesian decoder (a HuggingFace causal LM converted by `to_bayesian`) and the per-token predictive
    uncertainty of its Monte-Carlo posterior.

    The whole generation runs under `model.monte_carlo(samples)` and `model.pinned_samples()`: each of the S samples is ONE
    draw of the weights for every token, with its own slice of the KV cache (the sample-major [S*B] batch).  Prefill is one
    forward over the prompt (input_ids [B, T0], left-padded rows marked by attention_mask [B, T0]); every later step feeds
    one token per row with `past_key_values`.  The last position's [S, B, V] logits, divided by `temperature`, go through
    `mc_predictive` (the bf_predictive kernels); the next token is the argmax of the model-average probabilities or, with
    do_sample, a draw from them (torch.multinomial with `generator`), fed to all S samples.  With do_sample, top_k /
    top_p / min_p truncate the model-average row before the draw as HF's warpers do, in HF's order (top-k, top-p on the
    renormalised top-k set, min-p): one bf_probs_truncate launch per step (ops.truncate_probs; its contract and tie rule
    are in include/bayeformers_amd.h), on the one row all S samples share; the draw is from the renormalised kept set.
    top_k must be an int >= 1, top_p in (0, 1], min_p in [0, 1]; None, top_k >= V, top_p = 1 and min_p = 0 launch
    nothing.  The statistics keep their meaning: the entropies, the MI and token_prob are those of the unfiltered,
    temperature-scaled predictive (a kept probability is bitwise the unfiltered one).

    repetition_penalty, no_repeat_ngram_size and min_new_tokens are HF's logits processors, in HF's order and bitwise
    HF's chain on the fp32 upcast of each sample's logits (then / temperature): every token already in the row's
    sequence (prompt, padding and pads of finished rows included) is penalised once, l < 0 ? l * θ : l / θ; a token that
    would repeat an n-gram of the sequence is banned; eos_token_id is banned while fewer than min_new_tokens tokens were
    generated.  They act on the S sample rows of a batch row alike, in greedy decoding as in sampling (before top_k /
    top_p / min_p): one bf_logits_process launch per step (ops.process_logits; contract in include/bayeformers_amd.h)
    and a second `mc_predictive` on the processed logits, whose model-average row chooses the token.  The statistics and
    token_prob stay those of the unprocessed, temperature-scaled predictive.  repetition_penalty must be finite and
    positive, no_repeat_ngram_size an int in [0, 64], min_new_tokens an int >= 0 and, when positive, needs
    eos_token_id.  None, repetition_penalty = 1, no_repeat_ngram_size = 0 and min_new_tokens = 0 (or a step at or past
    min_new_tokens) launch nothing: the Generation is bitwise the one without them.  Rows past eos_token_id emit
    pad_token_id (default: eos_token_id).  No host synchronisation per step except the all-finished check, and none
    without eos_token_id.  Single process, eval mode and no gradient only.

    keep_weights / max_bytes go to `model.pinned_samples`: with keep_weights=True the prefill samples every Bayesian Linear's
    S weight draws once and the decode steps run on them (bf_gemm_nt_skinny) instead of drawing them again per token, at the
    cost of plan.kept_weight_bytes(model, S, compute dtype) bytes of device memory; the result is the same Generation.
    keep_weights="fp8" (bf16 compute) keeps them as centred FP8 rows instead — one bf16 posterior mean per layer and one
    e4m3 byte per sampled weight for its deviation from it, plan.kept_weight_bytes(..., fp8=True) bytes — and decodes on
    bf_gemm_nt_skinny_fp8; prefill and decode multiply by the same dequantised weights, which are not bitwise the bf16 draws
    (Model.pinned_samples).  Any other value raises ValueError.

    static_cache=True decodes on a transformers StaticCache of capacity T0 + max_new_tokens - 1, filled from the (unchanged)
    prefill: every step has the same shapes, the attention runs on bf_attention_decode_gqa_len (the fill is a device
    scalar), the mask is preallocated and the positions and ids are updated in place, and the per-step bookkeeping is one
    bf_generate_step launch.  do_sample then draws by an inverse CDF from a Philox uniform per (row, step) keyed by a seed
    drawn once per call from `generator` (or torch's default generator): the same generator state gives the same text,
    but not the text of the default path's torch.multinomial.  graph=True (implies static_cache) runs one decode step
    eagerly, captures the next one in a HIP graph and replays it for the rest; the Generation is bitwise the one
    static_cache=True returns.  With eos_token_id the all-finished check runs every 8 replays (rows past EOS emit pad with
    zero statistics either way).  Both need a model routed by fuse_attention, a single process and no sliding-window
    layers — except in Mistral, Qwen2 and Qwen3 models, whose sliding layers get full-capacity static layers (capacity
    slots each, not W) and decode on bf_attention_decode_gqa_len_window.

    kv_cache="fp8" (implies static_cache; bf16 compute only) keeps that static cache as e4m3 rows — per cached K or V row D
    bytes and one fp32 power-of-two scale (include/bayeformers_amd_kv8.h), plan.kv_cache_bytes(..., fp8=True) bytes, 0.52x
    the bf16 cache at head size 128 — and decodes on bf_attention_decode_gqa_kv8, which reads the rows as they are: half
    the bytes kept and half the bytes every step reads.  The prompt's cache is bf16 until it is handed over (one
    bf_kv8_append per layer, each dynamic layer released as it goes); every later step appends its row with the same
    entry.  It composes with graph=True, keep_weights in any form, truncation, the logits processors, the sliding-window
    families and soft-capping.  The cached rows carry e4m3's rounding (at most 2^-4 relative per element), so the
    Generation is close to, not bitwise, the bf16 cache's.  None (the default) changes nothing; any other value, or a
    compute dtype other than bfloat16, raises ValueError.

    prefill_chunk=C (an int >= 17; needs a model routed by fuse_attention) feeds the prompt in spans of C tokens against the
    cache instead of one forward over all of it: only C positions of activations exist at a time, only the last span's
    last position goes through the lm_head (`logits_to_keep=1` where the wrapped model's forward takes it), and on the
    static_cache / graph / kv_cache="fp8" paths the spans go straight into the static cache — no DynamicCache, no
    hand-over, and with kv_cache="fp8" the prompt's cache never exists in bf16.  Each span's attention runs on
    bf_attention_chunk_gqa (bf_attention_chunk_gqa_kv8 on the FP8 cache): `chunked_attention()` is switched on for the
    prefill and restored afterwards; a last span of at most 16 tokens runs the decode kernels.  The decode steps, the
    graph and the Generation's fields are unchanged; the values are those of another valid 16-bit route of the same
    function (attention over cached, for FP8 quantised, keys), close to, not bitwise, the whole-prompt prefill's.  Without
    keep_weights every span draws the same pinned weights again — S draws of every layer per span — so chunking is best
    combined with keep_weights.  None, or C >= T0, is the whole-prompt prefill, bit for bit; any other value raises
    ValueError.

    sliding_cache="ring" (implies static_cache; Mistral, Qwen2, Qwen3 and Gemma 2) keeps each sliding-window layer of that
    static cache as a ring buffer of C = W + 15 slots (ops.ring_slots) instead of the capacity, the key with sequence index
    j in slot j % C (kv_cache.RingStaticLayer; include/bayeformers_amd_ring.h): plan.kv_cache_bytes(..., ring=True) bytes.
    A step appends its rows with one bf_kv_ring_append launch per layer and decodes on bf_attention_decode_gqa_ring, which
    walks the same sequence-index keys as the window kernel and reads each from its slot: the Generation is bitwise the one
    static_cache=True returns.  Full-attention layers, and sliding layers whose C is not below the capacity, stay plain
    layers.  It composes with graph=True, with kv_cache="fp8" (e4m3 rings: bf_kv8_ring_append,
    bf_attention_decode_gqa_ring_kv8), keep_weights, truncation, the logits processors and soft-capping.  Nothing but
    those kernels can read a ring: a call against one that they do not take raises RuntimeError.  It is refused
    (ValueError) together with prefill_chunk — a span of more than 16 queries needs more live keys than C — and on a
    config none of whose layers would get a ring.  None (the default) changes nothing; any other value raises ValueError.

    speculative=γ (implies static_cache; needs keep_weights) is greedy speculative decoding with the posterior mean as the
    draft model: an iteration drafts γ tokens per row under `model.posterior_mean()` — the same network on one weight set,
    1/S of the weight traffic, with a bf16 cache of its own at B rows — then scores the last kept token and the γ drafts
    under the S pinned draws in ONE forward of γ + 1 queries per row (the same skinny GEMM and decode attention launches
    as a one-token step), and keeps the longest prefix the model-average argmax agrees with plus the model average's own
    next token (one bf_spec_accept launch; all rows advance together by the shortest agreeing run over the unfinished
    rows).  Both caches' fill pointers are then set back by the rejected tokens, on the device.  Every emitted token is the
    model average's argmax given the tokens before it, and the statistics are those of the verified position: the text and
    the uncertainties are those of greedy generation on another valid 16-bit route (γ + 1 queries through the decode
    kernels) — close to, not bitwise, the one-token loop's.  `Generation.speculation` counts {verify steps, drafts
    proposed, drafts accepted}.  γ must be an int in [1, DECODE_MAX_QUERIES - 1] with B * (γ + 1) <= ops.SKINNY_ROWS.  It
    composes with graph=True (the whole iteration is one captured graph; the host reads the step counter and the finished
    flags every 8 replays, and iterations past max_new_tokens write nothing), kv_cache="fp8" (the samples' cache; the
    draft's stays bf16), temperature, eos_token_id / pad_token_id, prefill_chunk, the sliding-window families on their
    full-capacity layers and soft-capping.  Refused (ValueError): no keep_weights; do_sample and the truncation
    arguments (rejection sampling against the draft is not built); the logits processors (they depend on the tokens of
    earlier positions of the same span); sliding_cache="ring" (a rejected draft's key would already have overwritten a
    live slot); group; models with a bnn.LoRALinear, a bnn.Embedding or a bnn.Experts (no posterior-mean forward yet).  None (the
    default) changes nothing, bit for bit."""
    samples, max_new_tokens = int(samples), int(max_new_tokens)
    if samples < 1:
        raise ValueError(f"sample_generate: samples={samples} (at least 1)")
    if max_new_tokens < 1:
        raise ValueError(f"sample_generate: max_new_tokens={max_new_tokens} (at least 1)")
    if not temperature > 0.0:
        raise ValueError(f"sample_generate: temperature={temperature} (must be positive)")
    gamma = _checked_speculative(speculative, input_ids, do_sample, (top_k, top_p, min_p),
                                 (repetition_penalty, no_repeat_ngram_size, min_new_tokens), sliding_cache, group,
                                 keep_weights)
    truncation = _truncation(top_k, top_p, min_p, do_sample)
    processors = _processors(repetition_penalty, no_repeat_ngram_size, min_new_tokens, eos_token_id)
    if kv_cache is not None and not (isinstance(kv_cache, str) and kv_cache == "fp8"):
        raise ValueError(f"sample_generate: kv_cache={kv_cache!r} (None or \"fp8\")")
    if sliding_cache is not None and not (isinstance(sliding_cache, str) and sliding_cache == "ring"):
        raise ValueError(f"sample_generate: sliding_cache={sliding_cache!r} (None or \"ring\")")
    if sliding_cache is not None and prefill_chunk is not None:
        raise ValueError("sample_generate: sliding_cache=\"ring\" does not take prefill_chunk: a span of more than "
                         f"{_MIN_PREFILL_CHUNK - 1} queries needs more live keys than a ring holds")
    static_cache = bool(static_cache) or bool(graph) or kv_cache is not None or sliding_cache is not None \
        or gamma is not None
    if static_cache and group is not None:
        raise ValueError("sample_generate: static_cache / graph generation runs in a single process (group must be None)")
    if group is not None:
        raise NotImplementedError("sample_generate: S-sharded generation is not supported (single process)")
    if not isinstance(model, Model):
        raise TypeError("sample_generate: model must be a bnn.Model (bayeformers_amd.to_bayesian)")
    if any(getattr(l, "local", False) for l in model.fused_children()):
        raise ValueError("sample_generate: this model runs local reparameterisation (local_reparameterization), which "
                         "draws fresh activation noise at every forward; a generated text is one weight draw per sample "
                         "— switch it off first (local_reparameterization(model, False))")
    if model.training:
        raise RuntimeError("sample_generate: put the model in eval mode (model.eval())")
    if torch.is_grad_enabled():
        raise RuntimeError("sample_generate: call it under torch.no_grad() or torch.inference_mode()")
    if input_ids.dim() != 2 or input_ids.shape[1] < 1:
        raise ValueError(f"sample_generate: input_ids must be [B, T0] with T0 >= 1 (got {tuple(input_ids.shape)})")
    if attention_mask is not None and attention_mask.shape != input_ids.shape:
        raise ValueError("sample_generate: attention_mask must have the shape of input_ids")
    from transformers import DynamicCache

    if pad_token_id is None:
        pad_token_id = eos_token_id if eos_token_id is not None else 0
    if kv_cache is not None and bfr.get_compute_dtype() != torch.bfloat16:
        raise ValueError(f"sample_generate: kv_cache=\"fp8\" needs bfloat16 compute (set_compute_dtype): at "
                         f"{bfr.get_compute_dtype()} the dequantised cache rows are not exact")
    chunk = _checked_prefill_chunk(model, prefill_chunk, input_ids.shape[1])
    if gamma is not None:
        from .nn.layers.linear import Linear

        other = sorted({type(l).__name__ for l in model.fused_children() if not isinstance(l, Linear)})
        if other:
            raise ValueError(f"sample_generate: speculative needs a posterior-mean draft, and the model's {', '.join(other)} "
                             "layers have no posterior-mean forward yet (bnn.Linear only)")
        return _generate_speculative(model, input_ids, attention_mask, samples, max_new_tokens, gamma, temperature,
                                     eos_token_id, int(pad_token_id), keep_weights, max_bytes, bool(graph), kv_cache, chunk)
    if static_cache:
        return _generate_static(model, input_ids, attention_mask, samples, max_new_tokens, do_sample, temperature,
                                eos_token_id, int(pad_token_id), generator, keep_weights, max_bytes, bool(graph),
                                truncation, processors, kv_cache, chunk, sliding_cache)
    S, n = samples, max_new_tokens
    B, T0 = input_ids.shape
    dev = input_ids.device
    inner = model.model if model.model is not None else model
    cache = DynamicCache(config=getattr(inner, "config", None))
    ids = input_ids.repeat(S, 1)
    mask = attention_mask.to(torch.long).repeat(S, 1) if attention_mask is not None else None
    # left padding: positions count the visible tokens (what the framework's generate passes)
    pos = (mask.cumsum(-1) - 1).clamp(min=0) if mask is not None else None

    sequences = torch.full((B, T0 + n), int(pad_token_id), dtype=torch.long, device=dev)
    sequences[:, :T0] = input_ids
    stats = torch.zeros((4, B, n), dtype=torch.float32, device=dev)
    lengths = torch.zeros(B, dtype=torch.long, device=dev)
    finished = torch.zeros(B, dtype=torch.bool, device=dev)
    with model.monte_carlo(S), model.pinned_samples(keep_weights=keep_weights, max_bytes=max_bytes):
        if chunk is None:
            out = model(input_ids=ids, attention_mask=mask, position_ids=pos, past_key_values=cache, use_cache=True)
            lp = model.log_prob_samples().clone()
        else:  # the prompt in spans against the DynamicCache, each under the mask up to its end
            out, lp = _chunked_prefill(model, ids, pos, (lambda b: mask[:, :b]) if mask is not None else (lambda b: None),
                                       cache, _prefill_spans(T0, chunk))
        for t in range(n):
            logits = out.logits[:, -1, :].reshape(S, B, -1)
            if temperature != 1.0:
                logits = logits.float() / temperature
            pred = mc_predictive(logits)
            choice = _processed(out, pred, processors, t, sequences, T0, S, eos_token_id, temperature)
            if do_sample:
                tok = torch.multinomial(_truncated(choice.probs, truncation), 1, generator=generator).squeeze(1)
            else:
                tok = choice.prediction
            step = torch.stack([pred.predictive_entropy, pred.expected_entropy, pred.mutual_information,
                                pred.probs.gather(1, tok[:, None]).squeeze(1)])
            if eos_token_id is not None:
                tok = torch.where(finished, torch.full_like(tok, int(pad_token_id)), tok)
                step = torch.where(finished[None, :], 0.0, step)
                lengths += (~finished).long()
                finished = finished | (tok == int(eos_token_id))
            else:
                lengths += 1
            sequences[:, T0 + t] = tok
            stats[:, :, t] = step
            if t == n - 1 or (eos_token_id is not None and bool(finished.all())):
                break
            ids = tok.repeat(S)[:, None]
            if mask is not None:
                mask = torch.cat([mask, mask.new_ones((S * B, 1))], 1)
                pos = pos[:, -1:] + 1
            out = model(input_ids=ids, attention_mask=mask, position_ids=pos, past_key_values=cache, use_cache=True)
    return Generation(sequences, stats[0], stats[1], stats[2], stats[3], lengths, lp[:, 0], lp[:, 1])


def _prefill_spans(T0: int, C: int) -> List[Tuple[int, int]]:
    """The [a, b) token spans a prompt of T0 tokens is fed in at prefill_chunk=C: C tokens each, the last one shorter."""
    if T0 < 1 or C < 1:
        raise ValueError(f"_prefill_spans: T0={T0}, C={C} (both at least 1)")
    return [(a, min(a + C, T0)) for a in range(0, T0, C)]


_MIN_PREFILL_CHUNK = 17  # (a span of at most 16 tokens is a decode step: the chunk kernels are for more)


def _checked_prefill_chunk(model: Model, prefill_chunk, T0: int) -> Optional[int]:
    """sample_generate's checked prefill_chunk: None when the prompt goes in one forward (None, or a chunk of at least T0
    tokens), else the chunk — which needs the model's attention routed through the kernels."""
    if prefill_chunk is None:
        return None
    if isinstance(prefill_chunk, bool) or not isinstance(prefill_chunk, numbers.Integral) \
            or prefill_chunk < _MIN_PREFILL_CHUNK:
        raise ValueError(f"sample_generate: prefill_chunk={prefill_chunk!r} (None or an int >= {_MIN_PREFILL_CHUNK})")
    if prefill_chunk >= T0:
        return None
    from .attention import _ATTENTION_NAME

    inner = model.model if model.model is not None else model
    if getattr(getattr(inner, "config", None), "_attn_implementation", None) != _ATTENTION_NAME:
        raise RuntimeError("sample_generate: prefill_chunk needs the model's attention routed through the HIP kernels "
                           "— call bayeformers_amd.fuse_attention(model) first")
    return int(prefill_chunk)


def _chunked_prefill(model: Model, ids: Tensor, pos: Optional[Tensor], mask_to, cache, spans):
    """The prefill of sample_generate(prefill_chunk=...): one forward per span [a, b) of the prompt against `cache`, with
    input_ids[:, a:b], position_ids[:, a:b] and the attention mask mask_to(b), under `chunked_attention()` (restored
    afterwards, also on an exception).  A span's output is dropped as soon as its forward has updated the cache; only the
    last span's is returned, with one position of logits where the wrapped model's forward takes `logits_to_keep`.
    Returns (out, lp): lp the log-probs of the pinned draws, read after the first span (every span draws the same)."""
    import inspect

    from .attention import _CHUNKED_ATTENTION

    inner = model.model if model.model is not None else model
    try:
        keep = {"logits_to_keep": 1} if "logits_to_keep" in inspect.signature(inner.forward).parameters else {}
    except (TypeError, ValueError):
        keep = {}
    before = _CHUNKED_ATTENTION[0]
    _CHUNKED_ATTENTION[0] = True
    try:
        out = lp = None
        for a, b in spans:
            out = None  # the span before: nothing of it is read
            out = model(input_ids=ids[:, a:b], attention_mask=mask_to(b), position_ids=pos[:, a:b] if pos is not None else None,
                        past_key_values=cache, use_cache=True, **keep)
            if lp is None:
                lp = model.log_prob_samples().clone()
    finally:
        _CHUNKED_ATTENTION[0] = before
    return out, lp


def _truncation(top_k, top_p, min_p, do_sample: bool) -> Optional[Tuple[Optional[int], Optional[float], Optional[float]]]:
    """sample_generate's checked (top_k, top_p, min_p), the no-op settings as None; None when all are no-ops."""
    if (top_k is not None or top_p is not None or min_p is not None) and not do_sample:
        raise ValueError("sample_generate: top_k / top_p / min_p truncate a draw: they need do_sample=True")
    if top_k is not None and (isinstance(top_k, bool) or not isinstance(top_k, numbers.Integral) or top_k < 1):
        raise ValueError(f"sample_generate: top_k={top_k!r} (an int >= 1)")
    if top_p is not None and not (isinstance(top_p, numbers.Real) and 0.0 < top_p <= 1.0):
        raise ValueError(f"sample_generate: top_p={top_p!r} (must be in (0, 1])")
    if min_p is not None and not (isinstance(min_p, numbers.Real) and 0.0 <= min_p <= 1.0):
        raise ValueError(f"sample_generate: min_p={min_p!r} (must be in [0, 1])")
    k = int(top_k) if top_k is not None else None
    p = float(top_p) if top_p is not None and top_p < 1.0 else None
    m = float(min_p) if min_p is not None and min_p > 0.0 else None
    return (k, p, m) if (k, p, m) != (None, None, None) else None


_MAX_NGRAM = 64  # bf_logits_process's cap on no_repeat_ngram_size


def _processors(repetition_penalty, no_repeat_ngram_size, min_new_tokens,
                eos_token_id) -> Optional[Tuple[float, int, int]]:
    """sample_generate's checked (repetition_penalty, no_repeat_ngram_size, min_new_tokens), the no-op settings as
    (1.0, 0, 0); None when all are no-ops."""
    theta = repetition_penalty
    if theta is not None and (isinstance(theta, bool) or not isinstance(theta, numbers.Real) or
                              not math.isfinite(theta) or not theta > 0.0):
        raise ValueError(f"sample_generate: repetition_penalty={theta!r} (must be finite and positive)")
    for name, v, hi in (("no_repeat_ngram_size", no_repeat_ngram_size, _MAX_NGRAM), ("min_new_tokens", min_new_tokens, None)):
        if v is not None and (isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < 0 or
                              (hi is not None and v > hi)):
            raise ValueError(f"sample_generate: {name}={v!r} (an int >= 0{f' and <= {hi}' if hi else ''})")
    if min_new_tokens and eos_token_id is None:
        raise ValueError("sample_generate: min_new_tokens bans eos_token_id: it needs an eos_token_id")
    p = (float(theta) if theta is not None else 1.0, int(no_repeat_ngram_size or 0), int(min_new_tokens or 0))
    return p if p != (1.0, 0, 0) else None


def _processing_at(processors, t: int) -> bool:
    """Whether step t launches the processors: a penalty or an n-gram ban acts at every step, the eos ban before
    min_new_tokens only."""
    return processors is not None and (processors[0] != 1.0 or processors[1] > 0 or t < processors[2])


def _processed(out, pred: "Predictive", processors, t, sequences: Tensor, T0: int, S: int, eos_token_id,
               temperature: float, step: Optional[Tensor] = None) -> "Predictive":
    """The predictive a step's token is chosen from: `pred` itself when no processor acts at step t, else the predictive
    of the last position's logits processed by one bf_logits_process launch (at the device step `step` when given)."""
    if not _processing_at(processors, t):
        return pred
    from . import ops

    theta, ngram, m = processors
    raw = out.logits[:, -1, :]
    processed = ops.process_logits(raw, sequences, T0, step if step is not None else t, S, theta, ngram, m,
                                   eos_token_id, temperature)
    return mc_predictive(processed.view(S, sequences.shape[0], -1))


def _truncated(probs: Tensor, truncation) -> Tensor:
    """The model-average rows [B, V] a draw samples from: truncated by one bf_probs_truncate launch, or as they are
    when every criterion is a no-op (top_k >= V included)."""
    if truncation is None:
        return probs
    top_k, top_p, min_p = truncation
    if top_k is not None and top_k >= probs.shape[-1]:
        top_k = None
    if (top_k, top_p, min_p) == (None, None, None):
        return probs
    from . import ops

    return ops.truncate_probs(probs, top_k, top_p, min_p)


_FINISHED_EVERY = 8  # graph replays between two all-finished checks (host synchronisations) of sample_generate(graph=True)


# Model families whose attention modules are known to apply the config's sliding window (they hand it to the attention
# function, which the window kernels then apply over a full-capacity cache): a family joins together with a test of its
# static / graph generation.  Others with sliding layers — a Llama config that carries layer_types, whose attention
# ignores them — stay refused.
_SLIDING_STATIC_FAMILIES = ("mistral", "qwen2", "qwen3", "gemma2")


_STATIC_LAYER_HOOK = None  # tests: a StaticLayer subclass every layer of _static_cache's cache is built from instead


def _sliding_windows(config, capacity: int) -> List[Optional[int]]:
    """Per cache layer of a decoder config, the window W of a sliding-window layer that static generation serves (the
    families of _SLIDING_STATIC_FAMILIES), None for every other layer: the layers transformers' StaticCache would build as
    sliding ones, as _static_cache finds them.  Needs no GPU (the layers allocate lazily)."""
    from transformers import StaticCache

    text = config.get_text_config(decoder=True) if hasattr(config, "get_text_config") else config
    layers = StaticCache(config=config, max_cache_len=int(capacity)).layers
    if getattr(config, "model_type", None) not in _SLIDING_STATIC_FAMILIES:
        return [None] * len(layers)
    window = getattr(text, "sliding_window", None)
    return [int(window) if getattr(layer, "is_sliding", False) and window is not None else None for layer in layers]


def _static_cache(model: Model, capacity: int, kv_cache: Optional[str] = None, sliding_cache: Optional[str] = None):
    """A transformers StaticCache of `capacity` tokens for the wrapped decoder, or the reason it cannot serve.  For the
    families of _SLIDING_STATIC_FAMILIES the sliding-window layers get plain full-capacity StaticLayers too (transformers'
    StaticSlidingWindowLayer branches on a host count and rolls its buffer, so one captured graph could not serve every
    step): the mask carries the window and the decode kernel applies it.  Such a layer holds `capacity` slots, not W.
    kv_cache="fp8": every layer is a kv_cache.Fp8StaticLayer of the same capacity (after the same refusals).
    sliding_cache="ring": a sliding layer whose ops.ring_slots(W, capacity) is below the capacity becomes a
    kv_cache.RingStaticLayer (Fp8RingStaticLayer with kv_cache="fp8") of that many slots; a config on which no layer does
    is refused."""
    from transformers import StaticCache
    from transformers.cache_utils import StaticLayer

    from .attention import _ATTENTION_NAME, softcap_attention_enabled

    inner = model.model if model.model is not None else model
    config = getattr(inner, "config", None)
    if config is None or getattr(config, "_attn_implementation", None) != _ATTENTION_NAME:
        raise RuntimeError("sample_generate: static_cache / graph need the model's attention routed through the HIP kernels "
                           "— call bayeformers_amd.fuse_attention(model) first")
    if getattr(config, "attn_logit_softcapping", None) is not None and not softcap_attention_enabled():
        # (without the switch the decode steps would run the framework's attention, which ignores the cap)
        raise RuntimeError("sample_generate: static_cache / graph on a config with attn_logit_softcapping need the "
                           "soft-cap kernels — call bayeformers_amd.softcap_attention() first")
    cache = StaticCache(config=config, max_cache_len=int(capacity))
    if getattr(config, "model_type", None) in _SLIDING_STATIC_FAMILIES:
        cache.layers = [StaticLayer(max_cache_len=int(capacity)) if getattr(layer, "is_sliding", False) else layer
                        for layer in cache.layers]
    if any(type(layer) is not StaticLayer or getattr(layer, "is_sliding", False) for layer in cache.layers):
        raise ValueError("sample_generate: static_cache / graph take full-attention decoders only (this config has "
                         "sliding-window or other non-static cache layers)")
    if kv_cache is not None and kv_cache != "fp8":
        raise ValueError(f"sample_generate: kv_cache={kv_cache!r} (None or \"fp8\")")
    if sliding_cache is not None and sliding_cache != "ring":
        raise ValueError(f"sample_generate: sliding_cache={sliding_cache!r} (None or \"ring\")")
    cls = _STATIC_LAYER_HOOK
    if cls is None and kv_cache == "fp8":
        from .kv_cache import Fp8StaticLayer as cls
    if cls is not None:
        cache.layers = [cls(max_cache_len=int(capacity)) for _ in cache.layers]
    if sliding_cache == "ring":
        from . import ops
        from .kv_cache import Fp8RingStaticLayer, RingStaticLayer

        slots = [ops.ring_slots(w, int(capacity)) for w in _sliding_windows(config, int(capacity))]
        if not any(c is not None for c in slots):
            raise ValueError("sample_generate: sliding_cache=\"ring\" would change nothing here: the config has no "
                             "sliding-window layer whose ring (window + "
                             f"{ops.DECODE_MAX_QUERIES - 1} slots) is smaller than the capacity of {int(capacity)}")
        ring = Fp8RingStaticLayer if kv_cache == "fp8" else RingStaticLayer
        cache.layers = [layer if c is None else ring(max_cache_len=int(capacity), ring_slots=c)
                        for layer, c in zip(cache.layers, slots)]
    return cache


def _generate_static(model: Model, input_ids: Tensor, attention_mask: Optional[Tensor], S: int, n: int, do_sample: bool,
                     temperature: float, eos_token_id: Optional[int], pad_token_id: int,
                     generator: Optional[torch.Generator], keep_weights: Union[bool, str], max_bytes: Optional[int],
                     graph: bool, truncation=None, processors=None, kv_cache: Optional[str] = None,
                     prefill_chunk: Optional[int] = None, sliding_cache: Optional[str] = None) -> Generation:
    """sample_generate(static_cache=True / graph=True): the prefill of the default path (a DynamicCache, copied into the
    static one), then decode steps of one shape whose bookkeeping is bf_generate_step (after bf_probs_truncate with a
    truncation: the step's inverse-CDF draw over the filtered, unnormalised row samples the renormalised kept set; with
    logits processors, bf_logits_process at the device step and a second mc_predictive choose the token, and
    bf_generate_step_stat_probs reads its probability from the unprocessed row).  prefill_chunk (checked: smaller than
    T0): the prompt goes in spans straight into the static cache instead, under the full-capacity mask — no DynamicCache.
    sliding_cache="ring": the sliding layers of the static cache are ring buffers (`_static_cache`); the hand-over's
    `update` keeps the last ring_slots rows of the prompt in their slots, and nothing else changes."""
    from transformers import DynamicCache
    from transformers.cache_utils import DynamicLayer

    from . import ops

    B, T0 = input_ids.shape
    dev = input_ids.device
    static = _static_cache(model, T0 + n - 1, kv_cache, sliding_cache)
    inner = model.model if model.model is not None else model
    seed = None
    if do_sample:  # the generation's own Philox key: one draw from the caller's generator per call
        gdev = generator.device if generator is not None else torch.device("cpu")
        seed = torch.randint(0, 2 ** 63 - 1, (1,), generator=generator, device=gdev, dtype=torch.int64).to(dev)
    ids = input_ids.repeat(S, 1)
    mask = attention_mask.to(torch.long).repeat(S, 1) if attention_mask is not None else None
    pos = (mask.cumsum(-1) - 1).clamp(min=0) if mask is not None else None

    sequences = torch.full((B, T0 + n), int(pad_token_id), dtype=torch.long, device=dev)
    sequences[:, :T0] = input_ids
    stats = torch.zeros((4, B, n), dtype=torch.float32, device=dev)
    lengths = torch.zeros(B, dtype=torch.long, device=dev)
    finished = torch.zeros(B, dtype=torch.bool, device=dev)
    state = torch.zeros(2, dtype=torch.long, device=dev)  # {step, the epilogue's arrival count}
    # the step's inputs, written in place: the ids by the epilogue, the positions advanced by it; the mask covers the whole
    # capacity at once (keys past the fill are hidden by the causal mask built from the cache's fill)
    next_ids = torch.empty((S * B, 1), dtype=torch.long, device=dev)
    if mask is not None:
        positions = pos[:, -1:].clone()
        full_mask = torch.cat([mask, mask.new_ones((S * B, n - 1))], 1)
    else:
        positions = torch.full((S * B, 1), T0 - 1, dtype=torch.long, device=dev)
        full_mask = None

    def epilogue(out, t):
        logits = out.logits[:, -1, :].reshape(S, B, -1)
        if temperature != 1.0:
            logits = logits.float() / temperature
        pred = mc_predictive(logits)
        choice = _processed(out, pred, processors, t, sequences, T0, S, eos_token_id, temperature, step=state)
        ops.generate_step(_truncated(choice.probs, truncation), pred.predictive_entropy, pred.expected_entropy, pred.mutual_information, S, state,
                          sequences, T0, stats, finished, lengths, next_ids.view(-1), positions.view(-1), eos_token_id,
                          pad_token_id, seed, stat_probs=pred.probs if choice is not pred else None)

    def decode(t):
        epilogue(model(input_ids=next_ids, attention_mask=full_mask, position_ids=positions, past_key_values=static,
                       use_cache=True), t)

    def all_finished():
        return eos_token_id is not None and bool(finished.all())

    with model.monte_carlo(S), model.pinned_samples(keep_weights=keep_weights, max_bytes=max_bytes):
        if prefill_chunk is not None:  # each span is appended at the static cache's fill pointer by its own forward
            # the layers are allocated before the first span: its mask is then built from the fill (a device scalar, 0) like
            # every later one's, and its attention reads the first `chunk` slots and not the whole capacity
            config = inner.config.get_text_config(decoder=True) if hasattr(inner.config, "get_text_config") else inner.config
            heads = int(config.num_attention_heads)
            static.early_initialization(S * B, int(getattr(config, "num_key_value_heads", None) or heads),
                                        int(getattr(config, "head_dim", None) or config.hidden_size // heads),
                                        bfr.get_compute_dtype(), dev)
            out, lp = _chunked_prefill(model, ids, pos, lambda b: full_mask, static, _prefill_spans(T0, prefill_chunk))
        else:
            dynamic = DynamicCache(config=getattr(inner, "config", None))
            # (a sliding layer of the prefill keeps every key: they go to their own slots of the full-capacity static layer)
            dynamic.layers = [DynamicLayer() if getattr(layer, "is_sliding", False) else layer for layer in dynamic.layers]
            out = model(input_ids=ids, attention_mask=mask, position_ids=pos, past_key_values=dynamic, use_cache=True)
            lp = model.log_prob_samples().clone()
            for i, layer in enumerate(dynamic.layers):  # the prompt's keys and values fill the static cache's first T0 slots
                static.update(layer.keys, layer.values, i)
                layer.keys = layer.values = None  # released as it goes: the peak is the prompt's cache plus the static one so far
            del dynamic
        epilogue(out, 0)
        del out
        t = 1
        if n > 1 and not all_finished():
            decode(1)  # eagerly: plans, workspaces and the kept weights' launches are set up outside any capture
            t = 2
        # min_new_tokens alone: eager steps until its eos ban lifts, so the captured step has the launches of every replay
        settled = processors[2] if processors is not None and processors[:2] == (1.0, 0) else 0
        while graph and t < min(n, settled) and not all_finished():
            decode(t)
            t += 1
        if graph and t < n and not all_finished():
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                decode(t)
            replays = 0
            while t < n:
                g.replay()
                t, replays = t + 1, replays + 1
                if replays % _FINISHED_EVERY == 0 and all_finished():
                    break
            del g
        while t < n and not all_finished():
            decode(t)
            t += 1
    return Generation(sequences, stats[0], stats[1], stats[2], stats[3], lengths, lp[:, 0], lp[:, 1])


# tools/speculative_bench.py: a list that, while set, makes _generate_speculative(graph=True) capture the draft steps, the
# verify forward and the accept launch as three graphs and append the four events around each iteration's replays
_SECTION_TIMES = None


def _checked_speculative(speculative, input_ids: Tensor, do_sample: bool, truncation_args, processor_args, sliding_cache,
                         group, keep_weights) -> Optional[int]:
    """sample_generate's checked speculative=γ (None: off), with everything it is refused together with; needs no device."""
    if speculative is None:
        return None
    from . import ops

    top = ops.DECODE_MAX_QUERIES - 1
    if isinstance(speculative, bool) or not isinstance(speculative, numbers.Integral) or not 1 <= speculative <= top:
        raise ValueError(f"sample_generate: speculative={speculative!r} (None or an int in [1, {top}]: a verify step "
                         f"carries γ + 1 <= {ops.DECODE_MAX_QUERIES} queries)")
    gamma = int(speculative)
    B = int(input_ids.shape[0]) if input_ids.dim() == 2 else 1
    if B * (gamma + 1) > ops.SKINNY_ROWS:
        raise ValueError(f"sample_generate: speculative={gamma} with {B} prompt rows verifies {B * (gamma + 1)} rows per "
                         f"sample: the skinny GEMM takes at most {ops.SKINNY_ROWS} (B * (γ + 1) <= {ops.SKINNY_ROWS})")
    if not keep_weights:
        raise ValueError("sample_generate: speculative needs keep_weights (True or \"fp8\"): without kept weights there is "
                         "no S-fold weight stream for the verify step to amortise")
    if do_sample:
        raise ValueError("sample_generate: speculative is greedy: do_sample=True would need rejection sampling against "
                         "the draft's distribution, which is not built")
    if any(v is not None for v in truncation_args):
        raise ValueError("sample_generate: speculative does not take top_k / top_p / min_p: they truncate a draw, and "
                         "speculation is greedy")
    if any(v is not None for v in processor_args):
        raise ValueError("sample_generate: speculative does not take repetition_penalty / no_repeat_ngram_size / "
                         "min_new_tokens: inside a verified span they depend on the tokens of its earlier positions")
    if sliding_cache is not None:
        raise ValueError("sample_generate: speculative does not take sliding_cache=\"ring\": a rejected draft's key would "
                         "already have overwritten a live slot of the ring")
    if group is not None:
        raise ValueError("sample_generate: speculative generation runs in a single process (group must be None)")
    return gamma


def _generate_speculative(model: Model, input_ids: Tensor, attention_mask: Optional[Tensor], S: int, n: int, gamma: int,
                          temperature: float, eos_token_id: Optional[int], pad_token_id: int,
                          keep_weights: Union[bool, str], max_bytes: Optional[int], graph: bool,
                          kv_cache: Optional[str] = None, prefill_chunk: Optional[int] = None) -> Generation:
    """sample_generate(speculative=γ): greedy generation by draft and verify over two static caches of capacity
    T0 + n + γ — the samples' (S·B rows, FP8 with kv_cache="fp8"), prefilled by _generate_static's routes, and the
    draft's (B rows, always 16-bit), prefilled by one posterior-mean forward and set back by one token, so that the first
    draft step of EVERY iteration feeds two tokens: the last kept one and the one after it.  (After a fully accepted run
    the last draft was never fed to the draft model; after a rejection it was, and is rewritten with the same row.)

    One iteration, of fixed shapes: γ draft steps at B rows under `posterior_mean()` (argmax, fed to the next); one verify
    forward of [S·B, γ + 1] tokens, whose [S, B·(γ+1), V] logits go through mc_predictive as one batch of rows;
    bf_spec_accept; every layer of both caches has its fill pointer lowered by the device scalar that launch wrote.  Rows
    past a fill are overwritten by the next iteration and hidden meanwhile by the causal mask, which is built from the
    fill.  The host does not know how many tokens an iteration kept: it runs (graph: replays) iterations and reads the step
    counter and the finished flags — every iteration when eager, every _FINISHED_EVERY replays with a graph; iterations
    at or past n write nothing but the rewind."""
    from transformers import DynamicCache
    from transformers.cache_utils import DynamicLayer

    from . import ops

    B, T0 = input_ids.shape
    dev = input_ids.device
    G = int(gamma)
    # a verify step at step t writes slots T0 + t - 1 .. T0 + t - 1 + γ.  The last one that emits runs at t <= n - 1; an
    # iteration replayed after the n-th token (t = n: bf_spec_accept then only rewinds) still runs its forwards, one slot on
    capacity = T0 + n + G
    static = _static_cache(model, capacity, kv_cache, None)
    draft = _static_cache(model, capacity, None, None)
    inner = model.model if model.model is not None else model
    config = inner.config.get_text_config(decoder=True) if hasattr(inner.config, "get_text_config") else inner.config
    mask1 = attention_mask.to(torch.long) if attention_mask is not None else None
    pos1 = (mask1.cumsum(-1) - 1).clamp(min=0) if mask1 is not None else None
    ids = input_ids.repeat(S, 1)
    mask = mask1.repeat(S, 1) if mask1 is not None else None
    pos = pos1.repeat(S, 1) if pos1 is not None else None

    sequences = torch.full((B, T0 + n), int(pad_token_id), dtype=torch.long, device=dev)
    sequences[:, :T0] = input_ids
    stats = torch.zeros((4, B, n), dtype=torch.float32, device=dev)
    lengths = torch.zeros(B, dtype=torch.long, device=dev)
    finished = torch.zeros(B, dtype=torch.bool, device=dev)
    state = torch.zeros(2, dtype=torch.long, device=dev)
    speculation = torch.zeros(3, dtype=torch.long, device=dev)
    rewind = torch.zeros(1, dtype=torch.long, device=dev)
    first_ids = torch.empty(S * B, dtype=torch.long, device=dev)
    verify_ids = torch.zeros((S * B, G + 1), dtype=torch.long, device=dev)
    draft_ids = torch.zeros((B, 2), dtype=torch.long, device=dev)
    drafts = torch.zeros((B, G), dtype=torch.long, device=dev)
    steps = torch.arange(G + 1, device=dev)
    # positions: the verify forward feeds the last emitted token (the one after the prompt's last, to begin with) and the γ
    # drafts; the draft steps feed the token in front of it too.  bf_spec_accept advances both by the tokens kept.
    last = pos1[:, -1:] if pos1 is not None else torch.full((B, 1), T0 - 1, dtype=torch.long, device=dev)
    draft_pos = (last + steps[None, :]).contiguous()
    verify_pos = (last + 1 + steps[None, :]).repeat(S, 1).contiguous()
    if mask is not None:
        full_mask = torch.cat([mask, mask.new_ones((S * B, capacity - T0))], 1)
        draft_mask = full_mask[:B].contiguous()
    else:
        full_mask = draft_mask = None

    def mean_forward(tokens, positions):
        with model.posterior_mean():
            return model(input_ids=tokens, attention_mask=draft_mask, position_ids=positions, past_key_values=draft,
                         use_cache=True)

    verified = [None]  # the verify forward's Predictive, read by the accept section

    def draft_steps():
        for i in range(G):  # draft step i feeds draft i - 1 (the first: the last two tokens kept) and proposes draft i
            out = mean_forward(draft_ids if i == 0 else drafts[:, i - 1:i],
                               draft_pos[:, :2] if i == 0 else draft_pos[:, i + 1:i + 2])
            drafts[:, i] = out.logits[:, -1, :].argmax(-1)
        verify_ids.view(S, B, G + 1)[:, :, 1:] = drafts

    def verify():
        out = model(input_ids=verify_ids, attention_mask=full_mask, position_ids=verify_pos, past_key_values=static,
                    use_cache=True)
        logits = out.logits.reshape(S, B * (G + 1), -1)
        if temperature != 1.0:
            logits = logits.float() / temperature
        verified[0] = mc_predictive(logits)

    def accept():
        pred = verified[0]
        ops.speculative_accept(pred.prediction.view(B, G + 1), drafts, pred.probs, pred.predictive_entropy,
                               pred.expected_entropy, pred.mutual_information, S, state, sequences, T0, stats, finished,
                               lengths, verify_ids, verify_pos, draft_ids, draft_pos, rewind, speculation, eos_token_id,
                               pad_token_id)
        for cache in (static, draft):
            for layer in cache.layers:
                layer.cumulative_length.sub_(rewind[0])

    def iteration():
        draft_steps()
        verify()
        accept()

    def done():
        if eos_token_id is not None:
            return bool((state[0] >= n) | finished.all())
        return int(state[0]) >= n

    with model.monte_carlo(S), model.pinned_samples(keep_weights=keep_weights, max_bytes=max_bytes):
        if prefill_chunk is not None:
            heads = int(config.num_attention_heads)
            static.early_initialization(S * B, int(getattr(config, "num_key_value_heads", None) or heads),
                                        int(getattr(config, "head_dim", None) or config.hidden_size // heads),
                                        bfr.get_compute_dtype(), dev)
            out, lp = _chunked_prefill(model, ids, pos, lambda b: full_mask, static, _prefill_spans(T0, prefill_chunk))
        else:
            dynamic = DynamicCache(config=getattr(inner, "config", None))
            dynamic.layers = [DynamicLayer() if getattr(layer, "is_sliding", False) else layer for layer in dynamic.layers]
            out = model(input_ids=ids, attention_mask=mask, position_ids=pos, past_key_values=dynamic, use_cache=True)
            lp = model.log_prob_samples().clone()
            for i, layer in enumerate(dynamic.layers):
                static.update(layer.keys, layer.values, i)
                layer.keys = layer.values = None
            del dynamic
        # the first token, as _generate_static's step 0 chooses it
        logits = out.logits[:, -1, :].reshape(S, B, -1)
        if temperature != 1.0:
            logits = logits.float() / temperature
        pred = mc_predictive(logits)
        ops.generate_step(pred.probs, pred.predictive_entropy, pred.expected_entropy, pred.mutual_information, S, state,
                          sequences, T0, stats, finished, lengths, first_ids, None, eos_token_id, pad_token_id)
        del out, pred
        if n > 1:
            # the draft's prompt: one posterior-mean forward at B rows (the pinned draws and the kept weights stay as they
            # are), handed to its static cache; one token back, so that the first draft step rewrites the prompt's last
            dynamic = DynamicCache(config=getattr(inner, "config", None))
            dynamic.layers = [DynamicLayer() if getattr(layer, "is_sliding", False) else layer for layer in dynamic.layers]
            with model.posterior_mean():
                model(input_ids=input_ids, attention_mask=mask1, position_ids=pos1, past_key_values=dynamic, use_cache=True)
            for i, layer in enumerate(dynamic.layers):
                draft.update(layer.keys, layer.values, i)
                layer.keys = layer.values = None
            del dynamic
            for layer in draft.layers:
                layer.cumulative_length.sub_(1)
            verify_ids[:, 0] = first_ids
            draft_ids[:, 0] = input_ids[:, -1]
            draft_ids[:, 1] = first_ids[:B]
            if not done():
                iteration()  # eagerly: plans, workspaces and the mean weights are set up outside any capture
            if graph and not done():
                # one graph for the iteration — or, when a tool asks for the time split (_SECTION_TIMES), one per section
                times = _SECTION_TIMES
                graphs = []
                for section in ((iteration,) if times is None else (draft_steps, verify, accept)):
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g, pool=graphs[0].pool() if graphs else None):
                        section()
                    graphs.append(g)
                replays = 0
                while True:  # (ends: every iteration short of n emits at least one token)
                    marks = []
                    for g in graphs:
                        if times is not None:
                            marks.append(torch.cuda.Event(enable_timing=True))
                            marks[-1].record()
                        g.replay()
                    if times is not None:
                        marks.append(torch.cuda.Event(enable_timing=True))
                        marks[-1].record()
                        times.append(marks)
                    replays += 1
                    if replays % _FINISHED_EVERY == 0 and done():
                        break
                del graphs, g
            while not done():
                iteration()
    gen = Generation(sequences, stats[0], stats[1], stats[2], stats[3], lengths, lp[:, 0], lp[:, 1])
    gen.speculation = speculation
    return gen
