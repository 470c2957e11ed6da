"""The route table of the attention interface: which entry `bf._attention_interface` hands each call to, and with what.

    python tests/golden/make_attention_routes.py        # rewrites tests/golden/attention_routes.json

A full grid of calls on small CPU tensors (no sampling), the masks built by `bf._padding_mask_interface`.  Every kernel
entry (`ops.attention_forward_*`, `ops.Attention*Fn.apply`), `ops.kv8_dequantize`, `_softcap_eager` and the framework's
`sdpa_attention_forward` is replaced by a recorder; the `*_supported` predicates judge shapes, dtypes and strides without
asking for a device; the `*_kernel_wins` rules are the real ones.  A case's outcome is the chain of recorders it reached
(an FP8 call that dequantises re-enters the interface) or the exception it raised, each recorder with every non-tensor
argument and, for tensor arguments, whether one was passed ("T." and its dtype) or None.  The file is only ever
regenerated on purpose: tests/test_attention_routes_cpu.py replays the grid against it, so a refactor of the routing
must reproduce it unchanged.

The grid (N 2, Tk 48, H 8, bf16):
  kind      none (cache-free), dynamic, fixed (fixed capacity), kv8 (FP8), ring, ring_kv8 — and, beyond the decoder grid,
            packed (restarting position ids) and encoder (bidirectional)
  Tq        1, 4, 16, 17, 40, Tk          window   none, 8, 64 (>= Tk)        padding mask   no, yes
  softcap   none, set with softcap_attention() on, set with it off            need_grad, dropout 0 / 0.1, s_aux
  sliding_window kwarg   absent, agreeing, disagreeing                        chunked_attention() on / off
  shape     (H / Hkv, D) = (8/8, 64), (8/8, 256), (8/2, 256)
Pruned, because the call cannot be constructed (never because of its outcome):
  * none, packed, encoder: Tq = Tk only — without a cache the queries and the keys are the same tokens;
  * dynamic: Tq < Tk only — Tq = Tk against an empty dynamic cache is the cache-free call, kind none;
  * ring, ring_kv8: window 8 only — ops.ring_slots makes a ring only for a window with window + 15 < capacity; a layer
    without one, or with window 64, is a plain fixed-capacity layer (kinds fixed and kv8);
  * packed: no padding mask — transformers builds the packed mask only when no attention mask is given;
  * encoder: no window, softcap, s_aux, sliding_window or chunked axis — a bidirectional layer has no such argument;
    instead encoder_ragged_attention() on / off, since Tk 48 is no multiple of 128; head size 64 only, as the encoder
    kernels take no other (the three shapes would all record the same refusal);
  * (8/2, 64) is left out as redundant: no rule reads H / Hkv at head size 64 (decode_kernel_wins reads it at 128 only,
    prefill_kernel_wins and chunk_kernel_wins at 256 only), which keeps the table under its size limit.
"""
import inspect
import itertools
import json
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))  # the repository root, when run as a script

import bayeformers_amd as bf  # noqa: E402
from bayeformers_amd import ops  # noqa: E402

JSON_PATH = os.path.join(HERE, "attention_routes.json")

N, TK, H = 2, 48, 8
RING_WINDOW, RING_SLOTS = 8, 8 + ops.DECODE_MAX_QUERIES - 1
KINDS = ("none", "dynamic", "fixed", "kv8", "ring", "ring_kv8", "packed", "encoder")
TQS = (1, 4, 16, 17, 40, TK)
WINDOWS = (None, 8, 64)
SOFTCAPS = ("none", "on", "off")  # a softcap of 30.0 with the switch on / off
SLIDING_KWARGS = ("absent", "agree", "disagree")
SHAPES = ((8, 64), (8, 256), (2, 256))  # (Hkv, D)
AXES = ("kind", "Tq", "window", "pad", "shape", "softcap", "need_grad", "dropout", "s_aux", "sliding_window", "chunked")

FORWARDS = ("attention_forward", "attention_forward_any", "attention_forward_gqa", "attention_forward_gqa_band",
            "attention_forward_decode", "attention_forward_decode_len", "attention_forward_decode_kv8",
            "attention_forward_decode_ring", "attention_forward_decode_ring_kv8", "attention_forward_chunk",
            "attention_forward_chunk_kv8")
FUNCTIONS = ("AttentionFn", "AttentionAnyFn", "AttentionGqaFn", "AttentionGqaBandFn")
SUPPORTED = ("attention_decode_supported", "attention_decode_kv8_supported", "attention_chunk_supported",
             "attention_chunk_kv8_supported")


def cases():
    """Every case of the grid, in the order the JSON lists their outcomes."""
    for kind in KINDS:
        cache_free = kind in ("none", "packed", "encoder")
        for Tq, window, pad, shape in itertools.product(TQS, WINDOWS, (False, True), SHAPES):
            if (cache_free and Tq != TK) or (kind == "dynamic" and Tq == TK):
                continue
            if kind in ("ring", "ring_kv8") and window != RING_WINDOW:
                continue
            if kind == "packed" and pad:
                continue
            if kind == "encoder":
                if window is not None or shape != SHAPES[0]:
                    continue
                for need_grad, dropout, ragged in itertools.product((False, True), (0.0, 0.1), (False, True)):
                    yield dict(kind=kind, Tq=Tq, window=None, pad=pad, shape=shape, softcap="none", need_grad=need_grad,
                               dropout=dropout, s_aux=False, sliding_window="absent", chunked=ragged)  # chunked: the ragged switch
                continue
            for softcap, need_grad, dropout, s_aux, sliding, chunked in itertools.product(
                    SOFTCAPS, (False, True), (0.0, 0.1), (False, True), SLIDING_KWARGS, (False, True)):
                yield dict(kind=kind, Tq=Tq, window=window, pad=pad, shape=shape, softcap=softcap, need_grad=need_grad,
                           dropout=dropout, s_aux=s_aux, sliding_window=sliding, chunked=chunked)


def _mask(kind, Tq, window, pad):
    """The mask `_padding_mask_interface` builds for the case, as transformers would ask for it."""
    from transformers import masking_utils as mu

    padding = None
    if pad:
        padding = torch.ones(N, TK, dtype=torch.long)
        padding[1, :3] = 0  # left padding, as generation uses it
    if kind == "encoder":
        return bf._padding_mask_interface(N, TK, TK, 0, 0, mu.bidirectional_mask_function, padding)
    fn = mu.causal_mask_function if window is None else mu.sliding_window_causal_mask_function(window)
    if kind == "packed":
        ids = torch.zeros(N, TK, dtype=torch.long)
        ids[:, 20:] = 1  # two documents per row
        return bf._padding_mask_interface(N, TK, TK, 0, 0, mu.and_masks(fn, mu.packed_sequence_mask_function(ids)), None)
    if kind in ("none", "dynamic"):
        return bf._padding_mask_interface(N, Tq, TK, TK - Tq, 0, fn, padding)
    return bf._padding_mask_interface(N, Tq, TK, torch.tensor(TK - Tq), 0, fn, padding)  # the fill before the step, on the device


def _tensors(kind, Tq, shape, need_grad):
    Hkv, D = shape
    q = torch.zeros(N, Tq, H, D, dtype=torch.bfloat16).transpose(1, 2)  # the [B, H, T, D] view HF's projections give
    if need_grad:
        q.requires_grad_(True)
    if kind in ("none", "packed", "encoder"):
        k, v = (torch.zeros(N, TK, Hkv, D, dtype=torch.bfloat16).transpose(1, 2) for _ in range(2))
        return q, k, v
    rows = RING_SLOTS if kind in ("ring", "ring_kv8") else TK
    fp8 = kind in ("kv8", "ring_kv8")
    k, v = (torch.zeros(N, Hkv, rows, D, dtype=torch.uint8 if fp8 else torch.bfloat16) for _ in range(2))
    if fp8:
        k._bf_kv8_scale, v._bf_kv8_scale = (torch.ones(N, Hkv, rows) for _ in range(2))
    if rows != TK:
        k._bf_ring = v._bf_ring = (RING_SLOTS, TK)
    return q, k, v


def _show(x):
    if isinstance(x, torch.Tensor):
        return "T." + str(x.dtype).split(".")[-1]
    if isinstance(x, float):
        return repr(round(x, 6))
    if isinstance(x, (tuple, list)):
        return "(" + ",".join(_show(y) for y in x) + ")"
    if isinstance(x, ops.Dropout):
        return f"Dropout({x.p})"
    if isinstance(x, types.SimpleNamespace):
        return "module"
    return repr(x)


class Recorder:
    """Replaces the entries for as long as it is entered; `events` collects what the running case reached."""

    def __init__(self):
        self.events, self._undo = [], []

    def _set(self, owner, name, new):
        self._undo.append((owner, name, getattr(owner, name)))
        setattr(owner, name, new)

    def _record(self, name, real, skip, result):
        """A stand-in for `real` (or for what has that signature) that notes its arguments past the first `skip` (by name, defaults filled in)."""
        sig = real if isinstance(real, inspect.Signature) else inspect.signature(real)

        def stub(*args, **kwargs):
            bound = sig.bind(*args, **kwargs)
            bound.apply_defaults()
            shown = []
            for key, value in list(bound.arguments.items())[skip:]:
                if sig.parameters[key].kind is inspect.Parameter.VAR_KEYWORD:
                    shown += [f"{k}={_show(v)}" for k, v in sorted(value.items())]
                else:
                    shown.append(f"{key}={_show(value)}")
            self.events.append(f"{name}({', '.join(shown)})")
            return result(*args, **kwargs)

        return stub

    def __enter__(self):
        import transformers.integrations.sdpa_attention as sa

        def out(q, *a, **k):
            return torch.zeros(q.shape[0], q.shape[2], q.shape[1], q.shape[3], dtype=q.dtype)

        for name in FORWARDS:
            self._set(ops, name, self._record(name, getattr(ops, name), 3, out))
        for name in FUNCTIONS:  # forward(ctx, q, k, v, ...): apply takes it without the ctx
            real = getattr(ops, name)
            sig = inspect.signature(real.forward)
            bare = sig.replace(parameters=list(sig.parameters.values())[1:])
            self._set(ops, name, types.SimpleNamespace(apply=self._record(name + ".apply", bare, 3, out)))
        self._set(ops, "kv8_dequantize", self._record(
            "kv8_dequantize", ops.kv8_dequantize, 2, lambda q, scale, out=None: torch.zeros(q.shape, dtype=torch.bfloat16)))
        self._set(bf, "_softcap_eager", self._record("_softcap_eager", bf._softcap_eager, 4, lambda m, q, *a, **k: out(q)))
        self._set(sa, "sdpa_attention_forward", self._record(
            "sdpa_attention_forward", sa.sdpa_attention_forward, 4, lambda m, q, *a, **k: (out(q), None)))
        for name in SUPPORTED:
            real = getattr(ops, name)
            self._set(ops, name, lambda q, k, v, check_device=True, real=real: real(q, k, v, False))
        self._set(ops, "attention_supported", lambda q, k, v, causal=False, kv_heads=None: (
            (causal or kv_heads is not None) and q.dtype == k.dtype == v.dtype == torch.bfloat16
            and ops._gqa_supported(q, k, v, kv_heads)))  # non-causal: Tk 48 is below the encoder kernels' 128
        self._set(ops, "attention_any_supported", lambda q, k, v: (
            q.dtype == k.dtype == v.dtype == torch.bfloat16 and q.shape == k.shape == v.shape and q.shape[3] == 64
            and all(t.stride() == (TK * H * 64, 64, H * 64, 1) for t in (q, k, v))))
        return self

    def __exit__(self, *exc):
        for owner, name, old in reversed(self._undo):
            setattr(owner, name, old)


def run_case(rec, masks, case):
    """The outcome of one case: the recorders it reached, in order, or the exception."""
    kind, Tq, window = case["kind"], case["Tq"], case["window"]
    key = (kind, Tq, window, case["pad"])
    if key not in masks:
        masks[key] = _mask(*key)
    q, k, v = _tensors(kind, Tq, case["shape"], case["need_grad"])
    kwargs = {}
    if case["softcap"] != "none":
        kwargs["softcap"] = 30.0
    if case["s_aux"]:
        kwargs["s_aux"] = torch.zeros(H)
    if case["sliding_window"] != "absent":
        kwargs["sliding_window"] = window if case["sliding_window"] == "agree" else (window or 0) + 1
    module = types.SimpleNamespace(is_causal=kind != "encoder", training=case["dropout"] > 0.0)
    bf.softcap_attention(case["softcap"] == "on")
    (bf.encoder_ragged_attention if kind == "encoder" else bf.chunked_attention)(case["chunked"])
    rec.events.clear()
    try:
        with torch.enable_grad():
            bf._attention_interface(module, q, k, v, masks[key], dropout=case["dropout"], **kwargs)
    except Exception as e:  # noqa: BLE001  (the exception is the outcome)
        rec.events.append(f"{type(e).__name__}: {e}")
    finally:
        bf.softcap_attention(False)
        bf.chunked_attention(False)
        bf.encoder_ragged_attention(False)
    return " -> ".join(rec.events)


def replay():
    """(the distinct outcomes, in order of first appearance; for each case of cases(), the index of its outcome)."""
    outcomes, rows, masks = {}, [], {}
    with Recorder() as rec:
        for case in cases():
            rows.append(outcomes.setdefault(run_case(rec, masks, case), len(outcomes)))
    return list(outcomes), rows


def main():
    outcomes, rows = replay()
    # the commonest outcomes get the shortest numbers: one number per case is most of the file
    order = sorted(range(len(outcomes)), key=lambda i: (-rows.count(i), i))
    rank = {old: new for new, old in enumerate(order)}
    with open(JSON_PATH, "w") as f:
        f.write('{"axes": %s,\n "cases": %d,\n "outcomes": [\n  %s\n ],\n "rows": [%s]}\n' % (
            json.dumps(AXES), len(rows), ",\n  ".join(json.dumps(outcomes[i]) for i in order),
            ",".join(str(rank[i]) for i in rows)))
    print(f"{len(rows)} cases, {len(outcomes)} distinct outcomes, {os.path.getsize(JSON_PATH)} bytes -> {JSON_PATH}")


if __name__ == "__main__":
    sys.exit(main())
