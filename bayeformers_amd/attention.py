"""The HuggingFace attention interface of the package: `fuse_attention` registers `_attention_interface` (which kernel
entry a call runs on) and `_padding_mask_interface` (the masks, built on the device and marked for the router), and the
switches that gate the optional entries live here.  A call is described once — the marks of its mask (`_marks_of`), its
cache and its arguments (`_describe`) — and every route below reads that record.  `ops.X` and the framework's
`sdpa_attention_forward` are looked up at call time: tests replace them."""
import os
import sys
from typing import NamedTuple, Optional

import torch

from . import ops
from . import random as bfr
from .nn.model import Model

_ATTENTION_NAME = "bayeformers_amd"
# `_causal_attention` and `_softcap_eager` are called as the package's attributes, looked up at call time like `ops.X`:
# tests and tools replace `bayeformers_amd._causal_attention` / `bayeformers_amd._softcap_eager`, which re-exports them
_package = sys.modules[__package__]


class _Marks(NamedTuple):
    """What `_padding_mask_interface` hangs on the mask it returns (all defaults: no mask, or one it did not build)."""
    key_mask: Optional[torch.Tensor] = None   # additive fp32 [N, Tk] (a ring: [N, capacity]); None: nothing is padded
    mask_off: Optional[torch.Tensor] = None   # one device byte "the key mask hides nothing"; None whenever key_mask is
    causal: bool = False                      # the cache-free causal padding mask
    decode: bool = False                      # a step or a chunk against a cache, bottom-right aligned
    kv_len: Optional[torch.Tensor] = None     # a fixed-capacity cache: its fill after this call, one int64 on the device
    window: Optional[int] = None              # a sliding-window mask
    key_origin: int = 0                       # the sequence index of key 0 (a sliding cache that kept its last keys)
    band: Optional[tuple] = None              # packed sequences: ops.band_bounds' (lo, hi)
    band_window: Optional[int] = None         # ... and their window


_UNMARKED = _Marks()


def _marks_of(attention_mask) -> _Marks:
    """The one place the marks are read."""
    if attention_mask is None:
        return _UNMARKED
    marks = attention_mask.__dict__.get  # (cheaper than nine getattr with a default; this runs in every attention call)
    key_mask = marks("_bf_key_mask")
    return _Marks._make((  # (_make: the cheapest way to build the record)
        key_mask, marks("_bf_mask_off") if key_mask is not None else None, marks("_bf_causal", False),
        bool(marks("_bf_decode", False)), marks("_bf_kv_len"), marks("_bf_window"), marks("_bf_key_origin", 0),
        marks("_bf_band"), marks("_bf_band_window")))


class _Call(NamedTuple):
    """One call of `_attention_interface`, described once."""
    marks: _Marks
    cache: str             # none | plain | kv8 | ring | ring_kv8 (kv_cache's layers mark their tensors; plain: any 16-bit cache)
    masked: bool           # the call carries a mask
    Tq: int
    Tk: int                # the rows of `key`: a ring's slots, not its capacity
    need_grad: bool
    dropout: float
    softcap: Optional[float]
    sinks: bool            # attention sinks (`s_aux`), which no kernel applies
    window_conflict: bool  # the module's `sliding_window` argument disagrees with the window of the mask
    keys_ok: bool          # no key mask, or one over every key (a ring: over its capacity)
    scale: float
    scaling: Optional[float]  # as the caller gave it: what the framework's attention is handed


def _describe(query, key, value, attention_mask, dropout, scaling, kwargs) -> _Call:
    marks = _marks_of(attention_mask)
    N, _, Tq, D = query.shape
    Tk = key.shape[2]
    held = key.__dict__.get
    ring, fp8 = held("_bf_ring"), held("_bf_kv8_scale") is not None
    if ring is not None:
        cache = "ring_kv8" if fp8 else "ring"
    elif fp8:
        cache = "kv8"
    else:  # none: the queries' own keys — no cached-step mask and equal lengths, so no cached route could take the call
        cache = "none" if Tq == Tk and marks.kv_len is None and not marks.decode else "plain"
    # (a ring's 16-bit buffers, which kernels write, are not asked; e4m3 rows cannot require a gradient)
    need_grad = torch.is_grad_enabled() and (query.requires_grad or (
        cache != "ring" and (key.requires_grad or value.requires_grad)))
    softcap = kwargs.get("softcap")
    key_mask = marks.key_mask
    return _Call._make((
        marks, cache, attention_mask is not None, Tq, Tk, need_grad, dropout,
        float(softcap) if softcap is not None else None, kwargs.get("s_aux") is not None,
        marks.window is not None and "sliding_window" in kwargs and kwargs["sliding_window"] != marks.window,
        key_mask is None or key_mask.shape == (N, Tk if ring is None else ring[1]),
        scaling if scaling is not None else D ** -0.5, scaling))


def _framework(module, query, key, value, attention_mask, call, kwargs, cast=False):
    """The framework's scaled-dot-product attention; cast: a mask that is neither bool nor of the query's dtype is
    converted first (its kernels want one of the two) — only the prefill and the encoder fallbacks ask for that."""
    from transformers.integrations.sdpa_attention import sdpa_attention_forward

    if cast and attention_mask is not None and attention_mask.dtype not in (torch.bool, query.dtype):
        attention_mask = attention_mask.to(query.dtype)
    return sdpa_attention_forward(module, query, key, value, attention_mask, dropout=call.dropout, scaling=call.scaling,
                                  **kwargs)


def _attention_interface(module, query, key, value, attention_mask, dropout: float = 0.0, scaling=None, **kwargs):
    """Attention function in the HuggingFace `AttentionInterface` convention: query/key/value [B, H, T, D], returns
    ([B, T, H, D], None).  In this order: a ring-buffer cache and an FP8 cache (kv_cache's layers mark their tensors) take
    the cached routes (`_cached_attention`); causal calls (decoders) go to `_causal_attention`, whose kernels take any
    sequence length; the rest is the encoder's (`_encoder_attention`).  What no kernel takes goes to the framework's
    scaled-dot-product attention — except where that would be wrong: a soft-capped call runs `_softcap_eager`, an FP8
    cache is dequantised first, a ring refuses."""
    call = _describe(query, key, value, attention_mask, dropout, scaling, kwargs)
    if call.cache not in ("none", "plain"):
        return _cached_attention(module, query, key, value, attention_mask, call, kwargs)
    # causal: a mask _padding_mask_interface marked causal (the mask itself carries the structure), else what the caller
    # says with is_causal, else — with no mask — the module's own flag (HF decoders set module.is_causal and pass no mask
    # when nothing is padded); an explicit is_causal wins over the module flag, as in the framework's sdpa_attention_forward
    marks, explicit = call.marks, kwargs.get("is_causal", None)
    causal = bool(marks.causal or marks.decode or marks.window is not None or marks.band is not None) or (
        bool(explicit) if explicit is not None else (attention_mask is None and bool(getattr(module, "is_causal", False))))
    if causal:
        return _package._causal_attention(module, query, key, value, attention_mask, call, **kwargs)
    return _encoder_attention(module, query, key, value, attention_mask, call, kwargs)


def _encoder_attention(module, query, key, value, attention_mask, call, kwargs):
    """The bidirectional half: bf_attention_fwd (bf_attention_bwd behind it when a gradient is needed) for head size 64,
    T a multiple of 128, no mask or a key-padding mask; attention_probs_dropout runs inside the kernels on the Philox
    keep-mask of csrc/bf_philox.h, forward and backward.  Under `encoder_ragged_attention()` (off by default) a length
    those kernels refuse runs their tail forms (bf_attention_fwd_any and its siblings) — the same masks, the same dropout
    contract, inference and training alike.  Anything else goes to the framework."""
    usable = ops.attention_supported(query, key, value)
    any_length = (not usable and encoder_ragged_attention_enabled() and ops.attention_any_supported(query, key, value))
    usable = usable or any_length
    key_mask = mask_off = None
    if usable and call.marks.key_mask is not None and call.keys_ok:
        # built once per forward by _padding_mask_interface: additive fp32 [B, T] + the device flag "hides nothing"
        key_mask, mask_off = call.marks.key_mask, call.marks.mask_off
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
        return _framework(module, query, key, value, attention_mask, call, kwargs, cast=True)
    dropout = call.dropout
    drop = ops.Dropout(dropout, bfr.STATE.seed, bfr.dropout_call(), bfr.dropout_site(module), bfr.dropout_origin(),
                       bfr.dropout_counter()) if dropout > 0.0 else None
    if any_length:
        if call.need_grad:
            return ops.AttentionAnyFn.apply(query, key, value, key_mask, mask_off, call.scale, drop), None
        return ops.attention_forward_any(query, key, value, key_mask, call.scale, mask_off, drop=drop), None
    if call.need_grad:  # training: the same kernel, with bf_attention_bwd behind it
        return ops.AttentionFn.apply(query, key, value, key_mask, mask_off, call.scale, drop), None
    return ops.attention_forward(query, key, value, key_mask, call.scale, mask_off, drop=drop), None


def _causal_attention(module, query, key, value, attention_mask, call, **kwargs):
    """The causal half, on 16-bit keys.  A packed-sequence mask without a soft-cap is `_packed_attention`'s.  Attention
    sinks (`s_aux`), a module `sliding_window` that disagrees with the mask's window, and a soft-cap while
    `softcap_attention()` is off (the default) go to the framework's scaled-dot-product attention — which does NOT apply
    the cap — on every path alike.  A call against a cache is `_cached_attention`'s; what is left, and what that declines
    on a dynamic cache, is `_prefill_attention`'s."""
    if call.marks.band is not None and call.softcap is None:
        return _packed_attention(module, query, key, value, attention_mask, call, kwargs)
    if call.window_conflict or call.sinks or (call.softcap is not None and not softcap_attention_enabled()):
        return _framework(module, query, key, value, attention_mask, call, kwargs)
    if call.cache != "none":
        out = _cached_attention(module, query, key, value, attention_mask, call, kwargs)
        if out is not None:
            return out
    return _prefill_attention(module, query, key, value, attention_mask, call, kwargs)


class _Route(NamedTuple):
    """How one kind of cached call is served (`_cached_attention`)."""
    fp8: bool                        # e4m3 rows: the entries take the two row-scale tensors after q, k, v
    strict: bool                     # a step is Tq < Tk, and a dynamic cache may serve it (see _decode_step)
    decode_supported: str            # the ops predicate of the step entry ...
    decode: str                      # ... and the entry (16-bit, dynamic cache: the same name without its "_len")
    chunk_supported: Optional[str]   # likewise for a cached chunk; None: the kind has no chunk entry
    chunk: Optional[str]
    weighed: bool                    # ops.decode_kernel_wins / ops.chunk_kernel_wins are consulted
    declined: str                    # what happens when the kernels decline: framework | eager | dequantize | refuse


# The rules that weigh a kernel against the framework's attention are consulted on the plain route alone: that attention
# does not compute a soft-cap, and nothing else reads e4m3 rows or a ring.
_ROUTES = {
    "plain": _Route(False, True, "attention_decode_supported", "attention_forward_decode_len", "attention_chunk_supported",
                    "attention_forward_chunk", True, "framework"),
    "softcap": _Route(False, True, "attention_decode_supported", "attention_forward_decode_len", "attention_chunk_supported",
                      "attention_forward_chunk", False, "eager"),
    "kv8": _Route(True, False, "attention_decode_kv8_supported", "attention_forward_decode_kv8",
                  "attention_chunk_kv8_supported", "attention_forward_chunk_kv8", False, "dequantize"),
    "ring": _Route(False, False, "attention_decode_supported", "attention_forward_decode_ring", None, None, False, "refuse"),
    "ring_kv8": _Route(True, False, "attention_decode_kv8_supported", "attention_forward_decode_ring_kv8", None, None,
                       False, "refuse"),
}


def _decode_step(call, strict: bool) -> bool:
    """Whether a call is a step for the decode entries: no gradient, no dropout and few queries against a cache.  The
    plain 16-bit caches (strict): fewer queries than keys — the 16-query bound is `ops.attention_decode_supported`'s —
    and, on a dynamic cache (no `_bf_kv_len`), no mask (one query, nothing padded) or one marked `_bf_decode`; a
    fixed-capacity cache does not look at that mark.  FP8 rows and rings: the fill `_bf_kv_len` and at most
    DECODE_MAX_QUERIES queries, stated here — `Tq <= Tk` is their `*_supported` predicate's."""
    if call.need_grad or call.dropout != 0.0:
        return False
    if not strict:
        return call.marks.kv_len is not None and call.Tq <= ops.DECODE_MAX_QUERIES
    return call.Tq < call.Tk and (call.marks.kv_len is not None or not call.masked or call.marks.decode)


def _cached_chunk(call) -> bool:
    """Whether a call is a cached chunk for the chunk entries (bf_attention_chunk_gqa and its kv8 sibling), under
    `chunked_attention()`: more than 16 new queries (fewer run the decode kernels) and no more than the keys, no gradient,
    no dropout, no attention sinks, one of _padding_mask_interface's cached-step masks (`_bf_decode`, or `_bf_kv_len` on a
    fixed-capacity cache — the first chunk into a static cache included) whose window, if any, the module's
    `sliding_window` agrees with, and no key mask or a [N, Tk] one."""
    return (chunked_attention_enabled() and call.masked and not call.need_grad and call.dropout == 0.0 and not call.sinks
            and ops.DECODE_MAX_QUERIES < call.Tq <= call.Tk and (call.marks.decode or call.marks.kv_len is not None)
            and not call.window_conflict and call.keys_ok)


def _ring_refusal(call, query, key, value, kwargs) -> Optional[str]:
    """Why the ring decode entries cannot take a call against a ring-buffer cache (None: they can, shapes permitting): a
    step carries the fill `_bf_kv_len` and the window `_bf_window`, at most 16 queries that fit the ring with the window,
    no gradient, no dropout, no sinks, a soft-cap only under `softcap_attention()`, an agreeing `sliding_window`, and no
    key mask or a [N, capacity] one."""
    slots, capacity = key._bf_ring
    marks, Tq = call.marks, call.Tq
    if getattr(value, "_bf_ring", None) != key._bf_ring:
        return "its values are not the same ring's"
    if (getattr(key, "_bf_kv8_scale", None) is None) != (getattr(value, "_bf_kv8_scale", None) is None):
        return "only one of its keys and values carries FP8 scales"
    if Tq > ops.DECODE_MAX_QUERIES:
        return (f"it carries {Tq} queries: a step takes at most {ops.DECODE_MAX_QUERIES} (a ring of window + "
                f"{ops.DECODE_MAX_QUERIES - 1} slots holds no more live keys; prefill_chunk is not supported)")
    if marks.kv_len is None or marks.window is None:
        return "its mask is not the sliding-window mask of a fixed-capacity cache (no `_bf_kv_len` or no `_bf_window`)"
    if call.need_grad:
        return "it needs a gradient"
    if call.dropout != 0.0:
        return f"it carries attention dropout ({call.dropout})"
    if call.sinks:
        return "it carries attention sinks (s_aux)"
    if call.softcap is not None and not softcap_attention_enabled():
        return "it carries a logit soft-cap with softcap_attention() off"
    if call.window_conflict:
        return f"the module's sliding_window={kwargs['sliding_window']!r} disagrees with the mask's window {marks.window}"
    if marks.window + Tq - 1 > slots:
        return f"window {marks.window} with {Tq} queries needs {marks.window + Tq - 1} slots, the ring has {slots}"
    if not call.keys_ok:
        return f"its key mask is {tuple(marks.key_mask.shape)}, not [N, capacity] = {(query.shape[0], capacity)}"
    return None


def _cached_attention(module, query, key, value, attention_mask, call, kwargs):
    """Every call against a KV cache, by its row of `_ROUTES`.  A cached chunk (`_cached_chunk`, under
    `chunked_attention()`) runs the chunk entry, a step (`_decode_step`) the decode entry — on a fixed-capacity cache with
    its fill `_bf_kv_len`, each with the mask's window, the call's soft-cap and the key mask — when the entry's
    `*_supported` predicate takes the tensors and, on the plain route, the measured rule prefers the kernel.  Otherwise:
    the plain route runs the framework's attention (the bool mask hides the keys past the fill, so it is exact over the
    whole capacity), a soft-capped call `_softcap_eager`; FP8 rows are dequantised over the whole capacity
    (ops.kv8_dequantize: correct but slow) and the call starts over on the bf16 tensors, so the framework never sees
    uint8; a ring raises RuntimeError, since any other attention would read its rows as if they lay in sequence order.
    Returns None for a dynamic 16-bit cache it declines: `_prefill_attention` judges that call."""
    name = "softcap" if call.cache == "plain" and call.softcap is not None else call.cache
    route, marks = _ROUTES[name], call.marks
    why = None
    if route.declined == "refuse":
        why = _ring_refusal(call, query, key, value, kwargs)
    elif route.fp8 and getattr(value, "_bf_kv8_scale", None) is None:
        raise ValueError("bayeformers_amd: the keys of this call are FP8 cache rows but its values carry no scales")
    # sinks, a disagreeing window and a cap with its switch off: _causal_attention sent them to the framework before
    # this, a ring has just refused them, so this is the FP8 cache's way to the dequantised call
    clean = why is None and not (call.sinks or call.window_conflict
                                 or (call.softcap is not None and not softcap_attention_enabled()))
    entry = None
    if clean and route.chunk is not None and _cached_chunk(call) and getattr(ops, route.chunk_supported)(query, key, value) \
            and (not route.weighed or ops.chunk_kernel_wins(query.shape[1], key.shape[1], call.Tq, call.Tk, query.shape[3],
                                                            marks.window)):
        entry, more = route.chunk, {"key_origin": marks.key_origin}
    elif clean and _decode_step(call, route.strict) and call.keys_ok \
            and getattr(ops, route.decode_supported)(query, key, value) \
            and (not route.weighed or ops.decode_kernel_wins(
                query.shape[1], key.shape[1], call.Tq,
                # the keys a step reads: all Tk, or with a window the ~W + Tq - 1 some query sees
                call.Tk if marks.window is None else min(call.Tk, marks.window + call.Tq - 1), query.shape[3])):
        entry, more = route.decode, {}
        if route.declined == "refuse":
            more["ring_slots"], more["capacity"] = key._bf_ring
    if entry is not None:
        args = (query, key, value, key._bf_kv8_scale, value._bf_kv8_scale) if route.fp8 else (query, key, value)
        if marks.kv_len is None and entry == "attention_forward_decode_len":
            entry = "attention_forward_decode"  # a dynamic cache: every row is filled
        else:
            args += (marks.kv_len,)
        if name != "plain":  # (the plain route has no cap, and does not hand its entries an absent one)
            more["softcap"] = call.softcap
        return getattr(ops, entry)(*args, marks.key_mask, call.scale, marks.mask_off, window=marks.window, **more), None
    if route.declined == "refuse":
        raise RuntimeError("bayeformers_amd: the keys of this call are a ring-buffer cache (sliding_cache=\"ring\"), which only "
                           "the ring decode kernels read, and "
                           + (why or f"bf_attention_decode_gqa_{name} does not take its shapes, dtypes or strides"))
    if route.declined == "dequantize":
        return _attention_interface(module, query, ops.kv8_dequantize(key, key._bf_kv8_scale),
                                    ops.kv8_dequantize(value, value._bf_kv8_scale), attention_mask, call.dropout,
                                    call.scaling, **kwargs)
    if marks.kv_len is None:
        return None
    if route.declined == "eager":
        return _package._softcap_eager(module, query, key, value, attention_mask, call.dropout, call.scale, call.softcap), None
    return _framework(module, query, key, value, attention_mask, call, kwargs)


def _prefill_attention(module, query, key, value, attention_mask, call, kwargs):
    """Cache-free causal calls (prefill, training): bf_attention_fwd_gqa (bf_attention_bwd_gqa behind it) for equal query
    and key lengths — any length: one that is no multiple of 128 runs the kernels' tail forms, unless
    `ragged_attention(False)` or BF_NO_RAGGED_ATTENTION sends it to the framework — without dropout, with no mask, the
    sliding mask (`_bf_window`: the window siblings) or the causal padding mask, and with the call's soft-cap (the
    soft-cap entries).  Without a cap ops.prefill_kernel_wins is asked first (head size 256: a full-attention forward
    without gradients and without a mask stays on the framework's is_causal form, which measured faster); with one it is
    not, since the framework's attention does not compute that function.  Everything else — longer cached chunks the
    chunk entries did not take and a dynamic cache's declined steps included — goes to the framework's attention, a
    soft-capped call to `_softcap_eager`."""
    marks, T, window, softcap = call.marks, call.Tq, call.marks.window, call.softcap
    usable = (call.dropout == 0.0 and T == call.Tk and (T % 128 == 0 or ragged_attention_enabled())
              and ops.attention_supported(query, key, value, causal=True, kv_heads=key.shape[1])
              and (softcap is not None or ops.prefill_kernel_wins(query.shape[1], key.shape[1], T, query.shape[3],
                                                                  call.need_grad, window, masked=call.masked))
              # no mask, the sliding mask (key mask None: nothing padded) or the causal padding mask
              and (not call.masked or window is not None or (marks.causal and marks.key_mask is not None))
              and call.keys_ok)
    if not usable:
        if softcap is not None:
            return _package._softcap_eager(module, query, key, value, attention_mask, call.dropout, call.scale, softcap), None
        return _framework(module, query, key, value, attention_mask, call, kwargs, cast=True)
    if call.need_grad:
        return ops.AttentionGqaFn.apply(query, key, value, marks.key_mask, marks.mask_off, call.scale, True, window,
                                        softcap), None
    cap = {} if softcap is None else {"softcap": softcap}
    return ops.attention_forward_gqa(query, key, value, marks.key_mask, call.scale, True, marks.mask_off, window=window,
                                     **cap), None


def _packed_attention(module, query, key, value, attention_mask, call, kwargs):
    """_causal_attention for a packed-sequence mask (`_bf_band = (lo, hi)`, `_bf_band_window`: `_packed_mask`), without
    soft-capping: bf_attention_fwd_gqa_band (bf_attention_bwd_gqa_band behind it when a gradient is needed) under
    `packed_attention()`, for equal query and key lengths of any size (subject to `ragged_attention`) and the shapes
    ops.attention_supported takes.  Attention sinks (`s_aux`), a `sliding_window` argument that disagrees with the band's
    window (here a band without one disagrees with any — `window_conflict` asks only masks that carry `_bf_window`),
    attention dropout, unsupported shapes and the classes ops.prefill_kernel_wins sends there run the framework's
    scaled-dot-product attention over the dense mask."""
    (lo, hi), window = call.marks.band, call.marks.band_window
    B, H, T, D = query.shape
    usable = (packed_attention_enabled() and not call.sinks
              and not ("sliding_window" in kwargs and kwargs["sliding_window"] != window)
              and call.dropout == 0.0 and T == call.Tk and (T % 128 == 0 or ragged_attention_enabled())
              and ops.attention_supported(query, key, value, causal=True, kv_heads=key.shape[1])
              and tuple(lo.shape) == (B, T) and tuple(hi.shape) == (B, T)
              and ops.prefill_kernel_wins(H, key.shape[1], T, D, call.need_grad, window, masked=True))
    if not usable:
        return _framework(module, query, key, value, attention_mask, call, kwargs)
    if call.need_grad:
        return ops.AttentionGqaBandFn.apply(query, key, value, lo, hi, call.scale), None
    return ops.attention_forward_gqa_band(query, key, value, lo, call.scale), None


def _softcap_eager(module, query, key, value, attention_mask, dropout, scaling, softcap):
    """What a soft-capped call runs when no kernel takes it: the model's own eager chain (transformers' gemma2
    eager_attention_forward: repeat_kv, matmul, `/ softcap`, tanh, `* softcap`, `+ mask`, fp32 softmax, dropout, matmul) in
    plain torch.  The mask arrives in the SDPA format (bool, True = visible) and is turned into the additive one the chain
    adds; no mask means causal, bottom-right aligned (the module's is_causal).  Returns [B, Tq, H, D]."""
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
        out = _with_keys(tri, _visible(attention_mask), batch_size, q_length, kv_length)
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
    visible = _visible(attention_mask[:, kv_offset:kv_offset + kv_length] if attention_mask is not None else None)
    out = _with_keys(tri, visible, batch_size, q_length, kv_length)
    if q_length < kv_length:
        out._bf_decode = True  # a step against a cache (bottom-right aligned)
    out._bf_window = window
    out._bf_key_origin = kv_offset  # the sequence index of key 0 (a sliding cache kept its last keys): the chunk entries' tile grid
    return out


def _visible(padding):
    """A 2-D padding mask as bool, True = a real token (None stays None)."""
    return padding if padding is None or padding.dtype == torch.bool else padding != 0


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

    two_d = not kwargs.get("use_vmap", False) and (attention_mask is None or (
        attention_mask.dim() == 2 and attention_mask.shape == (batch_size, kv_length)))  # a 2-D padding mask or none
    if (mask_function is causal_mask_function and isinstance(q_offset, torch.Tensor) and kv_offset == 0
            and q_length is not None and kv_length is not None and 0 < q_length <= kv_length and two_d):
        # a fixed-capacity cache (transformers' StaticLayer: q_offset is its fill count, a device tensor, and kv_length its
        # capacity).  Tested before the comparisons below: on a tensor they synchronise with the host (or fail a capture).
        # Query i sees keys 0 .. q_offset + i, which hides the keys past the fill; the snapshot kv_len is the fill after
        # this forward's update (the cache bumps its counter in place during the forward)
        device = q_offset.device
        keys = torch.arange(kv_length, device=device)
        tri = keys[None, :] <= (q_offset.reshape(()) + torch.arange(q_length, device=device))[:, None]
        out = _with_keys(tri, _visible(attention_mask), batch_size, q_length, kv_length)
        out._bf_decode = True
        out._bf_kv_len = (q_offset.reshape(()) + q_length).reshape(1)
        return out

    if (mask_function is causal_mask_function and kv_offset == 0 and q_length is not None and kv_length is not None
            and 0 < q_length < kv_length and q_offset == kv_length - q_length and two_d):
        if attention_mask is None and q_length == 1:
            return None  # the new query sees every cached key: module.is_causal routes the call
        device = attention_mask.device if attention_mask is not None else kwargs.get("device", "cpu")
        keys = torch.arange(kv_length, device=device)
        tri = keys[None, :] <= torch.arange(q_offset, kv_length, device=device)[:, None]  # query i sees 0 .. q_offset + i
        out = _with_keys(tri, _visible(attention_mask), batch_size, q_length, kv_length)
        out._bf_decode = True  # causal, bottom-right aligned (_bf_causal stays the cache-free marker)
        return out

    if mask_function is causal_mask_function and q_offset == 0 and kv_offset == 0 and q_length == kv_length and two_d:
        # a decoder's causal mask over the cache-free sequence: None when nothing is padded (the framework's answer too:
        # the attention is then causal by module.is_causal); with a padding mask, sdpa_mask's [B, 1, T, T] bool mask built
        # on the device without a host round trip, carrying the key mask and "causal" for bf_attention_fwd_gqa
        if attention_mask is None:
            return None
        tri = torch.ones((q_length, kv_length), dtype=torch.bool, device=attention_mask.device).tril()
        out = _with_keys(tri, _visible(attention_mask), batch_size, q_length, kv_length)
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
    visible = _visible(attention_mask)
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
    from . import _install_pooled_last_layer  # (the package module imports this one)

    _install_pooled_last_layer(inner)
    return True
