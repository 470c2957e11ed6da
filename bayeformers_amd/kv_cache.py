"""The cache layers of sample_generate beside transformers' own.  The FP8 KV cache of kv_cache="fp8": a transformers
StaticLayer whose keys and values are e4m3 rows (include/bayeformers_amd_kv8.h) — D bytes and one fp32 power-of-two scale
per cached K or V row, 2 D + 8 bytes a row pair against 4 D in bf16.  The ring-buffer layers of sliding_cache="ring"
(include/bayeformers_amd_ring.h): a sliding-window layer that holds ring_slots rows instead of the capacity, the key with
sequence index j in row j % ring_slots, in 16 bits or as e4m3 rows."""
import torch
from transformers.cache_utils import StaticLayer

from . import ops


class Fp8StaticLayer(StaticLayer):
    """StaticLayer on e4m3 rows.  `keys` / `values` are uint8 [N, Hkv, capacity, D] and carry their scales [N, Hkv, capacity]
    fp32 as `_bf_kv8_scale`, the marker `_attention_interface` recognises an FP8-cache call by; `update` quantises the new
    rows at the fill pointer with one bf_kv8_append launch (the pointer is read on the device, so a captured update serves
    every step).  Mask sizes and the sequence length are StaticLayer's: the fixed-capacity mask of
    `_padding_mask_interface` serves it unchanged.  bfloat16 keys and values only."""

    def lazy_initialization(self, key_states: torch.Tensor, value_states: torch.Tensor) -> None:
        if key_states.dtype != torch.bfloat16 or value_states.dtype != torch.bfloat16:
            raise ValueError(f"Fp8StaticLayer: keys and values must be bfloat16 (got {key_states.dtype}): the dequantised rows "
                             "are exact in bfloat16 alone")
        if key_states.shape[-1] != value_states.shape[-1]:
            raise ValueError("Fp8StaticLayer: keys and values must share one head size")
        self.dtype, self.device = key_states.dtype, key_states.device
        self.batch_size, self.num_heads = key_states.shape[:2]
        self.k_head_dim = self.v_head_dim = key_states.shape[-1]
        rows = (self.batch_size, self.num_heads, self.max_cache_len)
        self.keys = torch.zeros(rows + (self.k_head_dim,), dtype=torch.uint8, device=self.device)
        self.values = torch.zeros(rows + (self.v_head_dim,), dtype=torch.uint8, device=self.device)
        self.key_scales = torch.zeros(rows, dtype=torch.float32, device=self.device)
        self.value_scales = torch.zeros(rows, dtype=torch.float32, device=self.device)
        self.keys._bf_kv8_scale, self.values._bf_kv8_scale = self.key_scales, self.value_scales
        self.cumulative_length = self.cumulative_length.to(self.device)
        for t in (self.keys, self.values, self.key_scales, self.value_scales, self.cumulative_length):
            torch._dynamo.mark_static_address(t)
        self.is_initialized = True

    def update(self, key_states: torch.Tensor, value_states: torch.Tensor, *args, **kwargs):
        if not self.is_initialized:
            self.lazy_initialization(key_states, value_states)
        ops.kv8_append(key_states, value_states, self.keys, self.values, self.key_scales, self.value_scales,
                       self.cumulative_length)
        self.cumulative_length.add_(key_states.shape[-2])
        return self.keys, self.values

    def store_bytes(self) -> int:
        """Device bytes of the layer's four tensors (0 before the first update)."""
        if not self.is_initialized:
            return 0
        return sum(t.numel() * t.element_size() for t in (self.keys, self.values, self.key_scales, self.value_scales))


class RingStaticLayer(StaticLayer):
    """StaticLayer of a sliding-window layer on a ring buffer.  `max_cache_len` stays the logical capacity — the mask sizes
    and the sequence length are StaticLayer's, so the fixed-capacity masks of `_padding_mask_interface` serve it unchanged,
    over sequence indices — while `keys` / `values` are [N, Hkv, ring_slots, D] and hold the key with sequence index j in
    row j % ring_slots (ops.ring_slots: the window plus the most queries a step carries, less one).  They carry the marker
    `_bf_ring = (ring_slots, capacity)` `_attention_interface` recognises a ring call by: nothing but the ring decode
    entries can read them.  `update` is one bf_kv_ring_append launch at the fill pointer `cumulative_length` — read on the
    device, counting every appended row, never wrapping — so a captured update serves every step; of more than ring_slots
    rows (the prompt's hand-over) the last ring_slots are kept.  bfloat16 or float16."""

    def __init__(self, max_cache_len: int, ring_slots: int, **kwargs):
        super().__init__(max_cache_len=max_cache_len, **kwargs)
        self.ring_slots = int(ring_slots)
        if not 1 <= self.ring_slots < int(max_cache_len):
            raise ValueError(f"RingStaticLayer: ring_slots={ring_slots} must be in [1, max_cache_len={max_cache_len}) — a "
                             "ring of the whole capacity is a plain StaticLayer")

    def _rows(self, key_states: torch.Tensor, value_states: torch.Tensor):
        if key_states.shape[-1] != value_states.shape[-1]:
            raise ValueError(f"{type(self).__name__}: keys and values must share one head size")
        self.dtype, self.device = key_states.dtype, key_states.device
        self.batch_size, self.num_heads = key_states.shape[:2]
        self.k_head_dim = self.v_head_dim = key_states.shape[-1]
        return (self.batch_size, self.num_heads, self.ring_slots)

    def _mark(self, *tensors) -> None:
        self.keys._bf_ring = self.values._bf_ring = (self.ring_slots, int(self.max_cache_len))
        self.cumulative_length = self.cumulative_length.to(self.device)
        for t in tensors + (self.cumulative_length,):
            torch._dynamo.mark_static_address(t)
        self.is_initialized = True

    def lazy_initialization(self, key_states: torch.Tensor, value_states: torch.Tensor) -> None:
        if key_states.dtype not in (torch.bfloat16, torch.float16) or value_states.dtype != key_states.dtype:
            raise ValueError(f"RingStaticLayer: keys and values must share bfloat16 or float16 (got {key_states.dtype}, "
                             f"{value_states.dtype})")
        rows = self._rows(key_states, value_states)
        self.keys = torch.zeros(rows + (self.k_head_dim,), dtype=self.dtype, device=self.device)
        self.values = torch.zeros(rows + (self.v_head_dim,), dtype=self.dtype, device=self.device)
        self._mark(self.keys, self.values)

    def update(self, key_states: torch.Tensor, value_states: torch.Tensor, *args, **kwargs):
        if not self.is_initialized:
            self.lazy_initialization(key_states, value_states)
        ops.kv_ring_append(key_states, value_states, self.keys, self.values, self.cumulative_length)
        self.cumulative_length.add_(key_states.shape[-2])
        return self.keys, self.values

    def store_bytes(self) -> int:
        """Device bytes of the layer's tensors (0 before the first update)."""
        if not self.is_initialized:
            return 0
        return sum(t.numel() * t.element_size() for t in (self.keys, self.values))


class Fp8RingStaticLayer(RingStaticLayer):
    """RingStaticLayer on e4m3 rows: Fp8StaticLayer's tensors with ring_slots rows — `keys` / `values` uint8
    [N, Hkv, ring_slots, D] carrying their scales [N, Hkv, ring_slots] fp32 as `_bf_kv8_scale` beside `_bf_ring` — and one
    bf_kv8_ring_append launch per `update`.  bfloat16 keys and values only."""

    def lazy_initialization(self, key_states: torch.Tensor, value_states: torch.Tensor) -> None:
        if key_states.dtype != torch.bfloat16 or value_states.dtype != torch.bfloat16:
            raise ValueError(f"Fp8RingStaticLayer: keys and values must be bfloat16 (got {key_states.dtype}): the "
                             "dequantised rows are exact in bfloat16 alone")
        rows = self._rows(key_states, value_states)
        self.keys = torch.zeros(rows + (self.k_head_dim,), dtype=torch.uint8, device=self.device)
        self.values = torch.zeros(rows + (self.v_head_dim,), dtype=torch.uint8, device=self.device)
        self.key_scales = torch.zeros(rows, dtype=torch.float32, device=self.device)
        self.value_scales = torch.zeros(rows, dtype=torch.float32, device=self.device)
        self.keys._bf_kv8_scale, self.values._bf_kv8_scale = self.key_scales, self.value_scales
        self._mark(self.keys, self.values, self.key_scales, self.value_scales)

    def update(self, key_states: torch.Tensor, value_states: torch.Tensor, *args, **kwargs):
        if not self.is_initialized:
            self.lazy_initialization(key_states, value_states)
        ops.kv8_ring_append(key_states, value_states, self.keys, self.values, self.key_scales, self.value_scales,
                            self.cumulative_length)
        self.cumulative_length.add_(key_states.shape[-2])
        return self.keys, self.values

    def store_bytes(self) -> int:
        if not self.is_initialized:
            return 0
        return sum(t.numel() * t.element_size() for t in (self.keys, self.values, self.key_scales, self.value_scales))
