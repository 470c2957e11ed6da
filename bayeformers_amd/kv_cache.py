"""The FP8 KV cache of sample_generate(kv_cache="fp8"): a transformers StaticLayer whose keys and values are e4m3 rows
(include/bayeformers_amd_kv8.h) — D bytes and one fp32 power-of-two scale per cached K or V row, 2 D + 8 bytes a row pair
against 4 D in bf16."""
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
