"""Host side of the causal attention route (no GPU): the mask function fuse_attention registers and the causal
classification of _attention_interface."""
import ctypes

import pytest
import torch

transformers = pytest.importorskip("transformers")
from transformers.masking_utils import (bidirectional_mask_function, causal_mask_function, sdpa_mask,  # noqa: E402
                                        sliding_window_causal_mask_function)

import bayeformers_amd as bf  # noqa: E402


def _padded(B=3, T=16):
    m = torch.ones(B, T, dtype=torch.long)
    m[1, T - 5:] = 0  # right padding
    m[2, :7] = 0      # left padding
    return m


def test_causal_padding_mask_is_sdpa_mask_with_markers():
    m = _padded()
    B, T = m.shape
    got = bf._padding_mask_interface(B, q_length=T, kv_length=T, mask_function=causal_mask_function, attention_mask=m)
    ref = sdpa_mask(batch_size=B, q_length=T, kv_length=T, mask_function=causal_mask_function, attention_mask=m)
    assert got.dtype == torch.bool and got.shape == (B, 1, T, T) and torch.equal(got, ref)
    assert got._bf_causal is True
    assert torch.equal(got._bf_key_mask, torch.where(m.bool(), 0.0, float("-inf")))
    assert got._bf_key_mask.dtype == torch.float32 and got._bf_mask_off.shape == (1,) and not bool(got._bf_mask_off)
    full = bf._padding_mask_interface(B, q_length=T, kv_length=T, mask_function=causal_mask_function,
                                      attention_mask=torch.ones(B, T, dtype=torch.bool))
    assert bool(full._bf_mask_off) and torch.equal(full[:, 0], torch.ones(T, T, dtype=torch.bool).tril().expand(B, T, T))


def test_causal_without_mask_is_none():
    assert bf._padding_mask_interface(2, q_length=8, kv_length=8, mask_function=causal_mask_function) is None


@pytest.mark.parametrize("kw", [dict(q_length=8, kv_length=16), dict(q_length=8, kv_length=8, q_offset=8, kv_offset=0),
                                dict(q_length=1, kv_length=9, q_offset=8), dict(q_length=8, kv_length=8, use_vmap=True)])
def test_offsets_unequal_lengths_and_vmap_go_to_sdpa_mask(kw):
    kv = kw["kv_length"]
    m = torch.ones(2, kv, dtype=torch.long)
    m[1, :3] = 0
    got = bf._padding_mask_interface(2, mask_function=causal_mask_function, attention_mask=m, **kw)
    ref = sdpa_mask(batch_size=2, mask_function=causal_mask_function, attention_mask=m, **kw)
    assert not hasattr(got, "_bf_causal")
    assert (got is None and ref is None) or torch.equal(got, ref)


def test_sliding_window_goes_to_sdpa_mask():
    m = _padded()
    B, T = m.shape
    fn = sliding_window_causal_mask_function(4)
    got = bf._padding_mask_interface(B, q_length=T, kv_length=T, mask_function=fn, attention_mask=m)
    ref = sdpa_mask(batch_size=B, q_length=T, kv_length=T, mask_function=fn, attention_mask=m)
    assert torch.equal(got, ref) and not hasattr(got, "_bf_causal")


def test_bidirectional_branch_unchanged():
    m = _padded()
    got = bf._padding_mask_interface(3, q_length=16, kv_length=16, mask_function=bidirectional_mask_function, attention_mask=m)
    assert got.shape == (3, 1, 1, 16) and not hasattr(got, "_bf_causal")


class _Module(torch.nn.Module):
    def __init__(self, causal):
        super().__init__()
        self.is_causal = causal


def _route(monkeypatch, module, mask=None, **kwargs):
    """Which branch _attention_interface takes for CPU tensors (both end in the framework's attention here)."""
    seen = {}
    monkeypatch.setattr(bf, "_causal_attention", lambda *a, **k: seen.setdefault("causal", True) and (None, None))
    import transformers.integrations.sdpa_attention as sa

    monkeypatch.setattr(sa, "sdpa_attention_forward", lambda *a, **k: seen.setdefault("bidirectional", True) and (None, None))
    q = torch.zeros(1, 2, 128, 64)
    bf._attention_interface(module, q, q, q, mask, **kwargs)
    return "causal" if "causal" in seen else "bidirectional"


def test_causal_module_with_no_mask_is_classified_causal(monkeypatch):
    assert _route(monkeypatch, _Module(True)) == "causal"
    assert _route(monkeypatch, _Module(False)) == "bidirectional"
    assert _route(monkeypatch, _Module(False), is_causal=True) == "causal"
    assert _route(monkeypatch, _Module(True), is_causal=False) == "bidirectional"  # the explicit argument wins
    marked = torch.ones(1, 1, 128, 128, dtype=torch.bool)
    marked._bf_causal = True
    assert _route(monkeypatch, _Module(False), marked) == "causal"
    # an explicit (unmarked) mask carries its own structure: the module flag alone does not make the call causal
    assert _route(monkeypatch, _Module(True), torch.ones(1, 1, 1, 128, dtype=torch.bool)) == "bidirectional"


def test_gqa_shape_struct_matches_header():
    from bayeformers_amd import _C

    # 6 int32 + 3 x 3 int64 = 96 bytes, as a C compiler lays out bf_attn_gqa_t
    assert ctypes.sizeof(_C.bf_attn_gqa_t) == 96 and _C.bf_attn_gqa_t.q_stride.offset == 24
    assert {"bf_attention_fwd_gqa", "bf_attention_bwd_gqa"} <= set(_C.SYMBOLS)
