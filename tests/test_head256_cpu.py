"""Host side of head size 256 (no GPU): the support predicates, the routing of calls that carry logit soft-capping or
attention sinks, and a Gemma 3 decoder's layers through fuse_attention."""
import pytest
import torch

transformers = pytest.importorskip("transformers")

import bayeformers_amd as bf  # noqa: E402
from bayeformers_amd import ops  # noqa: E402


def _qkv(D, T=16, Tk=None, H=4, Hkv=2, dtype=torch.bfloat16):
    Tk = T if Tk is None else Tk
    return (torch.zeros(1, H, T, D, dtype=dtype), torch.zeros(1, Hkv, Tk, D, dtype=dtype),
            torch.zeros(1, Hkv, Tk, D, dtype=dtype))


@pytest.mark.parametrize("D,ok", [(64, True), (128, True), (256, True), (96, False), (512, False)])
def test_support_predicates_take_head_size_256(D, ok):
    q, k, v = _qkv(D)
    assert ops._gqa_supported(q, k, v, 2) is ok
    q, k, v = _qkv(D, T=1, Tk=40)
    assert ops.attention_decode_supported(q, k, v, check_device=False) is ok
    assert not ops.attention_decode_supported(q.float(), k.float(), v.float(), check_device=False)  # fp32 stays refused


def test_decode_rule_has_a_head_256_verdict():
    # a verdict for every class the measurement covers (profiles/head256_attention.md); the 64 / 128 rule is unchanged
    for H, Hkv in ((8, 4), (8, 8), (16, 8), (4, 1)):
        for Tq in (1, 4, 16):
            for Tk in (512, 4096, 32768):
                assert isinstance(ops.decode_kernel_wins(H, Hkv, Tq, Tk, 256), bool)
    assert not ops.decode_kernel_wins(8, 8, 1, 512, 128) and ops.decode_kernel_wins(8, 8, 1, 1024, 128)
    assert ops.decode_kernel_wins(8, 2, 1, 512, 64)


# ---------------------------------------------------------------------------------------------------- routing
# (the fixture of tests/test_sliding_window_cpu.py, with the fixed-capacity entry recorded too)
@pytest.fixture
def launches(monkeypatch):
    """Pretend the kernels apply to CPU tensors and record which entry each call takes, with its window."""
    seen = []
    monkeypatch.setattr(ops, "attention_supported", lambda *a, **k: True)
    monkeypatch.setattr(ops, "attention_decode_supported", lambda *a, **k: True)
    monkeypatch.setattr(ops, "decode_kernel_wins", lambda *a, **k: True)

    def zeros(q):
        return torch.zeros(q.shape[0], q.shape[2], q.shape[1], q.shape[3], dtype=q.dtype)

    def fwd(q, k, v, key_mask, scaling, causal=True, mask_off=None, want_lse=False, window=None):
        seen.append(("gqa", window))
        return zeros(q)

    def dec(q, k, v, key_mask, scaling, mask_off=None, workspace=None, window=None):
        seen.append(("decode", window))
        return zeros(q)

    def dec_len(q, k, v, kv_len, key_mask, scaling, mask_off=None, workspace=None, window=None):
        seen.append(("decode_len", window))
        return zeros(q)

    import transformers.integrations.sdpa_attention as sa

    real_sdpa = sa.sdpa_attention_forward

    def sdpa(*a, **k):
        seen.append(("sdpa", None))
        k.pop("s_aux", None), k.pop("softcap", None)  # (what the framework's function does with them is not at issue)
        return real_sdpa(*a, **k)

    monkeypatch.setattr(ops, "attention_forward_gqa", fwd)
    monkeypatch.setattr(ops, "attention_forward_decode", dec)
    monkeypatch.setattr(ops, "attention_forward_decode_len", dec_len)
    monkeypatch.setattr(sa, "sdpa_attention_forward", sdpa)
    return seen


def _module():
    mod = torch.nn.Module()
    mod.is_causal = True
    return mod


EXTRAS = [dict(softcap=30.0), dict(s_aux=torch.zeros(2))]


@pytest.mark.parametrize("kw", EXTRAS, ids=["softcap", "s_aux"])
def test_softcap_and_sinks_without_a_window_go_to_sdpa_in_prefill(launches, kw):
    q = torch.zeros(1, 2, 128, 32)
    k = q[:, :1]
    bf._attention_interface(_module(), q, k, k, None, **kw)
    assert launches == [("sdpa", None)]
    bf._attention_interface(_module(), q, k, k, None, softcap=None, s_aux=None)
    assert launches[-1] == ("gqa", None)
    # ... and with the causal padding mask _padding_mask_interface builds
    from transformers.masking_utils import causal_mask_function

    pad = torch.ones(1, 128, dtype=torch.long)
    pad[0, 120:] = 0
    mask = bf._padding_mask_interface(1, q_length=128, kv_length=128, mask_function=causal_mask_function, attention_mask=pad)
    assert getattr(mask, "_bf_causal", False)
    del launches[:]
    bf._attention_interface(_module(), q, k, k, mask, **kw)
    bf._attention_interface(_module(), q, k, k, mask)
    assert launches == [("sdpa", None), ("gqa", None)]


@pytest.mark.parametrize("kw", EXTRAS, ids=["softcap", "s_aux"])
def test_softcap_and_sinks_without_a_window_go_to_sdpa_in_a_cached_step(launches, kw):
    q, k = torch.zeros(1, 2, 1, 32), torch.zeros(1, 1, 40, 32)
    bf._attention_interface(_module(), q, k, k, None, **kw)
    assert launches == [("sdpa", None)]
    bf._attention_interface(_module(), q, k, k, None)
    assert launches[-1] == ("decode", None)


@pytest.mark.parametrize("kw", EXTRAS, ids=["softcap", "s_aux"])
def test_softcap_and_sinks_go_to_sdpa_on_a_fixed_capacity_cache(launches, kw):
    from transformers.masking_utils import causal_mask_function

    q, k = torch.zeros(1, 2, 1, 32), torch.zeros(1, 1, 40, 32)
    mask = bf._padding_mask_interface(1, q_length=1, kv_length=40, q_offset=torch.tensor(7),
                                      mask_function=causal_mask_function, attention_mask=None, allow_is_causal_skip=False)
    assert getattr(mask, "_bf_kv_len", None) is not None
    bf._attention_interface(_module(), q, k, k, mask, **kw)
    assert launches == [("sdpa", None)]
    bf._attention_interface(_module(), q, k, k, mask)
    assert launches[-1] == ("decode_len", None)


def test_gemma3_head_256_layers_route_sliding_then_full(monkeypatch):
    """The real shape predicate and the real dispatch rules decide (on CPU tensors: shapes, dtypes, strides and
    alignment); only the device check and the launch are replaced.  With gradients (a training step) the sliding layer
    takes the window entry and the full layer the plain one, and so they do without gradients when the batch carries an
    attention mask; without gradients and without a mask the full layer's forward stays on SDPA's
    is_causal form, where profiles/head256_attention.md measured it faster (ops.prefill_kernel_wins)."""
    from transformers import AutoConfig, AutoModelForCausalLM

    import transformers.integrations.sdpa_attention as sa

    seen = []
    monkeypatch.setattr(ops, "attention_supported",
                        lambda q, k, v, causal=False, kv_heads=None: ops._gqa_supported(q, k, v, kv_heads))

    def fwd(q, k, v, key_mask, scaling, causal=True, mask_off=None, want_lse=False, window=None):
        seen.append(("gqa", window))
        out = torch.zeros(q.shape[0], q.shape[2], q.shape[1], q.shape[3], dtype=q.dtype)
        return (out, torch.zeros(q.shape[:3])) if want_lse else out

    real_sdpa = sa.sdpa_attention_forward

    def sdpa(*a, **k):
        seen.append(("sdpa", None))
        return real_sdpa(*a, **k)

    monkeypatch.setattr(ops, "attention_forward_gqa", fwd)
    monkeypatch.setattr(sa, "sdpa_attention_forward", sdpa)
    W = 48
    cfg = AutoConfig.for_model("gemma3_text", hidden_size=64, num_attention_heads=4, num_key_value_heads=2, head_dim=256,
                               num_hidden_layers=2, intermediate_size=128, vocab_size=64, max_position_embeddings=512,
                               sliding_window=W, layer_types=["sliding_attention", "full_attention"],
                               attn_implementation="sdpa")
    torch.manual_seed(0)
    model = AutoModelForCausalLM.from_config(cfg).eval().to(torch.bfloat16)
    assert type(model).__name__ == "Gemma3ForCausalLM" and model.model.layers[0].self_attn.head_dim == 256
    assert bf.fuse_attention(model)
    ids = torch.zeros(1, 128, dtype=torch.long)
    model(ids, use_cache=False)  # gradients recorded: ops.AttentionGqaFn, whose forward is the patched launch
    assert seen == [("gqa", W), ("gqa", None)]
    del seen[:]
    with torch.no_grad():
        model(ids, attention_mask=torch.ones_like(ids), use_cache=False)  # a tokenizer's batch: the fallback would run a dense mask
        assert seen == [("gqa", W), ("gqa", None)]
        del seen[:]
        model(ids, use_cache=False)
    assert seen == [("gqa", W), ("sdpa", None)]


def test_prefill_rule_keeps_head_64_and_128_on_the_kernels():
    for D in (64, 128):
        for T in (100, 512, 8192):
            for backward in (False, True):
                for masked in (False, True):
                    assert ops.prefill_kernel_wins(8, 4, T, D, backward, masked=masked)
                    assert ops.prefill_kernel_wins(8, 4, T, D, backward, 48, masked)
    # head size 256, class by class as profiles/head256_attention.md measured them
    win = ops.prefill_kernel_wins
    assert all(win(8, 4, T, 256, False, W) for T, W in ((512, 256), (2048, 512), (8192, 1024), (8192, 4096)))
    assert all(win(H, Hkv, T, 256, True, masked=m) for H, Hkv in ((8, 4), (16, 16), (8, 1)) for T in (512, 2048, 8192)
               for m in (False, True) if (Hkv, T, m) != (1, 512, True))
    assert not win(8, 1, 512, 256, True, masked=True)
    assert all(win(H, Hkv, T, 256, False, masked=True) for H, Hkv in ((8, 4), (16, 16), (8, 1)) for T in (512, 2048, 8192)
               if (H, T) != (16, 512))
    assert win(8, 4, 256, 256, False, masked=True) and not win(16, 16, 512, 256, False, masked=True)
    assert not any(win(H, Hkv, T, 256, False) for H, Hkv in ((8, 4), (16, 16), (8, 1)) for T in (256, 512, 2048, 8192))
    assert not win(8, 4, 512, 256, False, 512)  # a window that hides nothing is the unmasked class
