"""Host-side parts of static-cache / graph-replayed generation: sample_generate's refusals, the fixed-capacity mask of
_padding_mask_interface, the C entries' argument refusals and the generation Philox stream."""
import ctypes

import pytest
import torch
from transformers.masking_utils import causal_mask_function, sdpa_mask

import bayeformers_amd as bf
import bayeformers_amd.nn as bnn
from bayeformers_amd import _C
from bayeformers_amd.sampling import sample_generate


def _llama(fuse=True, **kw):
    from transformers import LlamaConfig, LlamaForCausalLM

    cfg = LlamaConfig(hidden_size=64, num_attention_heads=2, num_key_value_heads=1, num_hidden_layers=2,
                      intermediate_size=128, vocab_size=64, max_position_embeddings=64, attn_implementation="sdpa", **kw)
    torch.manual_seed(0)
    model = bf.to_bayesian(LlamaForCausalLM(cfg).eval(), delta=0.05, freeze=True).eval()
    if fuse:
        assert bf.fuse_attention(model)
    return model


@pytest.mark.parametrize("kw", [dict(static_cache=True), dict(graph=True)])
def test_static_generation_refuses_a_group(kw):
    with torch.no_grad(), pytest.raises(ValueError, match="single process"):
        sample_generate(_llama(), torch.zeros(1, 4, dtype=torch.long), samples=2, max_new_tokens=3, group=object(), **kw)


@pytest.mark.parametrize("kw", [dict(static_cache=True), dict(graph=True)])
def test_static_generation_needs_fuse_attention(kw):
    with torch.no_grad(), pytest.raises(RuntimeError, match="fuse_attention"):
        sample_generate(_llama(fuse=False), torch.zeros(1, 4, dtype=torch.long), samples=2, max_new_tokens=3, **kw)


@pytest.mark.parametrize("kw", [dict(static_cache=True), dict(graph=True)])
def test_static_generation_refuses_sliding_window_layers(kw):
    model = _llama(layer_types=["sliding_attention", "full_attention"], sliding_window=8)
    with torch.no_grad(), pytest.raises(ValueError, match="sliding"):
        sample_generate(model, torch.zeros(1, 4, dtype=torch.long), samples=2, max_new_tokens=3, **kw)


def test_static_generation_keeps_the_existing_refusals():
    tiny = bnn.Model(torch.nn.Linear(4, 4)).eval()
    with torch.no_grad(), pytest.raises(ValueError):
        sample_generate(tiny, torch.zeros(1, 4, dtype=torch.long), samples=0, graph=True)
    with pytest.raises(RuntimeError, match="no_grad"):
        sample_generate(_llama(), torch.zeros(1, 4, dtype=torch.long), samples=2, graph=True)


def _padded(B=2, T=12):
    m = torch.ones(B, T, dtype=torch.long)
    m[1, :3] = 0
    return m


@pytest.mark.parametrize("q_length", [1, 3])
@pytest.mark.parametrize("padded", [False, True])
def test_static_cache_mask(q_length, padded):
    """q_offset a tensor (a StaticLayer's fill), kv_length the capacity: the mask is causal from the fill, hides the keys
    past it and carries a snapshot of the fill after the step."""
    cap, fill = 12, 7
    m = _padded(T=cap) if padded else None
    offset = torch.tensor(fill)
    got = bf._padding_mask_interface(2, q_length=q_length, kv_length=cap, q_offset=offset,
                                     mask_function=causal_mask_function, attention_mask=m)
    ref = sdpa_mask(batch_size=2, q_length=q_length, kv_length=cap, q_offset=fill, mask_function=causal_mask_function,
                    attention_mask=m, allow_is_causal_skip=False)
    assert got.shape == (2, 1, q_length, cap) and torch.equal(got, ref)
    assert not got[..., fill + q_length:].any()  # nothing past the fill
    assert got._bf_decode is True and got._bf_kv_len.dtype == torch.int64 and got._bf_kv_len.tolist() == [fill + q_length]
    offset += 1  # the cache's update bumps its counter in place: the snapshot stays
    assert got._bf_kv_len.tolist() == [fill + q_length]
    if padded:
        assert torch.equal(got._bf_key_mask, torch.where(m.bool(), 0.0, float("-inf")))
        assert not bool(got._bf_mask_off)
    else:
        assert got._bf_key_mask is None and got._bf_mask_off is None


def _shape(N=2, Tq=1, Tk=100, H=8, Hkv=2, D=64):
    s = _C.bf_attn_decode_t(N, Tq, Tk, H, Hkv, D)
    for name, st in (("q_stride", (Tq * H * D, D, H * D)), ("k_stride", (Hkv * Tk * D, Tk * D, D)),
                     ("v_stride", (Hkv * Tk * D, Tk * D, D))):
        getattr(s, name)[:] = st
    return s


@pytest.mark.parametrize("kw", [dict(D=96), dict(Tq=17, Tk=100), dict(H=6, Hkv=4), dict(Tq=4, Tk=2)])
def test_decode_len_entry_refuses_shapes(kw):
    lib = _C.lib()
    rc = lib.bf_attention_decode_gqa_len(16, 16, 16, None, None, 16, 16, None, _C.BF_DT_BF16,
                                         ctypes.byref(_shape(**kw)), 0.125, None)
    assert rc != 0 and lib.bf_last_error()


@pytest.mark.parametrize("kv_len", [None, 12])
def test_decode_len_entry_needs_an_aligned_length(kv_len):
    lib = _C.lib()
    rc = lib.bf_attention_decode_gqa_len(16, 16, 16, None, None, kv_len, 16, None, _C.BF_DT_BF16,
                                         ctypes.byref(_shape()), 0.125, None)
    assert rc != 0 and b"kv_len" in lib.bf_last_error()


def _step_args(**kw):
    a = dict(probs=16, pe=16, ee=16, mi=16, B=2, V=64, S=2, state=16, n=4, seq=16, seq_stride=12, T0=8, stats=16,
             finished=16, lengths=16, next_ids=16, positions=16, eos=3, pad=0, do_sample=0, seed=None)
    a.update(kw)
    return list(a.values()) + [None]


@pytest.mark.parametrize("kw,what", [(dict(B=0), b"positive"), (dict(V=1 << 20), b"exceeds"), (dict(seq_stride=11), b"hold"),
                                     (dict(probs=None), b"NULL"), (dict(finished=None), b"finished"),
                                     (dict(do_sample=1), b"seed"), (dict(state=12), b"aligned")])
def test_generate_step_entry_refuses(kw, what):
    lib = _C.lib()
    assert lib.bf_generate_step(*_step_args(**kw)) != 0 and what in lib.bf_last_error()


def test_generate_stream_is_its_own():
    """The generation stream sits beside the weight streams (2 * layer + {0, 1}) and the dropout streams (bit 31)."""
    import re
    from pathlib import Path

    text = (Path(bf.__file__).parent / "csrc" / "bf_philox.h").read_text()
    stream = int(re.search(r"#define BF_GENERATE_STREAM (0x[0-9A-Fa-f]+)u", text).group(1), 16)
    dropout = int(re.search(r"#define BF_DROPOUT_STREAM (0x[0-9A-Fa-f]+)u", text).group(1), 16)
    assert stream & dropout == 0 and stream >= 1 << 20
