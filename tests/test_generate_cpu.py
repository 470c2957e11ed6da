"""Host-side parts of Monte-Carlo generation: sample_generate's argument checks, attention_decode_supported, the C entries'
shape refusals, Model.pinned_samples on the host counter and the cached-call mask of _padding_mask_interface."""
import ctypes

import pytest
import torch
from transformers.masking_utils import causal_mask_function, sdpa_mask

import bayeformers_amd as bf
import bayeformers_amd.nn as bnn
from bayeformers_amd import _C, ops
from bayeformers_amd import random as bfr
from bayeformers_amd.sampling import sample_generate


class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.lin = bnn.Linear(32, 8)

    def forward(self, x):
        return self.lin(x)


def _model():
    return bnn.Model(_Tiny()).eval()


@pytest.mark.parametrize("kw,exc", [(dict(samples=0), ValueError), (dict(max_new_tokens=0), ValueError),
                                    (dict(do_sample=True, temperature=0.0), ValueError),
                                    (dict(temperature=-1.0), ValueError), (dict(group=object()), NotImplementedError)])
def test_sample_generate_rejects_arguments(kw, exc):
    args = dict(samples=2, max_new_tokens=3)
    args.update(kw)
    with torch.no_grad(), pytest.raises(exc):
        sample_generate(_model(), torch.zeros(1, 4, dtype=torch.long), **args)


def test_sample_generate_needs_eval_and_no_grad():
    with pytest.raises(RuntimeError, match="eval"):
        with torch.no_grad():
            sample_generate(_model().train(), torch.zeros(1, 4, dtype=torch.long), samples=2, max_new_tokens=2)
    with pytest.raises(RuntimeError, match="no_grad"):
        sample_generate(_model(), torch.zeros(1, 4, dtype=torch.long), samples=2, max_new_tokens=2)


def _qkv(N=2, H=8, Hkv=2, Tq=1, Tk=100, D=64, dtype=torch.bfloat16, device="meta"):
    q = torch.empty(N, Tq, H, D, dtype=dtype, device=device).transpose(1, 2)
    k = torch.empty(N, Hkv, Tk, D, dtype=dtype, device=device)
    return q, k, torch.empty_like(k)


@pytest.mark.parametrize("kw,ok", [(dict(), True), (dict(D=128, H=32, Hkv=8, Tq=16, Tk=16), True), (dict(Hkv=1), True),
                                   (dict(Tq=4, Tk=1), False), (dict(D=96), False), (dict(Tq=17, Tk=100), False),
                                   (dict(H=6, Hkv=4), False), (dict(dtype=torch.float32), False)])
def test_attention_decode_supported_verdicts(kw, ok):
    q, k, v = _qkv(**kw)
    assert ops.attention_decode_supported(q, k, v, check_device=False) is ok
    assert ops.attention_decode_supported(q, k, v) is False  # not on a ROCm device
    qc, kc, vc = _qkv(device="cpu", **kw)
    assert ops.attention_decode_supported(qc, kc, vc, check_device=False) is ok
    assert ops.attention_decode_supported(qc, kc, vc) is False


def test_attention_decode_supported_needs_contiguous_features():
    q, k, v = _qkv()
    kt = torch.empty(2, 2, 64, 100, dtype=torch.bfloat16, device="meta").transpose(2, 3)
    assert not ops.attention_decode_supported(q, kt, v, check_device=False)


def _shape(N=2, Tq=1, Tk=100, H=8, Hkv=2, D=64):
    s = _C.bf_attn_decode_t(N, Tq, Tk, H, Hkv, D)
    for name, st in (("q_stride", (Tq * H * D, D, H * D)), ("k_stride", (Hkv * Tk * D, Tk * D, D)),
                     ("v_stride", (Hkv * Tk * D, Tk * D, D))):
        getattr(s, name)[:] = st
    return s


@pytest.mark.parametrize("kw", [dict(D=96), dict(Tq=17, Tk=100), dict(H=6, Hkv=4), dict(Tq=4, Tk=2)])
def test_c_entry_refuses(kw):
    lib = _C.lib()
    s = _shape(**kw)
    assert lib.bf_attention_decode_workspace_bytes(ctypes.byref(s)) == -1
    rc = lib.bf_attention_decode_gqa(16, 16, 16, None, None, 16, None, _C.BF_DT_BF16, ctypes.byref(s), 0.125, None)
    assert rc != 0 and lib.bf_last_error()


def test_workspace_is_a_function_of_the_shape():
    lib = _C.lib()
    assert lib.bf_attention_decode_workspace_bytes(ctypes.byref(_shape(Tk=100))) == 0  # one split: no partials
    long = lib.bf_attention_decode_workspace_bytes(ctypes.byref(_shape(Tk=16384, D=128)))
    assert long > 0 and long == lib.bf_attention_decode_workspace_bytes(ctypes.byref(_shape(Tk=16384, D=128)))


def test_pinned_samples_reserves_once_and_commits_once(monkeypatch):
    calls = {"reserve": [], "commit": []}
    real_reserve, real_commit = bfr.reserve_samples, bfr.commit_samples
    monkeypatch.setattr(bfr, "reserve_samples", lambda n: calls["reserve"].append(n) or real_reserve(n))
    monkeypatch.setattr(bfr, "commit_samples", lambda n: calls["commit"].append(n) or real_commit(n))
    bf.manual_seed(1, next_sample=40)
    model = bnn.Model(torch.nn.Linear(4, 4)).eval()  # no kernel layer: its forwards run on the CPU
    x = torch.randn(6, 4)
    with model.monte_carlo(3):
        with model.pinned_samples():
            assert model._pinned == (40, 0, 3)
            assert bfr.STATE.next_sample == 43
            for _ in range(4):
                with torch.no_grad():
                    model(x)
                assert model._last_base == 40
            with pytest.raises(RuntimeError):
                with model.pinned_samples():
                    pass
        assert model.__dict__.get("_pinned") is None
        with torch.no_grad():
            model(x)  # outside the block: fresh indices again
        assert model._last_base == 43
    assert calls == {"reserve": [3, 3], "commit": [3, 3]}
    assert bfr.STATE.next_sample == 46


def _padded(B=2, T=9):
    m = torch.ones(B, T, dtype=torch.long)
    m[1, :3] = 0
    return m


@pytest.mark.parametrize("q_length", [1, 4])
def test_cached_mask_carries_the_decode_key_mask(q_length):
    kv = 9
    m = _padded(T=kv)
    got = bf._padding_mask_interface(2, q_length=q_length, kv_length=kv, q_offset=kv - q_length,
                                     mask_function=causal_mask_function, attention_mask=m)
    ref = sdpa_mask(batch_size=2, q_length=q_length, kv_length=kv, q_offset=kv - q_length,
                    mask_function=causal_mask_function, attention_mask=m)
    assert torch.equal(got, ref)  # what the framework's attention takes when the kernel does not apply
    assert got._bf_decode is True and not hasattr(got, "_bf_causal")
    assert torch.equal(got._bf_key_mask, torch.where(m.bool(), 0.0, float("-inf")))
    assert got._bf_key_mask.dtype == torch.float32 and got._bf_mask_off.shape == (1,) and not bool(got._bf_mask_off)


def test_cached_mask_without_padding():
    assert bf._padding_mask_interface(2, q_length=1, kv_length=9, q_offset=8, mask_function=causal_mask_function) is None
    got = bf._padding_mask_interface(2, q_length=3, kv_length=9, q_offset=6, mask_function=causal_mask_function)
    ref = sdpa_mask(batch_size=2, q_length=3, kv_length=9, q_offset=6, mask_function=causal_mask_function)
    assert torch.equal(got, ref) and got._bf_decode is True and got._bf_key_mask is None


def test_decode_dispatch_carves_out_the_measured_loss():
    assert not ops.decode_kernel_wins(16, 16, 1, 512, 128)  # MHA, one query, short cache: SDPA measured faster
    assert ops.decode_kernel_wins(16, 16, 1, 4096, 128) and ops.decode_kernel_wins(16, 16, 4, 512, 128)
    assert ops.decode_kernel_wins(16, 4, 1, 512, 128) and ops.decode_kernel_wins(16, 16, 1, 512, 64)
