"""Host side of the decoder blocks' backward (no GPU): the float64 restatement of the three backward formulas against
torch.autograd.grad through transformers' own code, the C-ABI entries' bindings and argument checks."""
import ctypes

import pytest
import torch

import bayeformers_amd as bf
from bayeformers_amd import _C, ops
from decoder_blocks_bwd_ref import add_rmsnorm_bwd_ref, rope_bwd_ref, swiglu_bwd_ref
from decoder_blocks_ref import rope_ref


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


# ----------------------------------------------------------------------- the restatement is autograd of HF's arithmetic
def test_rmsnorm_backward_reference_equals_autograd_in_float64():
    """The add in front of LlamaRMSNorm, both outputs used (w1 weighs y, w2 the sum: dz_in).  The module upcasts to
    float32 inside whatever it is given, so autograd through the module itself agrees to float32's 1e-6 only; through its
    forward restated line for line in float64, to 1e-11."""
    pytest.importorskip("transformers")
    from transformers.models.llama.modeling_llama import LlamaRMSNorm

    g = torch.Generator().manual_seed(31)
    x = torch.randn(5, 7, 96, generator=g, dtype=torch.float64, requires_grad=True)
    res = torch.randn(5, 7, 96, generator=g, dtype=torch.float64, requires_grad=True)
    w1, w2 = (torch.randn(5, 7, 96, generator=g, dtype=torch.float64) for _ in range(2))
    norm = LlamaRMSNorm(96, eps=1e-5).double()
    with torch.no_grad():
        norm.weight.copy_(torch.randn(96, generator=g, dtype=torch.float64))
    for forward, tol in ((norm, 2e-6),
                         (lambda h: norm.weight * (h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + norm.variance_epsilon)), 1e-11)):
        for use_sum in (True, False):
            h = res + x
            loss = (forward(h) * w1).sum() + ((h * w2).sum() if use_sum else 0.0)
            gx, gr, gg = torch.autograd.grad(loss, (x, res, norm.weight))
            dz, dgamma, mag, mag_g = add_rmsnorm_bwd_ref(h.detach(), norm.weight.detach(), w1, norm.variance_epsilon,
                                                         dz_in=w2 if use_sum else None)
            assert torch.equal(gx, gr)  # dz is the gradient of x and of the residual alike
            assert _rel(dz, gx) < tol and _rel(dgamma, gg) < tol
            assert bool((mag >= dz.abs() * (1 - 1e-12)).all()) and bool((mag_g >= dgamma.abs() * (1 - 1e-12)).all())


def test_rope_backward_reference_equals_autograd_in_float64():
    pytest.importorskip("transformers")
    from transformers.models.llama.modeling_llama import apply_rotary_pos_emb

    g = torch.Generator().manual_seed(32)
    B, H, Hkv, T, D = 2, 4, 2, 9, 64
    q = torch.randn(B, H, T, D, generator=g, dtype=torch.float64, requires_grad=True)
    k = torch.randn(B, Hkv, T, D, generator=g, dtype=torch.float64, requires_grad=True)
    wq, wk = torch.randn(B, H, T, D, generator=g, dtype=torch.float64), torch.randn(B, Hkv, T, D, generator=g, dtype=torch.float64)
    half = torch.randn(B, T, D // 2, generator=g, dtype=torch.float64)
    equal = torch.cat((half, half), -1)                                    # what a rotary module returns
    unequal = torch.randn(B, T, D, generator=g, dtype=torch.float64)       # tables whose two halves differ
    for ang in (equal, unequal, unequal[:1]):
        cos, sin = ang.cos(), ang.sin()
        hq, hk = apply_rotary_pos_emb(q, k, cos, sin)
        gq, gk = torch.autograd.grad((hq * wq).sum() + (hk * wk).sum(), (q, k))
        assert _rel(rope_bwd_ref(wq, cos, sin)[0], gq) < 1e-12 and _rel(rope_bwd_ref(wk, cos, sin)[0], gk) < 1e-12
        # ... and against autograd of the forward formula of tests/decoder_blocks_ref.py
        gq2, = torch.autograd.grad((rope_ref(q, cos, sin)[0] * wq).sum(), q)
        assert _rel(rope_bwd_ref(wq, cos, sin)[0], gq2) < 1e-12
    # the transpose is not the forward with sin negated once the halves differ
    cos, sin = unequal.cos(), unequal.sin()
    assert _rel(rope_ref(wq, cos, -sin)[0], rope_bwd_ref(wq, cos, sin)[0]) > 1e-2
    cos, sin = equal.cos(), equal.sin()
    assert _rel(rope_ref(wq, cos, -sin)[0], rope_bwd_ref(wq, cos, sin)[0]) < 1e-12


def test_swiglu_backward_reference_equals_autograd_in_float64():
    pytest.importorskip("transformers")
    from transformers.activations import ACT2FN

    g = torch.Generator().manual_seed(33)
    gate = (torch.randn(6, 40, generator=g, dtype=torch.float64) * 4).requires_grad_()
    up = torch.randn(6, 40, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(6, 40, generator=g, dtype=torch.float64)
    for silu in (torch.nn.functional.silu, ACT2FN["silu"]):
        gg, gu = torch.autograd.grad((silu(gate) * up * w).sum(), (gate, up))
        dgate, dup, mag = swiglu_bwd_ref(gate.detach(), up.detach(), w)
        assert _rel(dgate, gg) < 1e-12 and _rel(dup, gu) < 1e-12 and bool((mag >= dgate.abs() * (1 - 1e-12)).all())
    hard = torch.tensor([-800.0, -100.0, -30.0, 30.0, 100.0, 800.0], dtype=torch.float64)
    dgate, dup, _ = swiglu_bwd_ref(hard, torch.full_like(hard, 2.0), torch.full_like(hard, 3.0))
    assert torch.isfinite(dgate).all() and torch.isfinite(dup).all()
    assert dgate[0] == 0 and dup[0] == 0 and dgate[-1] == 6.0 and dup[-1] == 2400.0


# ------------------------------------------------------------------------------------------- bindings, argument checks
NEW = ("bf_add_rmsnorm_bwd_workspace_bytes", "bf_add_rmsnorm_bwd", "bf_rope_qk_bwd", "bf_swiglu_bwd")


def test_symbols_are_bound_with_the_declared_argtypes():
    assert set(NEW) <= set(_C.SYMBOLS)
    lib = _C.lib()
    for name in NEW:
        assert getattr(lib, name).argtypes == _C.SYMBOLS[name][1] and getattr(lib, name).restype == _C.SYMBOLS[name][0]
    assert _C.SYMBOLS["bf_rope_qk_bwd"][1] == _C.SYMBOLS["bf_rope_qk"][1]  # the same bf_rope_t, the same arguments
    assert ops.BLOCK_BWD_CALLS.keys() == {"rmsnorm", "rope", "swiglu"} and ops.BLOCK_CALLS.keys() == {"rmsnorm", "rope", "swiglu"}
    assert lib.bf_version() == _C.ABI_VERSION == 6  # additions only
    for name in ("add_rmsnorm_backward", "rope_qk_backward", "swiglu_backward", "rmsnorm_bwd_supported", "swiglu_bwd_supported",
                 "AddRMSNormFn", "RopeQKFn", "SwiGLUFn"):
        assert hasattr(ops, name), name


def _err():
    return _C.lib().bf_last_error().decode()


def test_add_rmsnorm_bwd_refuses_bad_arguments_without_a_device():
    lib = _C.lib()
    f, wsb = lib.bf_add_rmsnorm_bwd, lib.bf_add_rmsnorm_bwd_workspace_bytes
    ok = dict(z=4096, gamma=16, pd=_C.BF_DT_F32, dy=8192, dz_in=None, dz=12288, dg=16384, ws=32768, wb=1 << 20,
              dt=_C.BF_DT_BF16, rows=4, N=64)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["z"], a["gamma"], a["pd"], a["dy"], a["dz_in"], a["dz"], a["dg"], a["ws"], a["wb"], a["dt"], a["rows"],
                 a["N"], 1e-6, None)

    for name in ("z", "gamma", "dy", "dz"):
        assert call(**{name: None}) == 1 and "null pointer" in _err(), name
    assert call(dg=None) == 1 and "null parameter gradient" in _err()
    assert call(z=4104) == 1 and "16-byte aligned" in _err()
    assert call(dz_in=8) == 1 and "16-byte aligned" in _err()
    assert call(ws=32776) == 1 and "16-byte aligned" in _err()
    assert call(N=60) == 1 and "multiple of 8" in _err()
    assert call(N=8200) == 1 and "at most 8192" in _err()
    assert call(dt=7) == 1 and "unknown dtype" in _err()
    assert call(pd=_C.BF_DT_F16) == 1 and "gamma must be fp32" in _err()
    assert call(rows=-1) == 1 and "bad shape" in _err()
    assert call(ws=None) == 1 and "workspace too small" in _err()
    need = wsb(4, 64)
    assert need == 64 * 4  # a wave per row at N = 64: the 4 rows are one workgroup's, which leaves one [N] fp32 partial row
    assert call(wb=need - 1) == 1 and "workspace too small" in _err()
    # the partials layout: one fp32 row per workgroup, 8 / 4 / 1 rows per workgroup, 1024 (512 beyond N = 2048) at most
    assert wsb(515, 768) == 65 * 768 * 4 and wsb(515, 1032) == 129 * 1032 * 4 and wsb(515, 4096) == 512 * 4096 * 4
    assert wsb(10 ** 6, 1024) == 1024 * 1024 * 4 and wsb(10 ** 6, 8192) == 512 * 8192 * 4
    assert wsb(0, 64) == 0 and wsb(4, 0) == 0


def test_rope_qk_bwd_refuses_bad_arguments_without_a_device():
    f = _C.lib().bf_rope_qk_bwd

    def shape(D=64, cos_batch=1, stride=64):
        s = _C.bf_rope_t(2, 4, 8, 2, D, cos_batch)
        for name in ("q_stride", "k_stride", "q_out_stride", "k_out_stride"):
            getattr(s, name)[:] = [4 * 8 * D, stride, 8 * D]
        return s

    def call(s, q=4096, cos=16, dt=_C.BF_DT_BF16, cd=_C.BF_DT_F32, out=12288):
        return f(q, 8192, cos, 32, cd, out, 16384, dt, ctypes.byref(s) if s is not None else None, None)

    assert call(None) == 1 and "bf_rope_qk_bwd: shape is NULL" in _err()
    assert call(shape(D=96)) == 1 and "head_dim=96 must be 64 or 128" in _err()
    assert call(shape(cos_batch=3)) == 1 and "cos_batch" in _err()
    assert call(shape(), q=None) == 1 and "null pointer" in _err()
    assert call(shape(), out=None) == 1 and "null pointer" in _err()
    assert call(shape(), cos=24) == 1 and "16-byte aligned" in _err()
    assert call(shape(stride=60)) == 1 and "multiples of 8" in _err()
    assert call(shape(stride=-64)) == 1 and "multiples of 8" in _err()
    assert call(shape(), dt=9) == 1 and "unknown dtype" in _err()
    assert call(shape(), cd=_C.BF_DT_F16) == 1 and "bf_rope_qk_bwd: cos / sin must be fp32" in _err()
    # the forward's messages still carry the forward's name
    assert _C.lib().bf_rope_qk(None, 8192, 16, 32, _C.BF_DT_F32, 4096, 8192, _C.BF_DT_BF16, ctypes.byref(shape()), None) == 1
    assert "bf_rope_qk: null pointer" in _err()


def test_swiglu_bwd_refuses_bad_arguments_without_a_device():
    f = _C.lib().bf_swiglu_bwd
    ok = dict(g=4096, gs=64, u=8192, us=64, dy=12288, ds=64, dg=16384, dgs=128, du=16384 + 128, dus=128, dt=_C.BF_DT_BF16,
              rows=4, N=64)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["g"], a["gs"], a["u"], a["us"], a["dy"], a["ds"], a["dg"], a["dgs"], a["du"], a["dus"], a["dt"], a["rows"],
                 a["N"], None)

    for name in ("g", "u", "dy", "dg", "du"):
        assert call(**{name: None}) == 1 and "null pointer" in _err(), name
    assert call(dy=12296) == 1 and "16-byte aligned" in _err()
    assert call(N=60) == 1 and "multiple of 8" in _err()
    for name in ("gs", "us", "ds", "dgs", "dus"):
        assert call(**{name: 32}) == 1 and "row strides" in _err(), name
        assert call(**{name: 68}) == 1 and "row strides" in _err(), name
    assert call(dt=5) == 1 and "unknown dtype" in _err()
    assert call(rows=-1) == 1 and "bad shape" in _err()
    assert call(rows=0) == 0


def test_backward_ops_refuse_cpu_tensors():
    x = torch.randn(4, 64)
    with pytest.raises(_C.BayeFormersAMDError, match="ROCm device"):
        ops.add_rmsnorm_backward(x, torch.ones(64), x, 1e-6)
    with pytest.raises(_C.BayeFormersAMDError, match="ROCm device"):
        ops.swiglu_backward(x, x, x)
    q = torch.randn(1, 2, 3, 64)
    with pytest.raises(_C.BayeFormersAMDError, match="ROCm device"):
        ops.rope_qk_backward(q, q, torch.ones(1, 3, 64), torch.zeros(1, 3, 64))
    assert not ops.rmsnorm_bwd_supported(x, None, torch.nn.LayerNorm(64)) and not ops.swiglu_bwd_supported(x, x)


# ------------------------------------------------------------------------------------------------ the rewrite's flag
def test_backward_flag_is_off_by_default_and_a_second_call_turns_it_on():
    pytest.importorskip("transformers")
    from test_decoder_blocks_cpu import _tiny

    model = _tiny("llama", layers=2)
    assert bf.fuse_decoder_blocks(model) == 2
    mods = [m for layer in model.model.layers for m in (layer, layer.self_attn, layer.mlp, layer.input_layernorm)] + [model.model.norm]
    assert not any(bf._blocks_backward(m) for m in mods)
    assert bf.fuse_decoder_blocks(model, backward=True) == 0  # nothing is rewritten twice ...
    assert all(bf._blocks_backward(m) for m in mods)          # ... but the layers already rewritten now record gradients
    assert bf.fuse_decoder_blocks(model) == 0 and all(bf._blocks_backward(m) for m in mods)
    fresh = _tiny("llama", layers=2)
    assert bf.fuse_decoder_blocks(fresh, backward=True) == 2 and bf._blocks_backward(fresh.model.layers[1].mlp)
    # off the device every fast form still declines: the framework's own step, its own gradients
    ids = torch.randint(0, 97, (2, 12), generator=torch.Generator().manual_seed(5))
    before = (dict(ops.BLOCK_CALLS), dict(ops.BLOCK_BWD_CALLS))
    fresh.train()
    fresh(input_ids=ids, labels=ids).loss.backward()
    assert fresh.model.norm.weight.grad is not None and (ops.BLOCK_CALLS, ops.BLOCK_BWD_CALLS) == before
