"""Host side of fuse_decoder_blocks(backward="all") (no GPU): the float64 restatement of the three backward formulas
(tests/family_blocks_bwd_ref.py) against torch.autograd.grad through transformers' own code, the fp32 emulations of the
kernels' operation order against the bounds of tests/test_gpu_family_blocks_bwd.py on that test's own inputs, the bindings
and argument checks of the new C entries, and the dispatch."""
import ctypes

import pytest
import torch

transformers = pytest.importorskip("transformers")

import bayeformers_amd as bf  # noqa: E402
import test_gpu_family_blocks_bwd as G  # noqa: E402  (the bounds, the inputs and the emulations; nothing here needs a GPU)
from bayeformers_amd import _C, ops  # noqa: E402
from family_blocks_bwd_ref import geglu_bwd_ref, norm_add_rmsnorm_bwd_ref, qknorm_rope_bwd_ref  # noqa: E402
from family_blocks_ref import norm_add_rmsnorm_ref  # noqa: E402
from test_family_blocks_cpu import KINDS, _tiny  # noqa: E402

F64 = torch.float64


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


class _Norm(torch.nn.Module):
    """Gemma2RMSNorm / Gemma3RMSNorm.forward (offset 1: `_norm(x) * (1.0 + weight)`) and Qwen3RMSNorm.forward (offset 0:
    `weight * (x * rsqrt(variance + eps))`) restated line for line without their upcast to float32, which would leave a
    float64 input with float32's precision (test_family_blocks_cpu.py restates the forwards the same way)."""

    def __init__(self, n, eps, offset, gen):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.randn(n, generator=gen, dtype=F64) * 0.5)
        self.eps, self.offset = eps, offset

    def forward(self, x):
        normed = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + self.eps)
        return normed * (1.0 + self.weight) if self.offset else self.weight * normed


# ------------------------------------------------------------------------- the restatement is autograd's, in float64
@pytest.mark.parametrize("family", ["gemma2", "qwen3"])
def test_norm_reference_equals_autograd_through_the_hf_modules(family):
    """Gemma2RMSNorm's forward (offset 1) / Qwen3RMSNorm's (offset 0) in float64: one norm, add + norm, and the sandwich
    norm -> add -> norm composed from the modules, with and without a second consumer of the sum."""
    woff = 1 if family == "gemma2" else 0
    g = torch.Generator().manual_seed(61)
    x, r = (torch.randn(5, 7, 96, generator=g, dtype=F64).requires_grad_() for _ in range(2))
    dy, dz_in = (torch.randn(5, 7, 96, generator=g, dtype=F64) for _ in range(2))
    pre, out = _Norm(96, 1e-6, woff, g), _Norm(96, 1e-5, woff, g)
    wp, wo = pre.weight.detach(), out.weight.detach()
    for use_pre in (True, False):
        for use_res in (True, False):
            for h in (dz_in, None):
                u = pre(x) if use_pre else x
                z = r + u if use_res else u
                y = out(z)
                outs, cots = ([y, z], [dy, h]) if h is not None else ([y], [dy])
                wanted = [x, out.weight] + ([r] if use_res else []) + ([pre.weight] if use_pre else [])
                got = torch.autograd.grad(outs, wanted, cots)
                ref = norm_add_rmsnorm_bwd_ref(x.detach(), z.detach(), wp if use_pre else None, wo, dy, 1e-6, 1e-5, woff, dz_in=h)
                assert _rel(ref["dx"], got[0]) < 1e-12 and _rel(ref["dgamma_out"], got[1]) < 1e-12
                if use_res:
                    assert _rel(ref["dz"], got[2]) < 1e-12
                if use_pre:
                    assert _rel(ref["dgamma_pre"], got[-1]) < 1e-12
                assert bool((ref["mag_dx"] >= ref["dx"].abs() * (1 - 1e-12)).all()) and bool((ref["mag_dz"] >= ref["dz"].abs() * (1 - 1e-12)).all())
    # only the sum was consumed
    z = r + pre(x)
    gx, gr, gw = torch.autograd.grad(z, [x, r, pre.weight], dz_in)
    ref = norm_add_rmsnorm_bwd_ref(x.detach(), z.detach(), wp, wo, None, 1e-6, 1e-5, woff, dz_in=dz_in)
    assert _rel(ref["dx"], gx) < 1e-12 and torch.equal(ref["dz"], gr) and _rel(ref["dgamma_pre"], gw) < 1e-12
    assert not ref["dgamma_out"].any()


def test_four_norm_sandwich_reference_equals_autograd():
    """Gemma2DecoderLayer's chain around a stand-in for the MLP: h1 = h + post(a), y1 = pre_ff(h1), h2 = h1 + post_ff(m(y1)),
    y2 = nxt(h2): two applications of the restatement, the second one's dz feeding the first one's dz_in."""
    g = torch.Generator().manual_seed(62)
    N = 64
    norms = [_Norm(N, 1e-6, 1, g) for _ in range(4)]
    post, pre_ff, post_ff, nxt = norms
    lin = torch.randn(N, N, generator=g, dtype=F64) / 8
    a, h = (torch.randn(6, N, generator=g, dtype=F64).requires_grad_() for _ in range(2))
    dy2, dh2 = (torch.randn(6, N, generator=g, dtype=F64) for _ in range(2))
    h1 = h + post(a)
    y1 = pre_ff(h1)
    m = y1 @ lin
    h2 = h1 + post_ff(m)
    y2 = nxt(h2)
    ga, gh, *gw = torch.autograd.grad([y2, h2], [a, h] + [n.weight for n in norms], [dy2, dh2])
    w = [n.weight.detach() for n in norms]
    second = norm_add_rmsnorm_bwd_ref(m.detach(), h2.detach(), w[2], w[3], dy2, 1e-6, 1e-6, 1, dz_in=dh2)
    dy1 = second["dx"] @ lin.T
    first = norm_add_rmsnorm_bwd_ref(a.detach(), h1.detach(), w[0], w[1], dy1, 1e-6, 1e-6, 1, dz_in=second["dz"])
    assert _rel(first["dx"], ga) < 1e-12 and _rel(first["dz"], gh) < 1e-12
    for got, ref in zip(gw, (first["dgamma_pre"], first["dgamma_out"], second["dgamma_pre"], second["dgamma_out"])):
        assert _rel(ref, got) < 1e-12


@pytest.mark.parametrize("family", ["gemma2", "qwen3", "gemma3"])
@pytest.mark.parametrize("equal", [True, False])
def test_rope_reference_equals_autograd_through_apply_rotary_pos_emb(family, equal):
    import importlib

    rope = importlib.import_module(f"transformers.models.{family}.modeling_{family}").apply_rotary_pos_emb
    g = torch.Generator().manual_seed(63)
    B, H, Hkv, T, D = 2, 4, 2, 9, 64
    q = torch.randn(B, H, T, D, generator=g, dtype=F64).requires_grad_()
    k = torch.randn(B, Hkv, T, D, generator=g, dtype=F64).requires_grad_()
    wq, wk = torch.randn(B, H, T, D, generator=g, dtype=F64), torch.randn(B, Hkv, T, D, generator=g, dtype=F64)
    ang = torch.randn(B, T, D // 2 if equal else D, generator=g, dtype=F64)
    ang = torch.cat((ang, ang), -1) if equal else ang
    cos, sin = ang.cos(), ang.sin()
    if family == "gemma2":  # no q / k norms: the rotation alone
        gq, gk = torch.autograd.grad(list(rope(q, k, cos, sin)), [q, k], [wq, wk])
        for got, w in ((gq, wq), (gk, wk)):
            ref, mag, none, _ = qknorm_rope_bwd_ref(w, cos, sin)
            assert none is None and _rel(ref, got) < 1e-12 and bool((mag >= ref.abs() * (1 - 1e-12)).all())
        return
    woff = 0 if family == "qwen3" else 1
    qn, kn = _Norm(D, 1e-6, woff, g), _Norm(D, 1e-6, woff, g)
    gq, gk, ggq, ggk = torch.autograd.grad(list(rope(qn(q), kn(k), cos, sin)), [q, k, qn.weight, kn.weight], [wq, wk])
    for got, gg, w, x, n in ((gq, ggq, wq, q, qn), (gk, ggk, wk, k, kn)):
        dx, mag, dg, mag_g = qknorm_rope_bwd_ref(w, cos, sin, x.detach(), n.weight.detach(), 1e-6, woff)
        assert _rel(dx, got) < 1e-12 and _rel(dg, gg) < 1e-12
        assert bool((mag >= dx.abs() * (1 - 1e-12)).all()) and bool((mag_g >= dg.abs() * (1 - 1e-12)).all())


def test_geglu_reference_equals_autograd_and_is_finite_at_the_hard_gates():
    import torch.nn.functional as F

    g = torch.Generator().manual_seed(64)
    gate = (torch.randn(6, 40, generator=g, dtype=F64) * 3).requires_grad_()
    up = torch.randn(6, 40, generator=g, dtype=F64).requires_grad_()
    dy = torch.randn(6, 40, generator=g, dtype=F64)
    gg, gu = torch.autograd.grad(F.gelu(gate, approximate="tanh") * up, [gate, up], dy)
    rg, ru, mag = geglu_bwd_ref(gate.detach(), up.detach(), dy)
    # (torch's own formula cancels in 1 + tanh for negative gates: compared over the tensor's largest element)
    assert _rel(rg, gg) < 1e-12 and _rel(ru, gu) < 1e-12 and bool((mag >= rg.abs() * (1 - 1e-12)).all())
    for dtype in (torch.bfloat16, torch.float16, torch.float32):
        gate, up, dy = G.hard_gates(dtype, device="cpu")
        rg, ru, mag = geglu_bwd_ref(gate, up, dy)
        assert torch.isfinite(rg).all() and torch.isfinite(ru).all() and torch.isfinite(mag).all()
        big = float(torch.finfo(dtype).max)
        assert torch.equal(rg[gate.double() == big], (dy.double() * up.double())[gate.double() == big])
        assert not rg[gate.double() == -big].any() and not ru[gate.double() == -big].any()


# ------------------------------------------------------------- the kernels' operation order stays inside the GPU bounds
@pytest.mark.parametrize("name", list(G.DTYPES))
def test_emulated_norm_backward_is_inside_the_gpu_tests_bounds(name):
    dtype = G.DTYPES[name]
    gen = torch.Generator().manual_seed(51)
    worst = 0.0
    for turn, (rows, N) in enumerate(((1, 64), (7, 256), (9, 768), (7, 1032), (9, 2304), (3, 8192))):
        x, res, dy, dz_in, gp, go = G.norm_inputs(gen, rows, N, dtype, device="cpu")
        woff, gdt = G.NORM_PARAMS[turn % 4]
        gp0, go = (g if gdt == "fp32" else g.to(dtype) for g in (gp, go))
        for gp in (gp0, None):
            for r in (res, None):
                z = norm_add_rmsnorm_ref(x, gp, r, go, 1e-6, 1e-5, woff, dtype)[1].to(dtype)  # what the forward stores
                for h in (dz_in, None):
                    for d in (dy, None):
                        if d is None and h is None:
                            continue
                        ref = norm_add_rmsnorm_bwd_ref(x, z, gp, go, d, 1e-6, 1e-5, woff, dz_in=h)
                        emu = G.emulate_norm_bwd(x, z, gp, go, d, h, 1e-6, 1e-5, woff, dtype)
                        ratios = G.norm_ratios(emu, ref, G.norm_bounds(ref, rows, dtype))
                        assert all(v <= 1.0 for v in ratios.values()), (rows, N, woff, gdt, ratios)
                        worst = max(worst, *ratios.values())
    print(f"[emulated norm backward {name}] worst error / bound {worst:.3f}")


@pytest.mark.parametrize("name", list(G.DTYPES))
def test_emulated_rope_and_geglu_backward_are_inside_the_gpu_tests_bounds(name):
    dtype = G.DTYPES[name]
    gen = torch.Generator().manual_seed(53)
    worst = 0.0
    for turn, (D, H, Hkv, T) in enumerate(((64, 8, 2, 5), (128, 8, 8, 5), (256, 16, 1, 5), (256, 8, 2, 1))):
        for equal in (True, False):
            cs_dtype = (dtype, torch.float32)[turn % 2]
            dq, dk, q, k, cos, sin, gq, gk = G.rope_inputs(gen, dtype, 3, T, H, Hkv, D, "view", 3, cs_dtype, equal, device="cpu")
            for gamma, woff in ((None, 0), (gq, 0), (gk.to(dtype), 1)):
                for src, x, heads in ((dq, q, H), (dk, k, Hkv)):
                    dx64, mag, dg64, mag_g = qknorm_rope_bwd_ref(src, cos, sin, x, gamma, 1e-6, woff)
                    bx, bg = G.rope_bounds(dx64, mag, dg64, mag_g, 3 * T * heads, dtype, gamma is not None)
                    ex, eg = G.emulate_qknorm_rope_bwd(src, cos, sin, x, gamma, 1e-6, woff, dtype)
                    ratios = [G._ratio(ex, dx64, bx)] + ([G._ratio(eg, dg64, bg)] if gamma is not None else [])
                    assert max(ratios) <= 1.0, (D, H, Hkv, T, equal, gamma is not None, ratios)
                    worst = max(worst, *ratios)
    gen = torch.Generator().manual_seed(56)
    cases = [(G._randn(gen, 7, 2816, dtype=dtype, device="cpu", scale=3.0), G._randn(gen, 7, 2816, dtype=dtype, device="cpu"),
              G._randn(gen, 7, 2816, dtype=dtype, device="cpu")), G.hard_gates(dtype, device="cpu")]
    for gate, up, dy in cases:
        rg, ru, mag = geglu_bwd_ref(gate, up, dy)
        bg, bu = G.geglu_bounds(rg, ru, mag, dtype)
        eg, eu = G.emulate_geglu_bwd(gate, up, dy, dtype)
        a, b = G._ratio(eg, rg, bg), G._ratio(eu, ru, bu)
        assert a <= 1.0 and b <= 1.0, (a, b)
        worst = max(worst, a, b)
    print(f"[emulated rope / geglu backward {name}] worst error / bound {worst:.3f}")


# --------------------------------------------------------------------------------------------- bindings and checks
def _err():
    return _C.lib().bf_last_error().decode()


def test_the_backward_entries_are_declared_bound_and_exported():
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    declared = open(os.path.join(root, "include", "bayeformers_amd_family_blocks_bwd.h")).read()
    forwards = open(os.path.join(root, "include", "bayeformers_amd_family_blocks.h")).read()
    assert forwards.count('#include "bayeformers_amd_family_blocks_bwd.h"') == 1  # reached through bayeformers_amd.h
    lib = _C.lib()
    assert sorted(_C.FAMILY_BLOCK_BWD_SYMBOLS) == ["bf_geglu_bwd", "bf_norm_add_rmsnorm_bwd", "bf_norm_add_rmsnorm_bwd_workspace_bytes",
                                                   "bf_qknorm_rope_bwd", "bf_qknorm_rope_bwd_workspace_bytes"]
    for name, (res, args) in _C.FAMILY_BLOCK_BWD_SYMBOLS.items():
        assert name + "(" in declared and name not in _C.SYMBOLS and name not in _C.FAMILY_BLOCK_SYMBOLS
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype == res
    assert _C.FAMILY_BLOCK_BWD_SYMBOLS["bf_geglu_bwd"] == _C.SYMBOLS["bf_swiglu_bwd"]
    assert ops.FAMILY_BLOCK_BWD_CALLS.keys() == {"norm_add_norm", "qknorm_rope", "geglu"}


def test_the_backward_header_prototypes_match_the_ctypes_signatures():
    """test_family_blocks_cpu.py's parse of the forwards' header, applied to include/bayeformers_amd_family_blocks_bwd.h and
    _C.FAMILY_BLOCK_BWD_SYMBOLS: the header declares exactly the table's entries, with each argument's class and width."""
    import os
    import re

    from test_host_api import _c_type_class, _ctypes_class

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "bayeformers_amd_family_blocks_bwd.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    header = re.sub(r"^\s*#.*$", "", header, flags=re.M)
    parsed = {}
    for ret, name, params in re.findall(r"([A-Za-z_][A-Za-z0-9_ \t\n\*]*?)\b(bf_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", header):
        assert name not in parsed, name
        parsed[name] = (_c_type_class(ret), [_c_type_class(a.strip()) for a in params.split(",")])
    assert set(parsed) == set(_C.FAMILY_BLOCK_BWD_SYMBOLS)
    assert not set(parsed) & (set(_C.SYMBOLS) | set(_C.FAMILY_BLOCK_SYMBOLS) | set(_C.SOFTCAP_SYMBOLS))
    for name, (res, args) in _C.FAMILY_BLOCK_BWD_SYMBOLS.items():
        c_res, c_args = parsed[name]
        assert _ctypes_class(res) == c_res, (name, "return")
        assert len(args) == len(c_args), (name, len(args), len(c_args))
        for i, (a, c) in enumerate(zip(args, c_args)):
            assert _ctypes_class(a) == c, (name, i, a, c)


def test_a_library_without_the_backward_entries_asks_for_a_rebuild(monkeypatch):
    monkeypatch.setattr(_C, "_lib", None)
    monkeypatch.setitem(_C.FAMILY_BLOCK_BWD_SYMBOLS, "bf_not_in_this_library_bwd", (ctypes.c_int, []))
    with pytest.raises(_C.BayeFormersAMDError, match="lacks bf_not_in_this_library_bwd.*rebuild"):
        _C.lib()
    assert _C._lib is None


def test_the_backward_entries_refuse_bad_arguments_without_a_device():
    lib = _C.lib()
    ok = dict(x=4096, z=8192, gp=32, go=64, pd=_C.BF_DT_F32, off=1, dy=12288, h=16384, dz=20480, dx=24576, dgp=128, dgo=256,
              ws=32768, wsb=1 << 20, dt=_C.BF_DT_BF16, rows=4, N=64)

    def norm(**kw):
        a = dict(ok, **kw)
        return lib.bf_norm_add_rmsnorm_bwd(a["x"], a["z"], a["gp"], a["go"], a["pd"], a["off"], a["dy"], a["h"], a["dz"], a["dx"],
                                           a["dgp"], a["dgo"], a["ws"], a["wsb"], a["dt"], a["rows"], a["N"], 1e-6, 1e-6, None)

    assert norm(z=None) == 1 and "null pointer" in _err()
    assert norm(dy=None, h=None) == 1 and "null pointer" in _err()
    assert norm(dgo=None) == 1 and "null parameter gradient" in _err()
    assert norm(dgp=None) == 1 and "null parameter gradient" in _err()
    assert norm(x=None) == 1 and "with gamma_pre x and dx are needed" in _err()
    assert norm(gp=None, dz=None) == 1 and "without it dz" in _err()
    assert norm(dy=12296) == 1 and "16-byte aligned" in _err()
    assert norm(N=60) == 1 and "multiple of 8" in _err()
    assert norm(N=8200) == 1 and "at most 8192" in _err()
    assert norm(off=2) == 1 and "weight_offset=2" in _err()
    assert norm(dt=7) == 1 and "unknown dtype" in _err()
    assert norm(pd=_C.BF_DT_F16) == 1 and "gammas must be fp32" in _err()
    assert norm(wsb=16) == 1 and "workspace too small" in _err()
    assert norm(rows=-1) == 1 and "bad shape" in _err()
    assert lib.bf_norm_add_rmsnorm_bwd_workspace_bytes(0, 64, 1) == 0
    assert lib.bf_norm_add_rmsnorm_bwd_workspace_bytes(4, 64, 1) == 2 * lib.bf_norm_add_rmsnorm_bwd_workspace_bytes(4, 64, 0) > 0
    # every layout: 32, 64 and 256 lanes per row (4, 4 and 1 rows per workgroup)
    assert [lib.bf_norm_add_rmsnorm_bwd_workspace_bytes(8, n, 0) // (4 * n) for n in (256, 2048, 2304)] == [1, 2, 8]

    def shape(D=64, cos_batch=1, stride=64, B=2):
        s = _C.bf_rope_t(B, 4, 8, 2, D, cos_batch)
        for name in ("q_stride", "k_stride", "q_out_stride", "k_out_stride"):
            getattr(s, name)[:] = [4 * 8 * D, stride, 8 * D]
        return s

    def rope(s, dqo=4096, q=8192, cos=16, gq=48, gk=64, dgq=128, pd=_C.BF_DT_F32, cd=_C.BF_DT_F32, off=0, wsb=1 << 20, dt=_C.BF_DT_BF16):
        return lib.bf_qknorm_rope_bwd(dqo, 12288, q, 16384, cos, 32, cd, gq, gk, pd, off, 1e-6, 20480, 24576, dgq, 256, 32768, wsb, dt,
                                      ctypes.byref(s) if s is not None else None, None)

    assert rope(None) == 1 and "shape is NULL" in _err()
    assert rope(shape(D=96)) == 1 and "head_dim=96 must be 64, 128 or 256" in _err()
    assert rope(shape(cos_batch=3)) == 1 and "cos_batch" in _err()
    assert rope(shape(), dqo=None) == 1 and "null pointer" in _err()
    assert rope(shape(), q=None) == 1 and "a gamma needs the forward's input" in _err()
    assert rope(shape(), dgq=None) == 1 and "a gamma needs the forward's input" in _err()
    assert rope(shape(), cos=24) == 1 and "16-byte aligned" in _err()
    assert rope(shape(stride=60)) == 1 and "multiples of 8" in _err()
    assert rope(shape(), off=2) == 1 and "weight_offset=2" in _err()
    assert rope(shape(), dt=9) == 1 and "unknown dtype" in _err()
    assert rope(shape(), cd=_C.BF_DT_F16) == 1 and "cos / sin must be fp32" in _err()
    assert rope(shape(), pd=_C.BF_DT_F16) == 1 and "gammas must be fp32" in _err()
    assert rope(shape(), wsb=16) == 1 and "workspace too small" in _err()
    s = shape(D=256)
    assert lib.bf_qknorm_rope_bwd_workspace_bytes(ctypes.byref(s), 0) == 0
    assert lib.bf_qknorm_rope_bwd_workspace_bytes(ctypes.byref(s), 1) == 5 * 2 * 256 * 4  # 2 * 4 * 10 * 16 lanes: 5 workgroups

    f = lib.bf_geglu_bwd
    assert f(None, 64, 4096, 64, 8192, 64, 12288, 64, 16384, 64, _C.BF_DT_BF16, 4, 64, None) == 1 and "null pointer" in _err()
    assert f(4104, 64, 4096, 64, 8192, 64, 12288, 64, 16384, 64, _C.BF_DT_BF16, 4, 64, None) == 1 and "16-byte aligned" in _err()
    assert f(4096, 64, 8192, 64, 12288, 64, 16384, 64, 20480, 64, _C.BF_DT_BF16, 4, 60, None) == 1 and "multiple of 8" in _err()
    assert f(4096, 64, 8192, 64, 12288, 64, 16384, 32, 20480, 64, _C.BF_DT_BF16, 4, 64, None) == 1 and "row strides" in _err()
    assert f(4096, 64, 8192, 64, 12288, 64, 16384, 64, 20480, 64, 5, 4, 64, None) == 1 and "unknown dtype" in _err()
    assert f(4096, 64, 8192, 64, 12288, 64, 16384, 64, 20480, 64, _C.BF_DT_F32, 0, 64, None) == 0


def test_backward_ops_refuse_cpu_tensors():
    x, w = torch.randn(4, 64), torch.ones(64)
    with pytest.raises(_C.BayeFormersAMDError, match="ROCm device"):
        ops.norm_add_rmsnorm_backward(x, x, w, w, x, 1e-6, 1e-6)
    with pytest.raises(_C.BayeFormersAMDError, match="ROCm device"):
        ops.geglu_backward(x, x, x)
    q = torch.randn(1, 2, 3, 64)
    with pytest.raises(_C.BayeFormersAMDError, match="ROCm device"):
        ops.qknorm_rope_backward(q, q, torch.ones(1, 3, 64), torch.zeros(1, 3, 64))


# -------------------------------------------------------------------------------------------------------------- dispatch
@pytest.mark.parametrize("kind", list(KINDS))
def test_backward_all_sets_the_flags_and_cpu_results_are_the_unrewritten_models(kind):
    model, plain = _tiny(kind), _tiny(kind)
    ids = torch.randint(0, 97, (2, 12), generator=torch.Generator().manual_seed(5))
    with pytest.raises(ValueError, match="backward="):
        bf.fuse_decoder_blocks(model, backward="yes", families="all")
    with pytest.raises(ValueError, match="backward="):
        bf.fuse_decoder_blocks(model, backward=1, families="all")
    assert "forward" not in model.model.layers[0].__dict__
    assert bf.fuse_decoder_blocks(model, backward=True, families=kind) == 3
    assert not any(hasattr(m, "_bf_blocks_backward") for m in model.modules())  # True keeps its meaning
    assert bf.fuse_decoder_blocks(model, backward="all", families=kind) == 0   # turns the flag on, counts nothing
    flagged = {n for n, m in model.named_modules() if getattr(m, "_bf_blocks_backward", False)}
    want = {"model.norm"}
    for i in range(3):
        want |= {f"model.layers.{i}", f"model.layers.{i}.self_attn", f"model.layers.{i}.mlp", f"model.layers.{i}.input_layernorm"}
    assert flagged == want, flagged ^ want
    fresh = _tiny(kind)
    assert bf.fuse_decoder_blocks(fresh, backward="all", families="all") == 3
    assert {n for n, m in fresh.named_modules() if getattr(m, "_bf_blocks_backward", False)} == want
    other = {"qwen3": "gemma2"}.get(kind, "qwen3")
    assert bf.fuse_decoder_blocks(_tiny(kind), backward="all", families=other) == 0
    before = (dict(ops.FAMILY_BLOCK_CALLS), dict(ops.BLOCK_CALLS), dict(ops.FAMILY_BLOCK_BWD_CALLS), dict(ops.BLOCK_BWD_CALLS))
    results = []
    for m in (plain, model):
        m.train()
        out = m(input_ids=ids, labels=ids)
        out.loss.backward()
        results.append((out.loss.detach(), out.logits.detach(), {n: p.grad for n, p in m.named_parameters()}))
    (l0, y0, g0), (l1, y1, g1) = results
    # fp32 on the CPU: every fast form declines and the modules' own forwards run — the same bits, gradients included
    assert torch.equal(l0, l1) and torch.equal(y0, y1) and g0.keys() == g1.keys()
    assert all(g1[n] is not None and torch.equal(g0[n], g1[n]) for n in g0)
    assert before == (ops.FAMILY_BLOCK_CALLS, ops.BLOCK_CALLS, ops.FAMILY_BLOCK_BWD_CALLS, ops.BLOCK_BWD_CALLS)


def test_backward_all_flags_the_default_families_too():
    import transformers as tf

    cfg = tf.LlamaConfig(hidden_size=128, num_attention_heads=2, num_key_value_heads=1, num_hidden_layers=2, intermediate_size=256,
                         vocab_size=97, max_position_embeddings=64, tie_word_embeddings=False, head_dim=64)
    torch.manual_seed(3)
    model = tf.LlamaForCausalLM(cfg).eval()
    assert bf.fuse_decoder_blocks(model, backward="all") == 2
    assert all(getattr(layer, "_bf_blocks_backward", False) for layer in model.model.layers)
