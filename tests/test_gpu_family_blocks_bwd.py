"""bf_norm_add_rmsnorm_bwd / bf_qknorm_rope_bwd / bf_geglu_bwd against the float64 restatement of
tests/family_blocks_bwd_ref.py, and fuse_decoder_blocks(backward="all") on training steps of two-layer Gemma 2, Gemma 3 and
Qwen3 decoders: eager, graphed, in training mode, checkpointed, and the cases in which it must step aside.

Tolerances are derived, not measured, in test_gpu_decoder_blocks_bwd.py's manner: u = 2^-24 is one fp32 rounding, ULP half
the spacing of the output format (relative), and every bound is  ULP |ref| + c u mag + TINY  with mag the magnitude the terms
of the result had before they could cancel (the reference returns it) and c counted from the kernel:

  norm   stage 2 is add_rmsnorm_bwd_kernel's arithmetic with w = woff + gamma formed in fp32 (one more rounding on each of
         the two terms): with D <= 41 the depth of an fp32 row sum (8 V fused multiply-adds per lane, V <= 4, 6 tree steps
         over a wave, 3 adds across the waves), dz carries at most (D + 15) u mag_dz <= 64 u mag_dz before it is rounded:
             dz:  ULP |ref| + 64 u mag_dz.
         Stage 1 takes that dz unrounded: its error, at most 64 u mag_dz element for element, goes through stage 1's linear
         map, whose absolute form applied to mag_dz is mag_dx by definition, and stage 1's own arithmetic adds 64 u of the
         map applied to |dz| <= mag_dz:
             dx:  ULP |ref| + 128 u mag_dx.
         dgamma (fp32): a term is formed in fp64 and added to the fp32 partial sum with one rounding; the `rows` terms of a
         column are merged by rows - 1 additions whatever the order, u sum |terms| each at most:
             dgamma_out:  u |ref| + rows u sum |dy z r|;
         dgamma_pre's terms carry dz's error as well, 64 u mag_dz |x| r each:
             dgamma_pre:  u |ref| + (rows + 64) u sum mag_dz |x| r      (mag_dz >= |dz|).
  rope   without gammas rope_qk_kernel's transpose: c = 2.  With a gamma the rotated dn (2 u of the rotation's magnitude) is
         the cotangent of a norm over D whose fp32 sums are 16 fused multiply-adds and at most 4 shuffle steps deep
         (D + 15 <= 64 again): dx: ULP |ref| + 66 u mag with mag the norm's absolute map applied to the rotation's
         magnitudes; dgamma: u |ref| + (terms + 2) u sum mag_rot |x| r, terms = B T heads.
  GeGLU  2k is formed in fp64 and rounded once (|2k| u absolute, |2k| <= 88 wherever e = exp(-|2k|) is a normal number), expf
         2 u: e carries 90 u; 1 + e, the reciprocal, e * that: 3 u.  Whichever of s and 1 - s is e / (1 + e) carries 93 u, the
         other one at most 47 u (e / (1 + e) <= 1 / 2 of e's error, and 2 u); the bracket s (1 + g q (1 - s)) is formed in
         fp64 and rounded once, then two products: 93 + 47 + 3 = 143 <= 144:
             dgate:  ULP |ref| + 144 u mag,     dup = dy (g s):  (ULP + 96 u) |ref|.
         Where e is subnormal the results it dominates are below 300 e |dy u| < TINY.

Before these constants were trusted, an fp32 torch emulation of each kernel's operation order was run on the CPU on the
tests' own inputs (the emulate_* functions; tests/test_family_blocks_bwd_cpu.py runs them without a GPU, and every kernel
test here on its first cases): it stays inside the bounds."""
import functools

import numpy as np
import pytest
import torch

from family_blocks_bwd_ref import K2C, K2CA, geglu_bwd_ref, norm_add_rmsnorm_bwd_ref, qknorm_rope_bwd_ref

pytestmark = pytest.mark.gpu

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
ULP = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -24}
TINY = {torch.bfloat16: 2.0 ** -126, torch.float16: 2.0 ** -25, torch.float32: 2.0 ** -126}
U = 2.0 ** -24
SEED = 0x5EED
NORM_ROWS, NORM_N = (1, 7, 9, 515), (64, 256, 768, 1032, 2304, 4096, 8192)
NORM_PARAMS = ((1, "fp32"), (0, "act"), (1, "act"), (0, "fp32"))  # (weight offset, the gammas' dtype), in turn


def _randn(gen, *shape, dtype, device="cuda", scale=1.0):
    return (torch.randn(*shape, generator=gen) * scale).to(device, dtype)


def _ratio(got, ref, bound):
    assert torch.isfinite(got).all()
    return float(((got.double() - ref).abs() / bound).max())


# ------------------------------------------------------------------------------------------------ bf_norm_add_rmsnorm_bwd
def norm_inputs(gen, rows, N, dtype, device="cuda"):
    """x, residual, dy, dz_in [rows, N] of dtype and two fp32 gammas around 0.5 (so that both offsets give weights that show)"""
    x, res = _randn(gen, rows, N, dtype=dtype, device=device), _randn(gen, rows, N, dtype=dtype, device=device, scale=3.0)
    dy, dz_in = _randn(gen, rows, N, dtype=dtype, device=device), _randn(gen, rows, N, dtype=dtype, device=device, scale=0.5)
    gp, go = ((0.5 + 0.5 * torch.randn(N, generator=gen)).to(device) for _ in range(2))
    return x, res, dy, dz_in, gp, go


def norm_bounds(ref, rows, dtype):
    b = {"dz": ULP[dtype] * ref["dz"].abs() + 64 * U * ref["mag_dz"] + TINY[dtype],
         "dx": ULP[dtype] * ref["dx"].abs() + 128 * U * ref["mag_dx"] + TINY[dtype],
         "dgamma_out": U * ref["dgamma_out"].abs() + rows * U * ref["mag_dgamma_out"] + 2.0 ** -126}
    if "dgamma_pre" in ref:
        b["dgamma_pre"] = U * ref["dgamma_pre"].abs() + (rows + 64) * U * ref["mag_dgamma_pre"] + 2.0 ** -126
    return b


def _emulate_stage(v, w, cot, eps):
    """One norm's backward in the kernel's order, fp32 on the CPU (the row sums in torch's own fp32 order; r from an fp64 sum
    of squares, each dgamma term in fp64 before it joins the fp32 sum) -> (dv unrounded, dgamma)"""
    N = v.shape[-1]
    rd = 1.0 / torch.sqrt((v.double() * v.double()).sum(-1, keepdim=True) / N + float(np.float32(eps)))
    r = rd.float()
    s = ((cot * w) * v).sum(-1, keepdim=True)
    k = r * r * r * (s * np.float32(1.0 / N))
    dv = torch.addcmul(r * (cot * w), -v, k)
    dgamma = torch.zeros(N)
    for row in range(v.shape[0]):
        dgamma = (dgamma.double() + cot[row].double() * v[row].double() * rd[row]).float()
    return dv, dgamma


def emulate_norm_bwd(x, z, gp, go, dy, dz_in, eps_pre, eps_out, woff, dtype):
    """-> {dz, dx rounded to dtype, dgamma_out, dgamma_pre fp32} as norm_add_rmsnorm_bwd_kernel forms them"""
    z = z.float().cpu()
    out = {}
    if dy is not None:
        dz, out["dgamma_out"] = _emulate_stage(z, np.float32(woff) + go.float().cpu(), dy.float().cpu(), eps_out)
    else:
        dz, out["dgamma_out"] = torch.zeros_like(z), torch.zeros(z.shape[-1])
    if dz_in is not None:
        dz = dz + dz_in.float().cpu()
    out["dz"] = dz.to(dtype)
    if gp is None:
        out["dx"] = out["dz"]
        return out
    dx, out["dgamma_pre"] = _emulate_stage(x.float().cpu(), np.float32(woff) + gp.float().cpu(), dz, eps_pre)
    out["dx"] = dx.to(dtype)
    return out


def norm_ratios(got, ref, bounds):
    return {k: _ratio(got[k], ref[k].to(got[k].device), bounds[k].to(got[k].device)) for k in bounds if k in got}


@pytest.mark.parametrize("name", list(DTYPES))
def test_norm_add_rmsnorm_bwd_matches_float64(name):
    """rows 1 / 7 / 9 / 515 x N 64 (a wave per row) / 256, 768 (half a wave per row) / 1032 (a vector count that is no
    multiple of 64) / 2304, 4096, 8192 (a workgroup per row, V = 2, 2, 4): an idle half wave, idle waves and a partial last
    workgroup among them; with and without gamma_pre, the residual and dz_in; offsets 0 / 1 and gammas in fp32 / the
    activation dtype in turn; z is what the forward kernel stored."""
    from bayeformers_amd import ops

    dtype = DTYPES[name]
    gen = torch.Generator().manual_seed(51)
    eps_pre, eps_out = 1e-6, 1e-5
    worst, emu, turn = {}, 0.0, 0
    for rows in NORM_ROWS:
        for N in NORM_N:
            x, res, dy, dz_in, gp32, go32 = norm_inputs(gen, rows, N, dtype)
            woff, gdt = NORM_PARAMS[turn % 4]
            turn += 1
            gp0, go = (g if gdt == "fp32" else g.to(dtype) for g in (gp32, go32))
            for gp in (gp0, None):
                for r in (res, None):
                    z = ops.norm_add_rmsnorm(x, gp, r, go, eps_pre, eps_out, woff)[0]  # what the forward saved
                    assert (z is x) == (gp is None and r is None)
                    for h in (dz_in, None):
                        before = ops.FAMILY_BLOCK_BWD_CALLS["norm_add_norm"]
                        dx, dz, dgp, dgo = ops.norm_add_rmsnorm_backward(x if gp is not None else None, z, gp, go, dy, eps_pre,
                                                                         eps_out, woff, grad_sum=h)
                        assert ops.FAMILY_BLOCK_BWD_CALLS["norm_add_norm"] - before == 1
                        assert dz.dtype == dtype and dz.shape == z.shape and dgo.dtype == torch.float32 and dgo.shape == (N,)
                        assert (dx is dz and dgp is None) if gp is None else (dx.dtype == dtype and dgp.dtype == torch.float32)
                        ref = norm_add_rmsnorm_bwd_ref(x, z, gp, go, dy, eps_pre, eps_out, woff, dz_in=h)
                        bounds = norm_bounds(ref, rows, dtype)
                        got = {"dz": dz, "dx": dx, "dgamma_out": dgo}
                        if gp is not None:
                            got["dgamma_pre"] = dgp
                        ratios = norm_ratios(got, ref, bounds)
                        assert all(v <= 1.0 for v in ratios.values()), (rows, N, woff, gdt, gp is not None, r is not None,
                                                                        h is not None, ratios)
                        for k, v in ratios.items():
                            worst[k] = max(worst.get(k, 0.0), v)
                        if gp is not None and r is not None and h is not None and rows in (7, 9):
                            e = emulate_norm_bwd(x, z, gp, go, dy, h, eps_pre, eps_out, woff, dtype)
                            emu = max(emu, *norm_ratios(e, {k: v.cpu() for k, v in ref.items()}, bounds).values())
    print(f"[norm_add_rmsnorm_bwd {name}] worst error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items())
          + f"; fp32 emulation {emu:.3f}")
    assert emu <= 1.0


def test_norm_add_rmsnorm_bwd_without_dy_in_place_and_repeatable():
    """dy = NULL (only the sum was consumed): dz = dz_in, dgamma_out = 0, stage 1 from dz_in.  dz over dy, dz over dz_in and
    dx over dz (in place) give the out-of-place bits, and two launches give the same dgammas bit for bit (no atomics)."""
    from bayeformers_amd import _C, ops

    gen = torch.Generator().manual_seed(52)
    rows, N, dtype = 515, 768, torch.bfloat16
    x, res, dy, h, gp, go = norm_inputs(gen, rows, N, dtype)
    z = ops.norm_add_rmsnorm(x, gp, res, go, 1e-6, 1e-6, 1)[0]
    dx0, dz0, dgp0, dgo0 = ops.norm_add_rmsnorm_backward(x, z, gp, go, None, 1e-6, 1e-6, 1, grad_sum=h)
    ref = norm_add_rmsnorm_bwd_ref(x, z, gp, go, None, 1e-6, 1e-6, 1, dz_in=h)
    assert torch.equal(dz0, h) and not dgo0.any()
    ratios = norm_ratios({"dx": dx0, "dgamma_pre": dgp0}, ref, norm_bounds(ref, rows, dtype))
    assert all(v <= 1.0 for v in ratios.values()), ratios
    with pytest.raises(_C.BayeFormersAMDError, match="no gradient"):
        ops.norm_add_rmsnorm_backward(x, z, gp, go, None, 1e-6, 1e-6, 1)

    dx, dz, dgp, dgo = ops.norm_add_rmsnorm_backward(x, z, gp, go, dy, 1e-6, 1e-6, 1, grad_sum=h)
    shaped = [t.view(5, 103, N) for t in (x, z, dy, h)]
    dx2, dz2, dgp2, dgo2 = ops.norm_add_rmsnorm_backward(shaped[0], shaped[1], gp, go, shaped[2], 1e-6, 1e-6, 1, grad_sum=shaped[3])
    assert dx2.shape == (5, 103, N) and torch.equal(dx2.view(rows, N), dx) and torch.equal(dz2.view(rows, N), dz)
    assert torch.equal(dgp2, dgp) and torch.equal(dgo2, dgo)
    lib = _C.lib()
    stream = torch.cuda.current_stream().cuda_stream

    def raw(gpre, d_dy, d_h, d_dz, d_dx):
        ws = torch.empty(lib.bf_norm_add_rmsnorm_bwd_workspace_bytes(rows, N, int(gpre is not None)), dtype=torch.uint8, device="cuda")
        a, b = torch.empty_like(dgo), torch.empty_like(dgo)
        _C.check(lib.bf_norm_add_rmsnorm_bwd(x.data_ptr(), z.data_ptr(), gpre.data_ptr() if gpre is not None else None,
                                             go.data_ptr(), _C.BF_DT_F32, 1, d_dy.data_ptr(), d_h.data_ptr(), d_dz.data_ptr(),
                                             d_dx.data_ptr() if d_dx is not None else None, a.data_ptr(), b.data_ptr(),
                                             ws.data_ptr(), ws.numel(), _C.BF_DT_BF16, rows, N, 1e-6, 1e-6, stream),
                 "bf_norm_add_rmsnorm_bwd")
        return a, b

    buf, out = dy.clone(), torch.empty_like(dx)  # dz over dy
    a, b = raw(gp, buf, h, buf, out)
    assert torch.equal(buf, dz) and torch.equal(out, dx) and torch.equal(a, dgp) and torch.equal(b, dgo)
    buf, out = h.clone(), torch.empty_like(dx)  # dz over dz_in
    a, b = raw(gp, dy, buf, buf, out)
    assert torch.equal(buf, dz) and torch.equal(out, dx) and torch.equal(a, dgp) and torch.equal(b, dgo)
    buf = torch.empty_like(dx)  # dx over dz: the later store stays
    a, b = raw(gp, dy, h, buf, buf)
    assert torch.equal(buf, dx) and torch.equal(a, dgp) and torch.equal(b, dgo)
    dz1 = ops.norm_add_rmsnorm_backward(None, z, None, go, dy, 1e-6, 1e-6, 1, grad_sum=h)
    buf = dy.clone()  # without gamma_pre, dz over dy
    _, b = raw(None, buf, h, buf, None)
    assert torch.equal(buf, dz1[1]) and torch.equal(b, dz1[3])


# ----------------------------------------------------------------------------------------------------- bf_qknorm_rope_bwd
def rope_inputs(gen, dtype, B, T, H, Hkv, D, layout, cos_batch, cs_dtype, equal, device="cuda"):
    """(dq_out, dk_out, q, k, cos, sin, gamma_q, gamma_k): the gradients in the given layout, the forward's inputs laid out
    [B, T, heads, D], tables with equal or unequal halves, fp32 gammas around 0.5"""
    def t4(heads, lay):
        if lay == "view":  # laid out [B, T, heads * D] and seen as [B, heads, T, D]
            return _randn(gen, B, T, heads * D, dtype=dtype, device=device).view(B, T, heads, D).transpose(1, 2)
        return _randn(gen, B, heads, T, D, dtype=dtype, device=device)

    dq, dk = t4(H, layout), t4(Hkv, layout)
    q, k = t4(H, "view"), t4(Hkv, "view")
    if equal:  # what the rotary module returns: the two halves carry the same angles
        ang = torch.rand(cos_batch, T, D // 2, generator=gen, dtype=torch.float64) * 200.0
        ang = torch.cat((ang, ang), -1)
    else:
        ang = torch.rand(cos_batch, T, D, generator=gen, dtype=torch.float64) * 200.0
    gq, gk = ((0.5 + 0.5 * torch.randn(D, generator=gen)).to(device) for _ in range(2))
    return dq, dk, q, k, ang.cos().to(device, cs_dtype), ang.sin().to(device, cs_dtype), gq, gk


def rope_bounds(dx64, mag, dg64, mag_g, terms, dtype, has_gamma):
    bx = ULP[dtype] * dx64.abs() + (66 if has_gamma else 2) * U * mag + TINY[dtype]
    bg = U * dg64.abs() + (terms + 2) * U * mag_g + 2.0 ** -126 if has_gamma else None
    return bx, bg


def emulate_qknorm_rope_bwd(dout, cos, sin, x, gamma, eps, woff, dtype):
    d, c, s = dout.float().cpu(), cos.float().cpu()[:, None], sin.float().cpu()[:, None]
    h = d.shape[-1] // 2
    d1, d2 = d[..., :h], d[..., h:]
    dn = torch.cat((torch.addcmul(d2 * s[..., h:], d1, c[..., :h]), torch.addcmul(-(d1 * s[..., :h]), d2, c[..., h:])), -1)
    if gamma is None:
        return dn.to(dtype), None
    D = d.shape[-1]
    dx, dg = _emulate_stage(x.float().cpu().reshape(-1, D), np.float32(woff) + gamma.float().cpu(), dn.reshape(-1, D), eps)
    return dx.view(d.shape).to(dtype), dg


def _rope_case(gen, dtype, B, T, H, Hkv, D, layout, cos_batch, cs_dtype, equal, mode, gdt, woff, emulate=False):
    """One launch against the reference -> (worst ratio, worst ratio of the emulation)"""
    from bayeformers_amd import ops

    dq, dk, q, k, cos, sin, gq, gk = rope_inputs(gen, dtype, B, T, H, Hkv, D, layout, cos_batch, cs_dtype, equal)
    gq, gk = (g if gdt == "fp32" else g.to(dtype) for g in (gq, gk))
    gq, gk = (gq if mode in ("q", "both") else None), (gk if mode == "both" else None)
    eps = 1e-6
    what = (B, T, H, Hkv, D, layout, cos_batch, cs_dtype, equal, mode, gdt, woff)
    dq0, dk0, q0, k0 = dq.clone(), dk.clone(), q.clone(), k.clone()
    before = ops.FAMILY_BLOCK_BWD_CALLS["qknorm_rope"]
    oq, ok, dgq, dgk = ops.qknorm_rope_backward(dq, dk, cos, sin, q, k, gq, gk, eps, woff)
    assert ops.FAMILY_BLOCK_BWD_CALLS["qknorm_rope"] - before == 1
    assert all(torch.equal(a, b) for a, b in ((dq, dq0), (dk, dk0), (q, q0), (k, k0))) and oq.shape == dq.shape and ok.shape == dk.shape
    # laid out [B, T, heads, D]: what the backward of the projections reads
    assert oq.transpose(1, 2).is_contiguous() and ok.transpose(1, 2).is_contiguous()
    assert (dgq is None) == (gq is None) and (dgk is None) == (gk is None)
    worst = emu = 0.0
    for got, dg, src, x, g, heads in ((oq, dgq, dq0, q0, gq, H), (ok, dgk, dk0, k0, gk, Hkv)):
        dx64, mag, dg64, mag_g = qknorm_rope_bwd_ref(src, cos, sin, x, g, eps, woff)
        bx, bg = rope_bounds(dx64, mag, dg64, mag_g, B * T * heads, dtype, g is not None)
        ratios = [_ratio(got, dx64, bx)] + ([_ratio(dg, dg64, bg)] if g is not None else [])
        assert max(ratios) <= 1.0, (what, ratios)
        worst = max(worst, *ratios)
        if emulate:
            ex, eg = emulate_qknorm_rope_bwd(src, cos, sin, x, g, eps, woff, dtype)
            emu = max(emu, _ratio(ex, dx64.cpu(), bx.cpu()), _ratio(eg, dg64.cpu(), bg.cpu()) if g is not None else 0.0)
    return worst, emu


@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("D", [64, 128, 256])
def test_qknorm_rope_bwd_matches_float64(name, D):
    """(H, Hkv) x T x both layouts x cos_batch x table dtype x equal / unequal halves, the gammas (none / q only / both), their
    dtype and the weight offset taking turns so that every (H, Hkv, T) meets every mode."""
    dtype = DTYPES[name]
    gen = torch.Generator().manual_seed(53 + D)
    B, worst, emu, turn = 3, 0.0, 0.0, 0
    for H, Hkv in ((8, 8), (8, 2), (16, 1)):
        for T in (1, 5, 128):
            for layout in ("view", "bhtd"):
                for cos_batch in (1, B):
                    for cs_dtype in (dtype, torch.float32):
                        for equal in (True, False):
                            mode, gdt, woff = ("none", "q", "both")[turn % 3], ("fp32", "act")[(turn // 3) % 2], (turn // 2) % 2
                            turn += 1
                            w, e = _rope_case(gen, dtype, B, T, H, Hkv, D, layout, cos_batch, cs_dtype, equal, mode, gdt, woff,
                                              emulate=T == 5)
                            worst, emu = max(worst, w), max(emu, e)
    print(f"[qknorm_rope_bwd {name} D={D}] worst error / bound {worst:.3f}, fp32 emulation {emu:.3f}")
    assert emu <= 1.0


def test_qknorm_rope_bwd_grid_stride_loop_and_repeatable():
    """3 * 128 * 48 heads * 16 lanes = 294912 lanes of work, beyond the 1024 workgroups of 256: the stride loop runs, and the
    dgamma partials of a lane cover several rounds.  Two launches give the same bits."""
    from bayeformers_amd import ops

    gen = torch.Generator().manual_seed(54)
    args = (torch.bfloat16, 3, 128, 40, 8, 256, "view", 1, torch.float32, True, "both", "fp32", 1)
    _rope_case(gen, *args)
    dq, dk, q, k, cos, sin, gq, gk = rope_inputs(gen, torch.bfloat16, 3, 128, 40, 8, 256, "view", 1, torch.float32, True)
    a = ops.qknorm_rope_backward(dq, dk, cos, sin, q, k, gq, gk, 1e-6, 1)
    b = ops.qknorm_rope_backward(dq, dk, cos, sin, q, k, gq, gk, 1e-6, 1)
    assert all(torch.equal(s, t) for s, t in zip(a, b))
    # the forward's inputs in another layout are copied into the one the kernel reads: the same bits
    c = ops.qknorm_rope_backward(dq, dk, cos, sin, q.contiguous(), k.contiguous(), gq, gk, 1e-6, 1)
    assert all(torch.equal(s, t) for s, t in zip(a, c))


@pytest.mark.parametrize("equal", [True, False])
def test_qknorm_rope_backward_is_the_adjoint_of_the_forward_kernel(equal):
    """<F(x), w> = <x, F'(w)> in fp32 without gammas, the products summed in float64, to 2^-20 of sum |terms|: kernel against
    kernel, at the three head sizes."""
    from bayeformers_amd import ops

    gen = torch.Generator().manual_seed(55)
    for D in (64, 128, 256):
        wq, wk, q, k, cos, sin, _, _ = rope_inputs(gen, torch.float32, 3, 37, 8, 2, D, "view", 3, torch.float32, equal)
        yq, yk = ops.qknorm_rope(q, k, cos, sin)
        dq, dk, _, _ = ops.qknorm_rope_backward(wq, wk, cos, sin)
        for y, w, x, d in ((yq, wq, q, dq), (yk, wk, k, dk)):
            lhs, rhs = (y.double() * w.double()), (x.double() * d.double())
            scale = float(lhs.abs().sum() + rhs.abs().sum())
            diff = abs(float(lhs.sum() - rhs.sum()))
            print(f"[adjoint D={D} equal={equal}] |<Fx, w> - <x, F'w>| / sum |terms| = {diff / scale:.3e}")
            assert diff <= 2.0 ** -20 * scale


# ------------------------------------------------------------------------------------------------------------ bf_geglu_bwd
def _gate_of(arg):
    """The gate whose 2k = g (2c + 2c 0.044715 g^2) is `arg` (bisection in float64)"""
    lo, hi = 0.0, 64.0
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if mid * (K2C + K2CA * mid * mid) < abs(arg) else (lo, mid)
    return float(np.copysign(lo, arg))


def hard_gates(dtype, device="cuda"):
    """test_swiglu_bwd_matches_float64's list of arguments at which exp saturates, underflows or would overflow, as the
    gates whose tanh argument 2k takes those values; +-the dtype's largest finite value, +-0 and the smallest subnormals;
    against every sign of up and dy -> gate, up, dy [8, 96]"""
    args = [-100.0, -30.0, -1.0, 1.0, 30.0, 100.0, -88.0, 88.0, -104.0, 89.0, -20.0, 20.0, 60.0, -60.0, 5.0, -5.0, 8.0, -8.0]
    big, tiny = torch.finfo(dtype).max, torch.finfo(dtype).smallest_normal * torch.finfo(dtype).eps
    hard = torch.tensor([_gate_of(a) for a in args] + [0.0, -0.0, big, -big], dtype=torch.float64).to(dtype)
    hard = torch.cat((hard, torch.tensor([tiny, -tiny], dtype=torch.float64).to(dtype)))
    assert hard.numel() == 24 and float(hard[-2]) > 0.0
    gate = hard.repeat(8, 4).to(device)
    up = torch.tensor([1.0, -1.0, 0.5, -0.25]).repeat_interleave(24)[None].repeat(8, 1).to(device, dtype)
    dy = torch.tensor([1.0, -1.0, 0.5, -0.5, -0.75, 0.75, -0.375, 0.375])[:, None].repeat(1, 96).to(device, dtype)
    return gate, up, dy


def geglu_bounds(rg, ru, mag, dtype):
    return ULP[dtype] * rg.abs() + 144 * U * mag + TINY[dtype], (ULP[dtype] + 96 * U) * ru.abs() + TINY[dtype]


def emulate_geglu_bwd(gate, up, dy, dtype):
    g, u, d = gate.float().cpu(), up.float().cpu(), dy.float().cpu()
    gd = g.double()
    arg = (gd * (gd * gd * K2CA + K2C)).float()
    e = torch.exp(-arg.abs())
    big = 1.0 / (1.0 + e)
    small = e * big
    s, ms = torch.where(arg >= 0, big, small), torch.where(arg >= 0, small, big)
    f = (s.double() * ((gd * (gd * gd * (3.0 * K2CA) + K2C)) * ms.double() + 1.0)).float()
    return (d * (u * f)).to(dtype), (d * (g * s)).to(dtype)


def _geglu_bwd_check(dgate, dup, gate, up, dy, dtype, what):
    rg, ru, mag = geglu_bwd_ref(gate, up, dy)
    bg, bu = geglu_bounds(rg, ru, mag, dtype)
    a, b = _ratio(dgate, rg, bg), _ratio(dup, ru, bu)
    assert a <= 1.0 and b <= 1.0, (what, a, b)
    eg, eu = emulate_geglu_bwd(gate, up, dy, dtype)
    return max(a, b), max(_ratio(eg, rg.cpu(), bg.cpu()), _ratio(eu, ru.cpu(), bu.cpu()))


@pytest.mark.parametrize("name", list(DTYPES))
def test_geglu_bwd_matches_float64(name):
    from bayeformers_amd import ops

    dtype = DTYPES[name]
    gen = torch.Generator().manual_seed(56)
    worst = emu = 0.0
    for rows, N in ((1, 64), (7, 2816), (33, 8200)):
        gate, up, dy = _randn(gen, rows, N, dtype=dtype, scale=3.0), _randn(gen, rows, N, dtype=dtype), _randn(gen, rows, N, dtype=dtype)
        before = ops.FAMILY_BLOCK_BWD_CALLS["geglu"]
        dgate, dup = ops.geglu_backward(gate, up, dy)
        assert ops.FAMILY_BLOCK_BWD_CALLS["geglu"] - before == 1 and dgate.shape == dup.shape == gate.shape
        w, e = _geglu_bwd_check(dgate, dup, gate, up, dy, dtype, (rows, N))
        worst, emu = max(worst, w), max(emu, e)
        # the two halves of one stacked [rows, 2N] buffer, as inputs and as outputs: the same bits
        both = torch.cat((gate, up), -1)
        sg, su = ops.geglu_backward(both[:, :N], both[:, N:], dy, stacked=True)
        assert sg.untyped_storage().data_ptr() == su.untyped_storage().data_ptr() and sg.stride(0) == su.stride(0) == 2 * N
        assert torch.equal(sg, dgate) and torch.equal(su, dup), (rows, N)
    gate, up, dy = hard_gates(dtype)
    dgate, dup = ops.geglu_backward(gate, up, dy)
    w, e = _geglu_bwd_check(dgate, dup, gate, up, dy, dtype, "hard gates")
    worst, emu = max(worst, w), max(emu, e)
    gf, dg, du = gate.float(), dgate.float(), dup.float()
    big = float(torch.finfo(dtype).max)
    # the exact limits: g -> +inf gives (dy u, dy g), g -> -inf (0, 0); 2k = -100: below the smallest normal number
    assert torch.equal(dg[gf == big], (dy.float() * up.float())[gf == big].to(dtype).float())
    assert torch.equal(du[gf == big], (dy.double() * big)[gf == big].to(dtype).float())
    assert not dg[gf == -big].any() and not du[gf == -big].any()
    far = gf == float(torch.tensor(_gate_of(-100.0), dtype=torch.float64).to(dtype))
    assert far.any() and bool((dg[far].abs() <= TINY[dtype]).all()) and bool((du[far].abs() <= TINY[dtype]).all())
    zero = gf == 0.0  # +-0: dgate = dy u / 2
    assert torch.equal(dg[zero], (dy.float() * up.float() * 0.5)[zero].to(dtype).float()) and not du[zero].any()
    assert ops.geglu_backward(gate.view(2, 4, 96), up.view(2, 4, 96), dy.view(2, 4, 96))[0].shape == (2, 4, 96)
    print(f"[geglu_bwd {name}] worst error / bound {worst:.3f}, fp32 emulation {emu:.3f}")
    assert emu <= 1.0


# ------------------------------------------------ one rounding must not lose to autograd's chain of roundings
@pytest.mark.parametrize("name", ["bf16", "fp16"])
def test_backward_kernels_are_no_worse_than_autograds_chains(name):
    """On the same 16-bit inputs each backward kernel's maximum error against float64 is not larger than the error of the
    framework's backward of the unfused op chain (transformers' modules in the 16-bit dtype).  The parameter gradients are
    compared as the kernels emit them, in fp32."""
    import torch.nn.functional as F
    from transformers.models.gemma2.modeling_gemma2 import Gemma2RMSNorm
    from transformers.models.qwen3.modeling_qwen3 import Qwen3RMSNorm, apply_rotary_pos_emb

    from bayeformers_amd import ops

    dtype = DTYPES[name]
    gen = torch.Generator().manual_seed(57)
    rows, N = 512, 1152
    x, res, dy, dz_in, gp, go = norm_inputs(gen, rows, N, dtype)
    x, res = x.requires_grad_(), res.requires_grad_()
    pre, out = Gemma2RMSNorm(N, eps=1e-6).to("cuda", dtype), Gemma2RMSNorm(N, eps=1e-6).to("cuda", dtype)
    with torch.no_grad():
        pre.weight.copy_(gp.to(dtype)), out.weight.copy_(go.to(dtype))
    h = res + pre(x)
    cx, cr, cgp, cgo = torch.autograd.grad([out(h), h], [x, res, pre.weight, out.weight], [dy, dz_in])
    z, wp, wo = h.detach(), pre.weight.detach(), out.weight.detach()  # (the chain's own sum: both differentiate one function)
    dx, dz, dgp, dgo = ops.norm_add_rmsnorm_backward(x.detach(), z, wp, wo, dy, 1e-6, 1e-6, 1, grad_sum=dz_in)
    ref = norm_add_rmsnorm_bwd_ref(x.detach(), z, wp, wo, dy, 1e-6, 1e-6, 1, dz_in=dz_in)
    for what, got, chain in (("dx", dx, cx), ("dz", dz, cr), ("dgamma_pre", dgp, cgp), ("dgamma_out", dgo, cgo)):
        ek, ec = float((got.double() - ref[what]).abs().max()), float((chain.double() - ref[what]).abs().max())
        print(f"[{name}] norm_add_rmsnorm_bwd {what} max error {ek:.4e}, autograd chain {ec:.4e}")
        assert ek <= ec

    for D, norms in ((256, False), (128, True)):  # Gemma 2's rotation at head size 256; Qwen3's q / k norms in front of it
        wq, wk, q, k, cos, sin, gq, gk = rope_inputs(gen, dtype, 2, 256, 8, 2, D, "view", 1, dtype, True)
        q, k = q.detach().requires_grad_(), k.detach().requires_grad_()
        if norms:
            qn, kn = Qwen3RMSNorm(D, eps=1e-6).to("cuda", dtype), Qwen3RMSNorm(D, eps=1e-6).to("cuda", dtype)
            with torch.no_grad():
                qn.weight.copy_(gq.to(dtype)), kn.weight.copy_(gk.to(dtype))
            gq, gk = qn.weight.detach(), kn.weight.detach()
            chain = torch.autograd.grad(list(apply_rotary_pos_emb(qn(q), kn(k), cos, sin)), [q, k, qn.weight, kn.weight], [wq, wk])
        else:
            gq = gk = None
            chain = torch.autograd.grad(list(apply_rotary_pos_emb(q, k, cos, sin)), [q, k], [wq, wk]) + (None, None)
        kq, kk, kgq, kgk = ops.qknorm_rope_backward(wq, wk, cos, sin, q.detach(), k.detach(), gq, gk, 1e-6, 0)
        rq, rk = (qknorm_rope_bwd_ref(w, cos, sin, t.detach(), g, 1e-6, 0) for w, t, g in ((wq, q, gq), (wk, k, gk)))
        for what, got, ch, r in (("dq", kq, chain[0], rq[0]), ("dk", kk, chain[1], rk[0]), ("dgamma_q", kgq, chain[2], rq[2]),
                                 ("dgamma_k", kgk, chain[3], rk[2])):
            if got is None:
                continue
            ek, ec = float((got.double() - r).abs().max()), float((ch.double() - r).abs().max())
            print(f"[{name}] qknorm_rope_bwd D={D} {what} max error {ek:.4e}, autograd chain {ec:.4e}")
            assert ek <= ec

    N = 2816
    gate, up = _randn(gen, rows, N, dtype=dtype, scale=3.0).requires_grad_(), _randn(gen, rows, N, dtype=dtype).requires_grad_()
    dy = _randn(gen, rows, N, dtype=dtype)
    cgate, cup = torch.autograd.grad(F.gelu(gate, approximate="tanh") * up, [gate, up], dy)
    kgate, kup = ops.geglu_backward(gate.detach(), up.detach(), dy)
    rg, ru, _ = geglu_bwd_ref(gate.detach(), up.detach(), dy)
    for what, got, chain, r in (("dgate", kgate, cgate, rg), ("dup", kup, cup, ru)):
        ek, ec = float((got.double() - r).abs().max()), float((chain.double() - r).abs().max())
        print(f"[{name}] geglu_bwd {what} max error {ek:.4e}, autograd chain {ec:.4e}")
        assert ek <= ec


# ------------------------------------------------------------------------------- the autograd functions, on their own
def test_autograd_functions_route_the_gradients_and_cast_the_dgammas():
    from bayeformers_amd import ops

    gen = torch.Generator().manual_seed(58)
    bf16 = torch.bfloat16
    x, r, w1, w2, gp, go = norm_inputs(gen, 9, 512, bf16)
    x, r = x.requires_grad_(), r.requires_grad_()
    gp, go = gp.to(bf16).requires_grad_(), go.to(bf16).requires_grad_()
    before = dict(ops.FAMILY_BLOCK_BWD_CALLS)
    z, y = ops.NormAddRMSNormFn.apply(x, gp, r, go, 1e-6, 1e-5, 1)
    gx, gr, ggp, ggo = torch.autograd.grad([y, z], [x, r, gp, go], [w1, w2])
    dx, dz, dgp, dgo = ops.norm_add_rmsnorm_backward(x.detach(), z.detach(), gp.detach(), go.detach(), w1, 1e-6, 1e-5, 1, grad_sum=w2)
    assert torch.equal(gx, dx) and torch.equal(gr, dz) and ggp.dtype == bf16 and torch.equal(ggp, dgp.to(bf16))
    assert torch.equal(ggo, dgo.to(bf16))
    # only the sum used: with gamma_pre stage 1 still runs (dy = NULL), without it the add's own backward, no launch
    z, y = ops.NormAddRMSNormFn.apply(x, gp, r, go, 1e-6, 1e-5, 1)
    gx, gr, ggp = torch.autograd.grad(z, [x, r, gp], w2)
    dx, dz, dgp, _ = ops.norm_add_rmsnorm_backward(x.detach(), z.detach(), gp.detach(), go.detach(), None, 1e-6, 1e-5, 1, grad_sum=w2)
    assert torch.equal(gx, dx) and torch.equal(gr, w2) and torch.equal(ggp, dgp.to(bf16))
    calls = ops.FAMILY_BLOCK_BWD_CALLS["norm_add_norm"]
    z, y = ops.NormAddRMSNormFn.apply(x, None, r, go, 0.0, 1e-5, 1)
    assert torch.equal(torch.autograd.grad(z, r, w2)[0], w2) and ops.FAMILY_BLOCK_BWD_CALLS["norm_add_norm"] == calls
    # no gamma_pre, no residual: one output
    y0 = ops.NormAddRMSNormFn.apply(x, None, None, go, 0.0, 1e-5, 1)
    assert torch.equal(torch.autograd.grad(y0, x, w1)[0],
                       ops.norm_add_rmsnorm_backward(None, x.detach(), None, go.detach(), w1, 0.0, 1e-5, 1)[0])
    wq, wk, q, k, cos, sin, gq, gk = rope_inputs(gen, bf16, 2, 5, 4, 2, 64, "bhtd", 1, torch.float32, True)
    q, k, gq = q.requires_grad_(), k.requires_grad_(), gq.to(bf16).requires_grad_()
    oq, ok = ops.QKNormRopeFn.apply(q, k, cos, sin, gq, None, 1e-6, 0)
    assert oq.data_ptr() != q.data_ptr() and oq.transpose(1, 2).is_contiguous()  # out of place
    gq_, gk_, gg = torch.autograd.grad([oq, ok], [q, k, gq], [wq, wk])
    rq, rk, rg, none = ops.qknorm_rope_backward(wq, wk, cos, sin, q.detach(), None, gq.detach(), None, 1e-6, 0)
    assert none is None and torch.equal(gq_, rq) and torch.equal(gk_, rk) and gg.dtype == bf16 and torch.equal(gg, rg.to(bf16))
    gate, up = _randn(gen, 9, 512, dtype=bf16).requires_grad_(), _randn(gen, 9, 512, dtype=bf16).requires_grad_()
    dg, du = torch.autograd.grad(ops.GeGLUFn.apply(gate, up), [gate, up], w1)
    kg, ku = ops.geglu_backward(gate.detach(), up.detach(), w1)
    assert torch.equal(dg, kg) and torch.equal(du, ku)
    moved = {k: ops.FAMILY_BLOCK_BWD_CALLS[k] - before[k] for k in before}
    assert moved == {"norm_add_norm": 6, "qknorm_rope": 2, "geglu": 2}, moved


# ------------------------------------------------------------------------------------ whole models, fused both ways
from test_gpu_family_blocks import EXPECT, L, _model, _shake_norms, softcap_on  # noqa: E402,F401

T_PROMPT, PAD, S, NB = 64, 9, 2, 4


def _layers(model):
    return next(m.layers for m in model.modules() if isinstance(getattr(m, "layers", None), torch.nn.ModuleList))


def _moved(now, was):
    return {k: now[k] - was[k] for k in was}


def _step(kind, dtype=torch.bfloat16, fuse=True, blocks="all", train=False, prepare=None):
    """One ELBO training step of the two-layer recipe on a padded prompt -> (loss, {name: grad}, counters moved, model)"""
    from test_gpu_causal_attention import _token_nll
    from test_gpu_head256_attention import _prompt

    import bayeformers_amd as bf
    from bayeformers_amd import ops
    from bayeformers_amd.sampling import elbo, sample_bayesian

    ids, mask = _prompt(T=T_PROMPT, pad=PAD)
    model = _shake_norms(_model(kind, dtype, fuse))
    for p in model.parameters():
        p.requires_grad_(p.dtype.is_floating_point)
    if blocks is not None:
        assert bf.fuse_decoder_blocks(model, backward=blocks, families="all") == L
    if train:
        model.train()
    if prepare is not None:
        prepare(model)
    counters = (ops.FAMILY_BLOCK_CALLS, ops.BLOCK_CALLS, ops.FAMILY_BLOCK_BWD_CALLS, ops.BLOCK_BWD_CALLS, ops.GQA_CALLS,
                ops.SOFTCAP_CALLS)
    before = [dict(c) for c in counters]
    bf.manual_seed(SEED)
    _, mean, lp, lq = sample_bayesian(model, {"input_ids": ids, "attention_mask": mask, "use_cache": False}, S)
    loss = elbo(lp, lq, _token_nll(mean[0].float(), ids, mask).double(), NB)
    loss.backward()
    moved = tuple(_moved(c, b) for c, b in zip(counters, before))
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    return loss.detach().clone(), grads, moved, model


@functools.lru_cache(maxsize=None)
def _fused_step(kind):
    """The eager fused bf16 step of a kind, computed once for the tests that compare against it; nobody changes it."""
    return _step(kind)[:3]


def _assert_same_grads(grads, ref, what):
    assert grads.keys() == ref.keys(), (what, set(grads) ^ set(ref))
    for n in ref:
        assert torch.equal(grads[n], ref[n]), (what, n)


@pytest.mark.parametrize("kind", list(EXPECT))
def test_fused_training_step_launches_and_accuracy(kind, softcap_on):
    """fuse_attention + fuse_decoder_blocks(backward="all", families="all") in bf16: the forward launches are EXPECT's, the
    backward launches per kind equal them, the attention backward ran; and against the fp32 unfused model every parameter
    tensor's e = max |g - g_ref| / max |g_ref| is at most 2 e_unfused16 + 2^-8 (the project's margin between two
    implementations of one rounding class, and one bf16 spacing of the tensor's largest element).  At most a quarter of the
    tensors may have a bound decided by the absolute term."""
    loss, grads, (fam, old, fam_b, old_b, gqa, cap) = _fused_step(kind)
    exp_fam, exp_old, _, exp_cap = EXPECT[kind]
    assert fam == exp_fam and old == exp_old and fam_b == exp_fam and old_b == exp_old, (fam, old, fam_b, old_b)
    assert gqa["bwd"] + gqa["bwd_window"] + cap["bwd"] == L and (cap["bwd"] > 0) == (exp_cap > 0), (gqa, cap)
    _, ref, moved_ref, _ = _step(kind, dtype=torch.float32, fuse=False, blocks=None)
    _, plain, moved16, _ = _step(kind, fuse=False, blocks=None)
    assert not any(v for m in moved_ref[:4] + moved16[:4] for v in m.values())
    assert ref.keys() == plain.keys() == grads.keys()
    bad, by_abs, norms = {}, 0, 0
    for n in sorted(ref):
        top = float(ref[n].double().abs().max())
        if top == 0.0:
            continue
        assert torch.isfinite(grads[n]).all(), n
        ef = float((grads[n].double() - ref[n].double()).abs().max()) / top
        e16 = float((plain[n].double() - ref[n].double()).abs().max()) / top
        by_abs += 2 * e16 < 2.0 ** -8
        norms += n.endswith("norm.weight")
        print(f"[{kind} bf16] {n}: fused {ef:.3e}, unfused {e16:.3e}")
        if ef > 2 * e16 + 2.0 ** -8:
            bad[n] = (ef, e16)
    print(f"[{kind} bf16] {by_abs} of {len(ref)} tensors have a bound decided by the absolute term")
    assert not bad, bad
    assert norms >= (4 * L + 1 if kind != "qwen3" else 2 * L + 1) + (2 * L if kind != "gemma2" else 0), norms
    assert 4 * by_abs <= len(ref)


@pytest.mark.parametrize("kind", list(EXPECT))
def test_training_mode_gives_the_eval_mode_fused_gradients(kind, softcap_on):
    loss, grads, moved = _fused_step(kind)
    loss_t, grads_t, moved_t, _ = _step(kind, train=True)
    assert moved_t[:4] == moved[:4] and torch.equal(loss_t, loss)  # the recipes have no dropout
    _assert_same_grads(grads_t, grads, "train()")


def test_graphed_training_step_replays_the_fused_gemma2_step_bitwise(softcap_on):
    """GraphedTrainingStep on the fused Gemma 2, lr 0: the replayed step's loss and every gradient are the eager fused
    step's bit for bit (no atomics, no allocation in the backward kernels), and the capture enqueued the launches."""
    from test_gpu_causal_attention import _token_nll
    from test_gpu_head256_attention import _prompt

    import bayeformers_amd as bf
    from bayeformers_amd import ops
    from bayeformers_amd.training import GraphedTrainingStep, training_step

    ids, mask = _prompt(T=T_PROMPT, pad=PAD)
    inputs = {"input_ids": ids, "attention_mask": mask, "use_cache": False}
    model = _shake_norms(_model("gemma2", torch.bfloat16, True))
    for p in model.parameters():
        p.requires_grad_(p.dtype.is_floating_point)
    assert bf.fuse_decoder_blocks(model, backward="all", families="all") == L
    params = dict(model.named_parameters())
    nll = lambda mean: _token_nll(mean[0].float(), ids, mask)
    opt = torch.optim.AdamW([p for p in model.parameters() if p.requires_grad], lr=torch.tensor(0.0, device="cuda"),
                            weight_decay=0.0, fused=True, capturable=True)
    bf.manual_seed(SEED)
    b0 = dict(ops.FAMILY_BLOCK_BWD_CALLS)
    loss_e = float(training_step(model, inputs, S, nll, opt, NB, max_grad_norm=None))
    assert _moved(ops.FAMILY_BLOCK_BWD_CALLS, b0) == EXPECT["gemma2"][0]
    grads_e = {n: p.grad.detach().clone() for n, p in params.items() if p.grad is not None}
    step = GraphedTrainingStep(model, inputs, S, nll, opt, NB, max_grad_norm=None, eager_steps=1)
    try:
        step()
        bf.manual_seed(SEED)
        b1, f1 = dict(ops.FAMILY_BLOCK_BWD_CALLS), dict(ops.FAMILY_BLOCK_CALLS)
        loss_g = float(step())  # capture + replay
        assert step.captures == 1
        captured, captured_fwd = _moved(ops.FAMILY_BLOCK_BWD_CALLS, b1), _moved(ops.FAMILY_BLOCK_CALLS, f1)
        grads_g = {n: p.grad.detach().clone() for n, p in params.items() if p.grad is not None}
    finally:
        step.close()
    print(f"[graphed fused gemma2 step] loss {loss_g:.6f} (eager {loss_e:.6f}); launches enqueued while capturing: "
          f"forward {captured_fwd}, backward {captured}")
    assert captured == EXPECT["gemma2"][0] and captured_fwd == EXPECT["gemma2"][0]
    assert loss_g == loss_e
    _assert_same_grads(grads_g, grads_e, "graph replay")


@pytest.mark.parametrize("reentrant", [True, False])
@pytest.mark.parametrize("kind", ["gemma2", "qwen3"])
def test_checkpointed_layers_keep_every_gradient(kind, reentrant, softcap_on):
    """Each decoder layer under torch.utils.checkpoint.  use_reentrant=False rebuilds the un-checkpointed graph: every
    gradient is the fused step's bit for bit.  use_reentrant=True runs a layer's first pass under no_grad and leaves a
    graph-less `_bf_normed` on a hidden state that requires grad, which the next norm must not take: no gradient is lost,
    the final norm's weight and the first layer's input norm's among them.  The norm behind a layer boundary is then a node
    of its own, and the recomputed layer's last norm -> add -> norm sees only its sum used: its first norm's backward still
    runs (dy = NULL), so a sandwich layer makes one more backward launch per boundary."""
    from torch.utils.checkpoint import checkpoint

    def wrap(model):
        for layer in _layers(model):
            inner = layer.forward
            layer.forward = (lambda h, *a, _f=inner, **kw:
                             checkpoint(functools.partial(_f, **kw), h, *a, use_reentrant=reentrant))

    loss, grads, moved = _fused_step(kind)
    loss_c, grads_c, moved_c, _ = _step(kind, prepare=wrap)
    if reentrant:
        assert all(moved_c[i][k] >= moved[i][k] for i in (2, 3) for k in moved[i])
    else:
        assert moved_c[2] == moved[2] and moved_c[3] == moved[3]
    assert all(moved_c[i][k] >= moved[i][k] for i in (0, 1) for k in moved[i])  # the recomputation launches the forwards again
    assert torch.equal(loss_c, loss) and grads_c.keys() == grads.keys(), set(grads_c) ^ set(grads)
    for n in grads:
        if n.endswith("layers.0.input_layernorm.weight") or n.endswith("model.norm.weight"):
            assert grads_c[n] is not None and bool(grads_c[n].any()), n
    assert sum(n.endswith("layers.0.input_layernorm.weight") or n.endswith("model.norm.weight") for n in grads) == 2
    if not reentrant:
        _assert_same_grads(grads_c, grads, "checkpoint(use_reentrant=False)")


# --------------------------------------------------------------------------------------------------------------- declines
def test_backward_true_sets_no_flag_on_the_families_and_a_bad_value_raises(softcap_on):
    import bayeformers_amd as bf

    _, grads, moved, model = _step("gemma3", blocks=True)
    assert not any(v for m in moved[:4] for v in m.values()) and len(grads) > 0
    with pytest.raises(ValueError, match="backward="):
        bf.fuse_decoder_blocks(model, backward="yes", families="all")
    assert bf.fuse_decoder_blocks(model, backward="all", families="all") == 0  # turns the flag on, counts nothing
    assert all(getattr(layer, "_bf_blocks_backward", False) for layer in _layers(model))


def test_active_attention_dropout_runs_the_modules_own_forward(softcap_on):
    def drop(model):
        for layer in _layers(model):
            layer.self_attn.attention_dropout = 0.1

    loss, grads, (fam, _, fam_b, _, _, _), _ = _step("gemma2", train=True, prepare=drop)
    assert fam == dict(EXPECT["gemma2"][0], qknorm_rope=0) and fam_b == fam, (fam, fam_b)
    assert bool(torch.isfinite(loss)) and all(torch.isfinite(v).all() for v in grads.values())


def test_a_hooked_norm_sends_its_layer_to_its_own_forward_the_rest_stays_fused(softcap_on):
    hits = []

    def hook(model):
        _layers(model)[1].pre_feedforward_layernorm.register_forward_hook(lambda m, a, o: hits.append(1))

    loss, grads, (fam, _, fam_b, _, _, _), _ = _step("gemma2", prepare=hook)
    loss0, grads0, _ = _fused_step("gemma2")
    assert hits == [1]
    # layer 1 ran its own forward: its input norm's output came with layer 0's hidden state, the final norm is a launch of
    # its own, and its attention and MLP are still the kernels'
    assert fam == {"norm_add_norm": 4, "qknorm_rope": L, "geglu": L} and fam_b == fam, (fam, fam_b)
    assert grads.keys() == grads0.keys() and all(torch.isfinite(v).all() for v in grads.values())
    assert bool(torch.isfinite(loss))
