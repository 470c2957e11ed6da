"""bf_add_rmsnorm_bwd / bf_rope_qk_bwd / bf_swiglu_bwd against the float64 restatement of tests/decoder_blocks_bwd_ref.py,
and fuse_decoder_blocks(backward=True) on decoder_train's training step: eager, graphed, in training mode, checkpointed,
and the cases in which it must step aside.

Tolerances are derived, not measured, with test_gpu_decoder_blocks.py's ULP (u16 below: half the spacing of the output
format, relative) and TINY.  u = 2^-24 is one fp32 rounding.  Every bound is  ULP |ref| + c u mag + TINY  with mag the
magnitude the terms of the result had before they could cancel (the reference returns it) and c counted from the kernel:

  RoPE   dx1 = fma(dy1, c1, fl(dy2 s2)): the product's rounding (u |dy2 s2|) and the fma's (u |dx1|) -> c = 2.
  SwiGLU e = expf(-|g|) 2u (1 ulp), 1 + e 1u, 1 / (1 + e) 1u, e * that 1u: s and 1 - s carry at most 6u each.
         dgate = dy (u (s fma(g, 1 - s, 1))): 6u on the term g (1 - s) (of mag) plus, relative to the result, s 6u, the fma
         1u and three products 3u -> 16u mag, c = 16 = 2^-20 / u.  dup = dy (g s): 6u + 2u <= 16u |ref|.
  RMSNorm the sum of squares is taken in fp64, so r carries one rounding (u).  With D the depth of an fp32 row sum — 8 V
         fused multiply-adds per lane, V <= 4, then 6 tree steps over a wave and 3 adds across a workgroup's waves: D <= 41
         — the row mean of z gamma dy carries (D + 2) u of mean |z gamma dy| (its product, the sum, the division by N).
         dz = fma(-z, k, r (gamma dy)) with k = r r r mean: k (3u of r + 3 products + D + 2) = (D + 8) u on the second
         term, the first term 3u (r, two products), the fma 1u, the add of dz_in 1u -> at most (D + 13) u mag <= 54 u mag:
         c = 64 = 2^-18 / u.
         dgamma (fp32): a term dy z r is formed in fp64 (dy z exact, r unrounded) and added to the fp32 partial sum with
         one rounding; the rows terms of a column are merged by rows - 1 additions in all, whatever the order (lanes, LDS,
         the second launch), u sum |terms| each at most, and the first term of every partial sum is rounded once, u |term|:
         the order-independent rows u sum |dy z r|.  So: ULP32 |ref| + rows u sum |dy z r|.

Before these constants were trusted, an fp32 torch emulation of each kernel's operation order was run on the CPU on the
test's own inputs (the _emulate_* functions; every test runs them on its first case): it stays inside the bounds."""

import functools

import numpy as np
import pytest
import torch

from decoder_blocks_bwd_ref import add_rmsnorm_bwd_ref, rope_bwd_ref, swiglu_bwd_ref

pytestmark = pytest.mark.gpu

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
ULP = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -24}
TINY = {torch.bfloat16: 2.0 ** -126, torch.float16: 2.0 ** -25, torch.float32: 2.0 ** -126}
U = 2.0 ** -24
SEED = 0x5EED


def _randn(gen, *shape, dtype, scale=1.0):
    return (torch.randn(*shape, generator=gen) * scale).to("cuda", dtype)


def _ratio(got, ref, bound):
    err = (got.double() - ref).abs()
    assert torch.isfinite(got).all()
    return float((err / bound).max())


# ---------------------------------------------------------------------------------------------------- bf_add_rmsnorm_bwd
def _rmsnorm_bounds(dz64, dg64, mag, mag_g, rows, dtype):
    return ULP[dtype] * dz64.abs() + 64 * U * mag + TINY[dtype], U * dg64.abs() + rows * U * mag_g + 2.0 ** -126


def _emulate_rmsnorm_bwd(z, gamma, dy, dz_in, eps, dtype):
    """The kernel's operation order in fp32 torch on the CPU (the row sums in torch's own fp32 order; r from an fp64 sum
    of squares and each dgamma term in fp64 before it joins the fp32 sum, as the kernel takes them) -> (dz rounded to
    dtype, dgamma fp32)."""
    z, g, dy = z.float().cpu(), gamma.float().cpu(), dy.float().cpu()
    N = z.shape[-1]
    rd = 1.0 / torch.sqrt((z.double() * z.double()).sum(-1, keepdim=True) / N + float(np.float32(eps)))
    r = rd.float()
    s = ((dy * g) * z).sum(-1, keepdim=True)
    k = r * r * r * (s * np.float32(1.0 / N))
    dz = torch.addcmul(r * (dy * g), -z, k)
    if dz_in is not None:
        dz = dz + dz_in.float().cpu()
    dgamma = torch.zeros(N)
    for row in range(z.shape[0]):
        dgamma = (dgamma.double() + dy[row].double() * z[row].double() * rd[row]).float()
    return dz.to(dtype), dgamma


@pytest.mark.parametrize("name", list(DTYPES))
def test_add_rmsnorm_bwd_matches_float64(name):
    """rows 1 / 7 / 9 / 515 x N 64 (a wave per row, V = 1) / 256, 768 (half a wave per row, V = 1, 3) / 1032 (a vector count
    that is no multiple of 64) / 4096, 8192 (a workgroup per row, V = 2, 4: the largest): an idle half wave, idle waves
    and a partial last workgroup among them; z from the forward with a residual and without, dz_in or none, gamma in fp32
    and in the activation dtype."""
    from bayeformers_amd import ops

    dtype = DTYPES[name]
    gen = torch.Generator().manual_seed(41)
    eps = 1e-5
    worst = [0.0, 0.0, 0.0]
    for rows in (1, 7, 9, 515):
        for N in (64, 256, 768, 1032, 4096, 8192):
            x = _randn(gen, rows, N, dtype=dtype)
            res = _randn(gen, rows, N, dtype=dtype, scale=3.0)
            dy, dz_in = _randn(gen, rows, N, dtype=dtype), _randn(gen, rows, N, dtype=dtype, scale=0.5)
            g32 = (1.0 + 0.5 * torch.randn(N, generator=gen)).cuda()
            first = True
            for gamma in (g32, g32.to(dtype)):
                for r in (res, None):
                    z = ops.add_rmsnorm(x, r, gamma, eps)[0]  # what the forward saved: its sum output, or x itself
                    assert (z is x) if r is None else torch.equal(z, r + x)
                    for h in (dz_in, None):
                        dz, dgamma = ops.add_rmsnorm_backward(z, gamma, dy, eps, grad_sum=h)
                        assert dz.dtype == dtype and dz.shape == z.shape and dgamma.dtype == torch.float32 and dgamma.shape == (N,)
                        dz64, dg64, mag, mag_g = add_rmsnorm_bwd_ref(z, gamma, dy, eps, dz_in=h)
                        bz, bg = _rmsnorm_bounds(dz64, dg64, mag, mag_g, rows, dtype)
                        rz, rg = _ratio(dz, dz64, bz), _ratio(dgamma, dg64, bg)
                        if first:  # the CPU emulation of the kernel's arithmetic sits inside the same bounds
                            ez, eg = _emulate_rmsnorm_bwd(z, gamma, dy, h, eps, dtype)
                            worst[2] = max(worst[2], _ratio(ez, dz64.cpu(), bz.cpu()), _ratio(eg, dg64.cpu(), bg.cpu()))
                            first = False
                        assert rz <= 1.0 and rg <= 1.0, (rows, N, gamma.dtype, r is not None, h is not None, rz, rg)
                        worst[0], worst[1] = max(worst[0], rz), max(worst[1], rg)
    print(f"[add_rmsnorm_bwd {name}] worst error / bound: dz {worst[0]:.3f}, dgamma {worst[1]:.3f}, fp32 emulation {worst[2]:.3f}")
    assert worst[2] <= 1.0


def test_add_rmsnorm_bwd_in_place_and_repeatable():
    """dz over dy (in place) gives the out-of-place bits, and two launches give the same dgamma bit for bit (no atomics)."""
    from bayeformers_amd import _C, ops

    gen = torch.Generator().manual_seed(42)
    rows, N = 515, 768
    z, dy, h = (_randn(gen, rows, N, dtype=torch.bfloat16) for _ in range(3))
    gamma = (1.0 + 0.5 * torch.randn(N, generator=gen)).cuda()
    before = ops.BLOCK_BWD_CALLS["rmsnorm"]
    dz, dg = ops.add_rmsnorm_backward(z, gamma, dy, 1e-6, grad_sum=h)
    dz2, dg2 = ops.add_rmsnorm_backward(z.view(5, 103, N), gamma, dy.view(5, 103, N), 1e-6, grad_sum=h.view(5, 103, N))
    assert ops.BLOCK_BWD_CALLS["rmsnorm"] - before == 2 and dz2.shape == (5, 103, N)
    assert torch.equal(dz2.view(rows, N), dz) and torch.equal(dg2, dg)
    lib = _C.lib()
    ws = torch.empty(lib.bf_add_rmsnorm_bwd_workspace_bytes(rows, N), dtype=torch.uint8, device="cuda")
    dg3, buf = torch.empty_like(dg), dy.clone()
    _C.check(lib.bf_add_rmsnorm_bwd(z.data_ptr(), gamma.data_ptr(), _C.BF_DT_F32, buf.data_ptr(), h.data_ptr(), buf.data_ptr(),
                                    dg3.data_ptr(), ws.data_ptr(), ws.numel(), _C.BF_DT_BF16, rows, N, 1e-6,
                                    torch.cuda.current_stream().cuda_stream), "bf_add_rmsnorm_bwd")
    assert torch.equal(buf, dz) and torch.equal(dg3, dg)


# ------------------------------------------------------------------------------------------------------- bf_rope_qk_bwd
def _rope_inputs(gen, dtype, B, T, H, Hkv, D, layout, cos_batch, cs_dtype, equal):
    if layout == "view":  # gradients laid out [B, T, heads * D] and seen as [B, heads, T, D]
        q = _randn(gen, B, T, H * D, dtype=dtype).view(B, T, H, D).transpose(1, 2)
        k = _randn(gen, B, T, Hkv * D, dtype=dtype).view(B, T, Hkv, D).transpose(1, 2)
    else:
        q, k = _randn(gen, B, H, T, D, dtype=dtype), _randn(gen, B, Hkv, T, D, dtype=dtype)
    if equal:  # what the rotary module returns: the two halves carry the same angles
        ang = torch.rand(cos_batch, T, D // 2, generator=gen, dtype=torch.float64) * 200.0
        ang = torch.cat((ang, ang), -1)
    else:
        ang = torch.rand(cos_batch, T, D, generator=gen, dtype=torch.float64) * 200.0
    return q, k, ang.cos().to("cuda", cs_dtype), ang.sin().to("cuda", cs_dtype)


def _emulate_rope_bwd(dy, cos, sin, dtype):
    dy, c, s = dy.float().cpu(), cos.float().cpu()[:, None], sin.float().cpu()[:, None]
    h = dy.shape[-1] // 2
    d1, d2 = dy[..., :h], dy[..., h:]
    return torch.cat((torch.addcmul(d2 * s[..., h:], d1, c[..., :h]), torch.addcmul(-(d1 * s[..., :h]), d2, c[..., h:])), -1).to(dtype)


@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("D", [64, 128])
def test_rope_qk_bwd_matches_float64(name, D):
    from bayeformers_amd import ops

    dtype = DTYPES[name]
    gen = torch.Generator().manual_seed(43 + D)
    B, worst, emu = 3, 0.0, 0.0
    for H, Hkv in ((8, 8), (8, 2), (16, 1)):
        for T in (1, 5, 128):
            for layout in ("view", "bhtd"):
                for cos_batch in (1, B):
                    for cs_dtype in (dtype, torch.float32):
                        for equal in (True, False):
                            q, k, cos, sin = _rope_inputs(gen, dtype, B, T, H, Hkv, D, layout, cos_batch, cs_dtype, equal)
                            what = (H, Hkv, T, layout, cos_batch, cs_dtype, equal)
                            q0, k0 = q.clone(), k.clone()
                            dq, dk = ops.rope_qk_backward(q, k, cos, sin)
                            assert torch.equal(q, q0) and torch.equal(k, k0) and dq.shape == q.shape and dk.shape == k.shape
                            # laid out [B, T, heads, D]: what the backward of the projections reads
                            assert dq.transpose(1, 2).is_contiguous() and dk.transpose(1, 2).is_contiguous()
                            for got, src in ((dq, q0), (dk, k0)):
                                ref, mag = rope_bwd_ref(src, cos, sin)
                                bound = ULP[dtype] * ref.abs() + 2 * U * mag + TINY[dtype]
                                ratio = _ratio(got, ref, bound)
                                assert ratio <= 1.0, (what, ratio)
                                worst = max(worst, ratio)
                                if T == 5:
                                    emu = max(emu, _ratio(_emulate_rope_bwd(src, cos, sin, dtype), ref.cpu(), bound.cpu()))
    print(f"[rope_qk_bwd {name} D={D}] worst error / bound {worst:.3f}, fp32 emulation {emu:.3f}")
    assert emu <= 1.0


@pytest.mark.parametrize("equal", [True, False])
def test_rope_backward_is_the_adjoint_of_the_forward_kernel(equal):
    """<rope_qk(x), w> = <x, rope_qk_backward(w)> in fp32, the products summed in float64, to 2^-20 of sum |terms|: kernel
    against kernel.  With unequal halves "the forward with -sin" fails this (shown on the same data)."""
    from bayeformers_amd import ops

    gen = torch.Generator().manual_seed(44)
    for D in (64, 128):
        q, k, cos, sin = _rope_inputs(gen, torch.float32, 3, 37, 8, 2, D, "view", 3, torch.float32, equal)
        wq, wk = _randn(gen, *q.shape, dtype=torch.float32), _randn(gen, *k.shape, dtype=torch.float32)
        yq, yk = ops.rope_qk(q, k, cos, sin)
        before = ops.BLOCK_BWD_CALLS["rope"]
        dq, dk = ops.rope_qk_backward(wq, wk, cos, sin)
        assert ops.BLOCK_BWD_CALLS["rope"] - before == 1
        nq, nk = ops.rope_qk(wq, wk, cos, -sin)  # not the adjoint unless the halves are equal
        for y, w, x, d, n in ((yq, wq, q, dq, nq), (yk, wk, k, dk, nk)):
            lhs, rhs = (y.double() * w.double()), (x.double() * d.double())
            scale = float(lhs.abs().sum() + rhs.abs().sum())
            diff = abs(float(lhs.sum() - rhs.sum()))
            wrong = abs(float(lhs.sum() - (x.double() * n.double()).sum()))
            print(f"[adjoint D={D} equal={equal}] |<Rx, w> - <x, R'w>| / sum |terms| = {diff / scale:.3e} (forward with -sin: {wrong / scale:.3e})")
            assert diff <= 2.0 ** -20 * scale
            assert (wrong <= 2.0 ** -20 * scale) == equal


# -------------------------------------------------------------------------------------------------------- bf_swiglu_bwd
def _emulate_swiglu_bwd(gate, up, dy, dtype):
    g, u, d = gate.float().cpu(), up.float().cpu(), dy.float().cpu()
    e = torch.exp(-g.abs())
    big = 1.0 / (1.0 + e)
    small = e * big
    s, ms = torch.where(g >= 0, big, small), torch.where(g >= 0, small, big)
    return (d * (u * (s * torch.addcmul(torch.ones_like(g), g, ms)))).to(dtype), (d * (g * s)).to(dtype)


def _swiglu_bwd_check(dgate, dup, gate, up, dy, dtype, what):
    rg, ru, mag = swiglu_bwd_ref(gate, up, dy)
    bg = ULP[dtype] * rg.abs() + 2.0 ** -20 * mag + TINY[dtype]
    bu = (ULP[dtype] + 2.0 ** -20) * ru.abs() + TINY[dtype]
    a, b = _ratio(dgate, rg, bg), _ratio(dup, ru, bu)
    assert a <= 1.0 and b <= 1.0, (what, a, b)
    eg, eu = _emulate_swiglu_bwd(gate, up, dy, dtype)
    return max(a, b), max(_ratio(eg, rg.cpu(), bg.cpu()), _ratio(eu, ru.cpu(), bu.cpu()))


@pytest.mark.parametrize("name", list(DTYPES))
def test_swiglu_bwd_matches_float64(name):
    from bayeformers_amd import ops

    dtype = DTYPES[name]
    gen = torch.Generator().manual_seed(45)
    worst = emu = 0.0
    for rows, N in ((1, 64), (7, 2816), (33, 8200)):
        gate, up, dy = _randn(gen, rows, N, dtype=dtype, scale=4.0), _randn(gen, rows, N, dtype=dtype), _randn(gen, rows, N, dtype=dtype)
        before = ops.BLOCK_BWD_CALLS["swiglu"]
        dgate, dup = ops.swiglu_backward(gate, up, dy)
        assert ops.BLOCK_BWD_CALLS["swiglu"] - before == 1 and dgate.shape == dup.shape == gate.shape
        w, e = _swiglu_bwd_check(dgate, dup, gate, up, dy, dtype, (rows, N))
        worst, emu = max(worst, w), max(emu, e)
        # the two halves of one stacked [rows, 2N] buffer, as inputs and as outputs: the same bits
        both = torch.cat((gate, up), -1)
        g2, u2 = both[:, :N], both[:, N:]
        sg, su = ops.swiglu_backward(g2, u2, dy, stacked=True)
        assert sg.untyped_storage().data_ptr() == su.untyped_storage().data_ptr() and sg.stride(0) == su.stride(0) == 2 * N
        assert torch.equal(sg, dgate) and torch.equal(su, dup), (rows, N)
    # gates where exp saturates, underflows or would overflow, against every sign of up and dy
    hard = torch.tensor([-100.0, -30.0, -1.0, 0.0, 1.0, 30.0, 100.0, -88.0, 88.0, -104.0, 89.0, -20.0, 20.0, -0.0, 60.0, -60.0])
    gate = hard.repeat(8, 4).to("cuda", dtype)
    up = torch.tensor([1.0, -1.0, 3.5, -0.25]).repeat_interleave(16)[None].repeat(8, 1).to("cuda", dtype)
    dy = torch.tensor([1.0, -1.0, 2.5, -0.5, 1.0, -1.0, 2.5, -0.5])[:, None].repeat(1, 64).to("cuda", dtype)
    dy[4:] = -dy[4:] * 0.75
    dgate, dup = ops.swiglu_backward(gate, up, dy)
    w, e = _swiglu_bwd_check(dgate, dup, gate, up, dy, dtype, "hard gates")
    worst, emu = max(worst, w), max(emu, e)
    gf, dg, du = gate.float(), dgate.float(), dup.float()
    # the limit 0 (in fp32 the true e^-100-sized values themselves, far below the smallest normal number)
    assert bool((dg[gf == -100.0].abs() <= TINY[dtype]).all()) and bool((du[gf == -100.0].abs() <= TINY[dtype]).all())
    assert torch.equal(dg[gf == 100.0], (dy.float() * up.float())[gf == 100.0].to(dtype).float())  # dgate -> dy u
    assert torch.equal(du[gf == 100.0], (dy.float() * 100.0)[gf == 100.0].to(dtype).float())       # dup -> dy g
    assert ops.swiglu_backward(gate.view(2, 4, 64), up.view(2, 4, 64), dy.view(2, 4, 64))[0].shape == (2, 4, 64)
    print(f"[swiglu_bwd {name}] worst error / bound {worst:.3f}, fp32 emulation {emu:.3f}")
    assert emu <= 1.0


# ------------------------------------------------ one rounding must not lose to autograd's chain of roundings
@pytest.mark.parametrize("name", ["bf16", "fp16"])
def test_backward_kernels_are_no_worse_than_autograds_chains(name):
    """On the same 16-bit inputs each backward kernel's maximum error against float64 is not larger than the error of the
    framework's backward of the unfused op chain (which rounds to the 16-bit dtype after every op)."""
    from transformers.models.llama.modeling_llama import LlamaRMSNorm, apply_rotary_pos_emb

    from bayeformers_amd import ops

    dtype = DTYPES[name]
    gen = torch.Generator().manual_seed(46)
    rows, N = 512, 1024
    x, r = _randn(gen, rows, N, dtype=dtype).requires_grad_(), _randn(gen, rows, N, dtype=dtype, scale=3.0)
    dy, dz_in = _randn(gen, rows, N, dtype=dtype), _randn(gen, rows, N, dtype=dtype, scale=0.5)
    norm = LlamaRMSNorm(N, eps=1e-5).to("cuda", dtype)
    with torch.no_grad():
        norm.weight.copy_((1.0 + 0.5 * torch.randn(N, generator=gen)).to("cuda", dtype))
    h = r + x
    cx, cg = torch.autograd.grad([norm(h), h], [x, norm.weight], [dy, dz_in])
    z = h.detach()
    dz, dgamma = ops.add_rmsnorm_backward(z, norm.weight.detach(), dy, norm.variance_epsilon, grad_sum=dz_in)
    dz64, dg64, _, _ = add_rmsnorm_bwd_ref(z, norm.weight.detach(), dy, norm.variance_epsilon, dz_in=dz_in)
    for what, got, chain, ref in (("dz", dz, cx, dz64), ("dgamma", dgamma.to(dtype), cg, dg64)):
        ek, ec = float((got.double() - ref).abs().max()), float((chain.double() - ref).abs().max())
        print(f"[{name}] add_rmsnorm_bwd {what} max error {ek:.4e}, autograd chain {ec:.4e}")
        assert ek <= ec

    q, k, cos, sin = _rope_inputs(gen, dtype, 2, 256, 8, 2, 64, "view", 1, dtype, True)
    q, k = q.detach().requires_grad_(), k.detach().requires_grad_()
    wq, wk = _randn(gen, *q.shape, dtype=dtype), _randn(gen, *k.shape, dtype=dtype)
    cq, ck = torch.autograd.grad(list(apply_rotary_pos_emb(q, k, cos, sin)), [q, k], [wq, wk])
    kq, kk = ops.rope_qk_backward(wq, wk, cos, sin)
    for what, got, chain, w in (("dq", kq, cq, wq), ("dk", kk, ck, wk)):
        ref = rope_bwd_ref(w, cos, sin)[0]
        ek, ec = float((got.double() - ref).abs().max()), float((chain.double() - ref).abs().max())
        print(f"[{name}] rope_qk_bwd {what} max error {ek:.4e}, autograd chain {ec:.4e}")
        assert ek <= ec

    N = 2816
    gate, up = _randn(gen, rows, N, dtype=dtype, scale=4.0).requires_grad_(), _randn(gen, rows, N, dtype=dtype).requires_grad_()
    dy = _randn(gen, rows, N, dtype=dtype)
    cgate, cup = torch.autograd.grad(torch.nn.functional.silu(gate) * up, [gate, up], dy)
    kgate, kup = ops.swiglu_backward(gate.detach(), up.detach(), dy)
    rg, ru, _ = swiglu_bwd_ref(gate.detach(), up.detach(), dy)
    for what, got, chain, ref in (("dgate", kgate, cgate, rg), ("dup", kup, cup, ru)):
        ek, ec = float((got.double() - ref).abs().max()), float((chain.double() - ref).abs().max())
        print(f"[{name}] swiglu_bwd {what} max error {ek:.4e}, autograd chain {ec:.4e}")
        assert ek <= ec


# ------------------------------------------------------------------------------- the autograd functions, on their own
def test_autograd_functions_route_both_gradients_and_cast_dgamma():
    from bayeformers_amd import ops

    gen = torch.Generator().manual_seed(47)
    x, r = _randn(gen, 9, 512, dtype=torch.bfloat16).requires_grad_(), _randn(gen, 9, 512, dtype=torch.bfloat16).requires_grad_()
    gamma = (1.0 + 0.5 * torch.randn(512, generator=gen)).to("cuda", torch.bfloat16).requires_grad_()
    w1, w2 = _randn(gen, 9, 512, dtype=torch.bfloat16), _randn(gen, 9, 512, dtype=torch.bfloat16)
    before = dict(ops.BLOCK_BWD_CALLS)
    z, y = ops.AddRMSNormFn.apply(x, r, gamma, 1e-6)
    gx, gr, gg = torch.autograd.grad([y, z], [x, r, gamma], [w1, w2])
    dz, dgamma = ops.add_rmsnorm_backward(z.detach(), gamma.detach(), w1, 1e-6, grad_sum=w2)
    assert torch.equal(gx, dz) and torch.equal(gr, dz) and gg.dtype == torch.bfloat16 and torch.equal(gg, dgamma.to(torch.bfloat16))
    # only y used: no dz_in; only the sum used: the add's own backward, no launch
    z, y = ops.AddRMSNormFn.apply(x, r, gamma, 1e-6)
    assert torch.equal(torch.autograd.grad(y, x, w1)[0], ops.add_rmsnorm_backward(z.detach(), gamma.detach(), w1, 1e-6)[0])
    calls = ops.BLOCK_BWD_CALLS["rmsnorm"]
    z, y = ops.AddRMSNormFn.apply(x, r, gamma, 1e-6)
    assert torch.equal(torch.autograd.grad(z, r, w2)[0], w2) and ops.BLOCK_BWD_CALLS["rmsnorm"] == calls
    # no residual: one output
    y0 = ops.AddRMSNormFn.apply(x, None, gamma, 1e-6)
    assert torch.equal(torch.autograd.grad(y0, x, w1)[0], ops.add_rmsnorm_backward(x.detach(), gamma.detach(), w1, 1e-6)[0])
    gate, up = _randn(gen, 9, 512, dtype=torch.bfloat16).requires_grad_(), _randn(gen, 9, 512, dtype=torch.bfloat16).requires_grad_()
    dg, du = torch.autograd.grad(ops.SwiGLUFn.apply(gate, up), [gate, up], w1)
    kg, ku = ops.swiglu_backward(gate.detach(), up.detach(), w1)
    assert torch.equal(dg, kg) and torch.equal(du, ku)
    moved = {k: ops.BLOCK_BWD_CALLS[k] - before[k] for k in before}
    assert moved == {"rmsnorm": 6, "rope": 0, "swiglu": 2}, moved


# -------------------------------------------------------------------------------------- decoder_train, fused both ways
def _errors(g, grads, loss, nll):
    """test_decoder_training_step_matches_reference's figures: (loss rel, nll rel, {tensor: error}) with its skip rule."""
    names = [str(n) for n in g["names"]]
    assert sorted(names) == sorted(grads), set(names) ^ set(grads)
    gmax = max(float(g[f"stat/{n}"][2]) for n in names)
    worst = {}
    for n in names:
        got = grads[n].detach().double().cpu().numpy()
        assert np.isfinite(got).all(), n
        ref_sum, ref_abs, ref_max = g[f"stat/{n}"]
        if ref_max < 1e-6 * gmax:
            continue
        worst[n] = abs(np.abs(got).sum() - ref_abs) / ref_abs
        if f"grad/{n}" in g.files:
            worst[n + " (full)"] = np.abs(got - g[f"grad/{n}"].astype(np.float64)).max() / ref_max
    return abs(loss - float(g["loss"])) / abs(float(g["loss"])), abs(nll - float(g["nll"])) / abs(float(g["nll"])), worst


def _step(golden_dir, dtype="bf16", blocks="backward", train=False, prepare=None):
    """One decoder_train training step -> (fixture, loss, nll, {name: grad}, counters moved).  blocks: None (unfused),
    "default" (fuse_decoder_blocks(model)) or "backward"."""
    from test_gpu_causal_attention import _decoder, _token_nll

    import bayeformers_amd as bf
    from bayeformers_amd import ops
    from bayeformers_amd.sampling import elbo, sample_bayesian

    g, bmodel, inputs, ids, mask = _decoder(golden_dir, "decoder_train", dtype)
    assert bf.fuse_attention(bmodel)
    L = int(g["config"][3])
    if blocks is not None:
        assert bf.fuse_decoder_blocks(bmodel, **({"backward": True} if blocks == "backward" else {})) == L
    if train:
        bmodel.train()
    extra = prepare(bmodel) if prepare is not None else None
    before = (dict(ops.BLOCK_CALLS), dict(ops.BLOCK_BWD_CALLS), dict(ops.GQA_CALLS))
    bf.manual_seed(SEED)
    bf.set_compute_dtype(dtype)
    try:
        raw, mean, lp, lq = sample_bayesian(bmodel, inputs, int(g["config"][8]))
        nll = _token_nll(mean[0].float(), ids, mask)
        loss = elbo(lp, lq, nll.double(), int(g["n_batches"]))
        loss.backward()
    finally:
        bf.set_compute_dtype("bf16")
    moved = tuple({k: now[k] - was[k] for k in was}
                  for was, now in zip(before, (ops.BLOCK_CALLS, ops.BLOCK_BWD_CALLS, ops.GQA_CALLS)))
    grads = {n: p.grad.detach().clone() for n, p in bmodel.named_parameters() if p.grad is not None}
    return g, float(loss.detach()), float(nll), grads, moved, extra


@functools.lru_cache(maxsize=None)
def _fused_bf16_step(golden_dir):
    """The eager fused bf16 step, computed once for the tests that compare against it; nobody changes what it returns."""
    return _step(golden_dir)


def _launches(L):
    return {"rmsnorm": 2 * L + 1, "rope": L, "swiglu": L}


def test_fused_training_step_matches_reference(golden_dir):
    """decoder_train (bf16) with fuse_attention + fuse_decoder_blocks(backward=True) against the reference, held to
    test_decoder_training_step_matches_reference's criteria as they stand — loss rel 1e-6, full rho gradients 2.1e-2 of
    max, sum |g| 3e-3, the same skip rule — the norm weights' gradients among the tensors compared; the unfused run's
    errors are printed beside the fused ones."""
    g, loss, nll, grads, (fwd, bwd, gqa), _ = _fused_bf16_step(golden_dir)
    _, loss0, nll0, grads0, (fwd0, bwd0, _), _ = _step(golden_dir, blocks=None)
    L = int(g["config"][3])
    el, en, worst = _errors(g, grads, loss, nll)
    el0, en0, worst0 = _errors(g, grads0, loss0, nll0)
    print(f"[decoder_train bf16] fused   loss rel {el:.2e}, nll rel {en:.2e}; unfused loss rel {el0:.2e}, nll rel {en0:.2e}")
    for k in sorted(worst, key=lambda k: -worst[k]):
        print(f"[decoder_train bf16] {k}: fused {worst[k]:.2e}, unfused {worst0[k]:.2e}")
    assert fwd == _launches(L) and bwd == _launches(L), (fwd, bwd)
    assert gqa["fwd"] == L and gqa["bwd"] == L
    assert not any(fwd0.values()) and not any(bwd0.values())
    assert el <= 1e-6
    assert sum(k.endswith("(full)") for k in worst) == 2
    norms = [k for k in worst if k.endswith("norm.weight")]
    assert len(norms) == 2 * L + 1, norms
    assert all(v <= (2.1e-2 if k.endswith("(full)") else 3e-3) for k, v in worst.items()), worst


def test_fused_training_step_fp32_matches_reference_like_the_unfused_step(golden_dir):
    """The same step on an fp32 model under set_compute_dtype("fp32"): the formulas without 16-bit rounding.  Fused and
    unfused are each compared with the fixture's reference gradients; a fused error may be at most 2x the unfused error
    of the same run plus 1e-7 of max |g| (the model's largest gradient element), in the unit of each figure: over the
    tensor's max for a full tensor's figure, over sum |g_ref| for the sum |g| figure."""
    g, loss, nll, grads, (fwd, bwd, _), _ = _step(golden_dir, dtype="fp32")
    _, loss0, nll0, grads0, _, _ = _step(golden_dir, dtype="fp32", blocks=None)
    L = int(g["config"][3])
    assert fwd == _launches(L) and bwd == _launches(L), (fwd, bwd)
    el, en, worst = _errors(g, grads, loss, nll)
    el0, en0, worst0 = _errors(g, grads0, loss0, nll0)
    print(f"[decoder_train fp32] fused loss rel {el:.2e}, nll rel {en:.2e}; unfused loss rel {el0:.2e}, nll rel {en0:.2e}")
    names = [str(n) for n in g["names"]]
    gmax = max(float(g[f"stat/{n}"][2]) for n in names)
    bad = {}
    for k in sorted(worst, key=lambda k: -worst[k]):
        n = k[:-len(" (full)")] if k.endswith("(full)") else k
        ref_sum, ref_abs, ref_max = g[f"stat/{n}"]
        slack = 1e-7 * gmax / (ref_max if k.endswith("(full)") else ref_abs)
        print(f"[decoder_train fp32] {k}: fused {worst[k]:.2e}, unfused {worst0[k]:.2e}")
        if worst[k] > 2 * worst0[k] + slack:
            bad[k] = (worst[k], worst0[k])
    assert el <= 2 * el0 + 1e-7 and not bad, bad
    assert any(k.endswith("norm.weight") for k in worst)


def test_graphed_training_step_replays_the_fused_step_bitwise(golden_dir):
    """GraphedTrainingStep on the fused model, lr 0: the replayed step's loss and every gradient are the eager fused
    step's bit for bit (no atomics, no allocation in the backward kernels), and the capture enqueued L backward launches
    of each kind (2 L + 1 of the norm's)."""
    from test_gpu_causal_attention import _decoder, _token_nll

    import bayeformers_amd as bf
    from bayeformers_amd import ops
    from bayeformers_amd.training import GraphedTrainingStep, training_step

    g, bmodel, inputs, ids, mask = _decoder(golden_dir, "decoder_train", "bf16")
    params = dict(bmodel.named_parameters())
    S, NB, L = int(g["config"][8]), int(g["n_batches"]), int(g["config"][3])
    assert bf.fuse_attention(bmodel) and bf.fuse_decoder_blocks(bmodel, backward=True) == L
    nll = lambda mean: _token_nll(mean[0].float(), ids, mask)
    opt = torch.optim.AdamW([p for p in bmodel.parameters() if p.requires_grad], lr=torch.tensor(0.0, device="cuda"),
                            weight_decay=0.0, fused=True, capturable=True)
    bf.set_compute_dtype("bf16")
    bf.manual_seed(SEED)
    b0 = dict(ops.BLOCK_BWD_CALLS)
    loss_e = float(training_step(bmodel, inputs, S, nll, opt, NB, max_grad_norm=None))
    assert {k: ops.BLOCK_BWD_CALLS[k] - b0[k] for k in b0} == _launches(L)
    grads_e = {n: p.grad.detach().clone() for n, p in params.items() if p.grad is not None}
    step = GraphedTrainingStep(bmodel, inputs, S, nll, opt, NB, max_grad_norm=None, eager_steps=1)
    try:
        step()
        bf.manual_seed(SEED)
        b1, f1 = dict(ops.BLOCK_BWD_CALLS), dict(ops.BLOCK_CALLS)
        loss_g = float(step())  # capture + replay
        assert step.captures == 1
        captured = {k: ops.BLOCK_BWD_CALLS[k] - b1[k] for k in b1}
        captured_fwd = {k: ops.BLOCK_CALLS[k] - f1[k] for k in f1}
        grads_g = {n: p.grad.detach().clone() for n, p in params.items() if p.grad is not None}
    finally:
        step.close()
    print(f"[graphed fused training step] loss {loss_g:.6f} (eager {loss_e:.6f}); launches enqueued while capturing: "
          f"forward {captured_fwd}, backward {captured}")
    assert captured == _launches(L) and captured_fwd == _launches(L)
    assert loss_g == loss_e and grads_g.keys() == grads_e.keys()
    for n in grads_e:
        assert torch.equal(grads_g[n], grads_e[n]), n
    _, _, worst = _errors(g, grads_g, loss_g, float("nan"))
    assert all(v <= (2.1e-2 if k.endswith("(full)") else 3e-3) for k, v in worst.items()), worst


def _assert_same_grads(grads, ref, what):
    assert grads.keys() == ref.keys(), (what, set(grads) ^ set(ref))
    for n in ref:
        assert grads[n] is not None and torch.equal(grads[n], ref[n]), (what, n)


def test_training_mode_gives_the_eval_mode_fused_gradients(golden_dir):
    g, loss, nll, grads, (fwd, bwd, _), _ = _fused_bf16_step(golden_dir)
    _, loss_t, _, grads_t, (fwd_t, bwd_t, _), _ = _step(golden_dir, train=True)
    assert fwd_t == fwd and bwd_t == bwd and loss_t == loss  # the fixture has no dropout
    _assert_same_grads(grads_t, grads, "train()")


@pytest.mark.parametrize("reentrant", [True, False])
def test_checkpointed_layers_keep_every_gradient(golden_dir, reentrant):
    """Each decoder layer under torch.utils.checkpoint: no gradient is lost — the final norm's gamma and the first
    layer's input norm's among them.  Reentrant checkpointing runs a layer's first pass under no_grad and leaves a
    graph-less `_bf_normed` on a hidden state that requires grad: the next norm must not take it, or its gamma has no
    gradient.
    use_reentrant=False rebuilds the un-checkpointed graph: every gradient is the fused step's bit for bit.
    use_reentrant=True cuts the graph at every layer boundary, so the norm behind a boundary is a node of its own there:
    its dz reaches the hidden state rounded to bf16 and autograd adds the residual path's gradient with a second rounding,
    where the un-checkpointed step hands that gradient to the kernel as dz_in and rounds the sum once.  That is L extra
    bf16 roundings (2^-8 relative each) on the hidden-state gradient, nothing else: the gradients are held to the
    fixture's own criteria and to 2 L 2^-8 of each tensor's max against the fused step's."""
    from torch.utils.checkpoint import checkpoint

    def wrap(bmodel):
        for layer in bmodel.model.model.layers:
            inner = layer.forward
            layer.forward = (lambda h, *a, _f=inner, **kw:
                             checkpoint(functools.partial(_f, **kw), h, *a, use_reentrant=reentrant))

    g, loss, nll, grads, (fwd, bwd, _), _ = _fused_bf16_step(golden_dir)
    _, loss_c, nll_c, grads_c, (fwd_c, bwd_c, _), _ = _step(golden_dir, prepare=wrap)
    L = int(g["config"][3])
    assert bwd_c == bwd and all(fwd_c[k] >= fwd[k] for k in fwd)  # the recomputation launches the forwards again
    assert loss_c == loss
    assert grads_c.keys() == grads.keys(), set(grads_c) ^ set(grads)
    for n in ("model.model.norm.weight", "model.model.layers.0.input_layernorm.weight"):
        assert grads_c.get(n) is not None, n
    diff = {n: float((grads_c[n].double() - grads[n].double()).abs().max() / grads[n].double().abs().max().clamp_min(1e-300))
            for n in grads}
    top = max(diff, key=diff.get)
    print(f"[checkpoint reentrant={reentrant}] forward launches {fwd_c}, backward launches {bwd_c}; "
          f"largest max |g - g_fused| / max |g_fused|: {diff[top]:.3e} ({top})")
    if not reentrant:
        _assert_same_grads(grads_c, grads, "checkpoint(use_reentrant=False)")
        return
    el, en, worst = _errors(g, grads_c, loss_c, nll_c)
    assert all(v <= (2.1e-2 if k.endswith("(full)") else 3e-3) for k, v in worst.items()), worst
    assert all(v <= 2 * L * 2.0 ** -8 for v in diff.values()), {n: v for n, v in diff.items() if v > 2 * L * 2.0 ** -8}


# --------------------------------------------------------------------------------------------------------------- declines
def test_default_rewrite_launches_no_backward_kernel(golden_dir):
    _, _, _, grads, (fwd, bwd, _), _ = _step(golden_dir, blocks="default")
    assert not any(fwd.values()) and not any(bwd.values()) and len(grads) > 0


def test_hooked_modules_keep_their_forward_the_rest_stays_fused(golden_dir):
    hits = []

    def hook(bmodel):
        layer = bmodel.model.model.layers[1]
        return (layer.mlp.act_fn.register_forward_hook(lambda m, a, o: hits.append(1)),
                layer.post_attention_layernorm.register_forward_hook(lambda m, a, o: hits.append(2)))

    g, loss, nll, grads, (fwd, bwd, gqa), handles = _step(golden_dir, prepare=hook)
    for h in handles:
        h.remove()
    assert sorted(hits) == [1, 2]
    # layer 1 ran its own forward (its input norm and the final norm are still the kernel's), its MLP its own activation
    assert fwd == {"rmsnorm": 4, "rope": 2, "swiglu": 1} and bwd == fwd, (fwd, bwd)
    el, en, worst = _errors(g, grads, loss, nll)
    assert el <= 1e-6 and all(v <= (2.1e-2 if k.endswith("(full)") else 3e-3) for k, v in worst.items()), worst


def test_active_attention_dropout_runs_the_modules_own_forward(golden_dir):
    def drop(bmodel):
        for layer in bmodel.model.model.layers:
            layer.self_attn.attention_dropout = 0.1

    g, loss, nll, grads, (fwd, bwd, _), _ = _step(golden_dir, train=True, prepare=drop)
    L = int(g["config"][3])
    assert fwd == dict(_launches(L), rope=0) and bwd == fwd, (fwd, bwd)
    assert np.isfinite(loss) and all(torch.isfinite(v).all() for v in grads.values())
