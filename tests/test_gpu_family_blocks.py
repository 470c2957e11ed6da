"""bf_norm_add_rmsnorm / bf_qknorm_rope / bf_geglu against the float64 restatement of tests/family_blocks_ref.py, and
fuse_decoder_blocks(families="all") on whole Gemma 2, Gemma 3 and Qwen3 decoders: logits, the arguments the attention
interface receives, generation, and the cases in which the rewrite must step aside.

Tolerances are derived, not measured, by the rules of tests/test_gpu_decoder_blocks.py: inputs are the rounded values of the
tested dtype, the reference is float64 on those, ULP is half the spacing of the output format relative to a power of two
(the most one correct rounding adds, relative to the result) and TINY the absolute term for results the format cannot hold
to that relative precision."""

import pytest
import torch

from family_blocks_ref import geglu_ref, norm_add_rmsnorm_ref, qknorm_rope_ref, rmsnorm64
from test_gpu_decoder_blocks import DTYPES, SEED, TINY, ULP, _randn, _rmsnorm_bound, _rope_inputs

pytestmark = pytest.mark.gpu


def _moved(counter, before):
    return {k: counter[k] - before[k] for k in before}


# -------------------------------------------------------------------------------------------------- bf_norm_add_rmsnorm
def _nan_call(x, gpre, res, gout, off, z, y, eps_pre, eps_out):
    """bf_norm_add_rmsnorm through the C-ABI: every nullable argument as given, outputs where the caller says."""
    from bayeformers_amd import _C, ops

    rows, N = x.shape
    _C.check(_C.lib().bf_norm_add_rmsnorm(x.data_ptr(), gpre.data_ptr() if gpre is not None else None,
                                          res.data_ptr() if res is not None else None, gout.data_ptr(),
                                          ops._TORCH2BF[gout.dtype], off, z.data_ptr() if z is not None else None, y.data_ptr(),
                                          ops._TORCH2BF[x.dtype], rows, N, eps_pre, eps_out,
                                          torch.cuda.current_stream().cuda_stream), "bf_norm_add_rmsnorm")


@pytest.mark.parametrize("name", list(DTYPES))
def test_norm_add_rmsnorm_matches_float64(name):
    """z: with u64 / z64 the restatement's values (rounded where the kernel rounds), |z - z64| <= ULP (|u64| + |z64|) + TINY:
    room for one inner rounding that went the other way plus the add's own rounding.  (The kernel evaluates the first norm in
    fp64 so that its rounded u is the restatement's; eps_pre and eps_out are powers of two, the same number as a float and
    as a double.)  Without gamma_pre nothing precedes the add and z is bitwise the framework's `residual + x`.
    y: against the float64 norm of the kernel's OWN z, within test_gpu_decoder_blocks._rmsnorm_bound (one rounding plus the
    fp32 evaluation error of the statistics; the factor weight_offset + gamma adds one fp32 rounding, 2^-24 relative).
    Without sum_out, y is the same bits; so is the in-place form."""
    dtype = DTYPES[name]
    gen = torch.Generator().manual_seed(41)
    eps_pre, eps_out = 2.0 ** -20, 2.0 ** -17
    worst_z = worst_y = 0.0
    for rows in (1, 7, 515):
        for N in (64, 256, 768, 2304, 8192):
            x = _randn(gen, rows, N, dtype=dtype, scale=2.0)
            r = _randn(gen, rows, N, dtype=dtype, scale=3.0)
            w32 = 0.5 * torch.randn(2, N, generator=gen)
            for off in (0, 1):
                g32 = ((1.0 - off) + w32).cuda()  # weights around 1 for offset 0, around 0 for Gemma's (1 + weight)
                for gam in (g32, g32.to(dtype)):
                    for gpre in (gam[0], None):
                        for res in (r, None):
                            what = (rows, N, off, gam.dtype, gpre is not None, res is not None)
                            z = torch.full_like(x, float("nan"))
                            y = torch.empty_like(x)
                            _nan_call(x, gpre, res, gam[1], off, z, y, eps_pre, eps_out)
                            u64, z64, _ = norm_add_rmsnorm_ref(x, gpre, res, gam[1], eps_pre, eps_out, off, dtype)
                            if gpre is None:
                                assert torch.equal(z, r + x if res is not None else x), what
                            else:
                                err = (z.double() - z64).abs()
                                bound = ULP[dtype] * (u64.abs() + z64.abs()) + TINY[dtype]
                                assert torch.isfinite(z).all() and bool((err <= bound).all()), (what, float((err / bound).max()))
                                worst_z = max(worst_z, float((err / bound).max()))
                            y64 = rmsnorm64(z, gam[1], eps_out, off)
                            err = (y.double() - y64).abs()
                            bound = _rmsnorm_bound(y64, dtype)
                            assert torch.isfinite(y).all() and bool((err <= bound).all()), (what, float((err / bound).max()))
                            worst_y = max(worst_y, float((err / bound).max()))
                            y2 = torch.empty_like(x)  # without the sum output
                            _nan_call(x, gpre, res, gam[1], off, None, y2, eps_pre, eps_out)
                            assert torch.equal(y2, y), what
                            xi, ri = x.clone(), (res.clone() if res is not None else None)  # in place: z over the residual, y over x
                            _nan_call(xi, gpre, ri, gam[1], off, ri, xi, eps_pre, eps_out)
                            assert torch.equal(xi, y) and (ri is None or torch.equal(ri, z)), what
    print(f"[norm_add_rmsnorm {name}] worst error / bound: z {worst_z:.3f}, y {worst_y:.3f}")


def test_norm_add_rmsnorm_op():
    from bayeformers_amd import ops

    gen = torch.Generator().manual_seed(42)
    x, r = _randn(gen, 3, 5, 768, dtype=torch.bfloat16), _randn(gen, 3, 5, 768, dtype=torch.bfloat16)
    gp, go = (0.3 * torch.randn(768, generator=gen)).cuda(), (0.3 * torch.randn(768, generator=gen)).cuda()
    before, old = dict(ops.FAMILY_BLOCK_CALLS), dict(ops.BLOCK_CALLS)
    z, y = ops.norm_add_rmsnorm(x, gp, r, go, 1e-6, 1e-6)
    z0, y0 = ops.norm_add_rmsnorm(x, None, None, go, 0.0, 1e-6)
    z1, y1 = ops.norm_add_rmsnorm(x, gp, r, go, 1e-6, 1e-6, want_sum=False)
    assert _moved(ops.FAMILY_BLOCK_CALLS, before) == {"norm_add_norm": 3, "qknorm_rope": 0, "geglu": 0} and ops.BLOCK_CALLS == old
    assert z0 is x and z1 is None and torch.equal(y1, y) and z.shape == y.shape == x.shape
    z64 = norm_add_rmsnorm_ref(x, gp, r, go, 1e-6, 1e-6, 1, torch.bfloat16)[1]
    assert bool(((z.double() - z64).abs() <= ULP[torch.bfloat16] * 2 * z64.abs() + TINY[torch.bfloat16]).all())  # (coarse: the op's plumbing)
    assert bool(((y0.double() - rmsnorm64(x, go, 1e-6, 1)).abs() <= _rmsnorm_bound(rmsnorm64(x, go, 1e-6, 1), torch.bfloat16)).all())
    assert bool(((y.double() - rmsnorm64(z, go, 1e-6, 1)).abs() <= _rmsnorm_bound(rmsnorm64(z, go, 1e-6, 1), torch.bfloat16)).all())
    norm = torch.nn.RMSNorm(768).cuda()
    assert ops.norm_add_rmsnorm_supported(x, norm, r, norm) and not ops.norm_add_rmsnorm_supported(x[..., :60], norm, None, norm)
    assert not ops.norm_add_rmsnorm_supported(x, norm, r.float(), norm)


# ------------------------------------------------------------------------------------------------------- bf_qknorm_rope
def _qkrope_check(got, x, cos, sin, gamma, eps, off, dtype, what):
    y64, mag = qknorm_rope_ref(x, cos, sin, gamma, eps, off)
    err = (got.double() - y64).abs()
    # test_gpu_decoder_blocks._rope_check's bound — one rounding of the result, 2^-20 mag for the fp32 rounding of each
    # product before the two can cancel — with the normaliser's fp32 evaluation error added: rstd from a sum of at most 256
    # squares, two multiplies and the offset add are a few 2^-24 relative on each normalised value, 2^-20 mag again
    bound = ULP[dtype] * y64.abs() + 2.0 ** -19 * mag + TINY[dtype]
    assert torch.isfinite(got).all() and bool((err <= bound).all()), (what, float((err / bound).max()))
    return float((err / bound).max())


@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("D", [64, 128, 256])
def test_qknorm_rope_matches_float64(name, D):
    from bayeformers_amd import ops

    dtype = DTYPES[name]
    gen = torch.Generator().manual_seed(43 + D)
    B, worst, eps = 2, 0.0, 1e-6
    for H, Hkv in ((8, 2), (3, 1)):
        for T in (1, 5, 130):
            for layout in ("view", "bhtd"):
                for cos_batch in (1, B):
                    for cs_dtype in (dtype, torch.float32):
                        q, k, cos, sin = _rope_inputs(gen, dtype, B, T, H, Hkv, D, layout, cos_batch, cs_dtype)
                        w = 0.5 * torch.randn(2, D, generator=gen)
                        for off in (None, 0, 1):  # no gammas; Qwen3's; Gemma 3's.  The gammas in the tables' dtype.
                            g = None if off is None else ((1.0 - off) + w).to("cuda", cs_dtype)
                            gq, gk = (None, None) if g is None else (g[0], g[1])
                            what = (H, Hkv, T, layout, cos_batch, cs_dtype, off)
                            q0, k0 = q.clone(), k.clone()
                            qo, ko = ops.qknorm_rope(q, k, cos, sin, gq, gk, eps=eps, weight_offset=off or 0)
                            assert torch.equal(q, q0) and torch.equal(k, k0) and qo.shape == q.shape and ko.shape == k.shape
                            worst = max(worst, _qkrope_check(qo, q0, cos, sin, gq, eps, off or 0, dtype, what),
                                        _qkrope_check(ko, k0, cos, sin, gk, eps, off or 0, dtype, what))
                            if off is None and D in (64, 128):  # bf_rope_qk's function, its bits
                                rq, rk = ops.rope_qk(q, k, cos, sin)
                                assert torch.equal(qo, rq) and torch.equal(ko, rk), what
                            qc, kc = q.clone(), k.clone()
                            qi, ki = ops.qknorm_rope(qc, kc, cos, sin, gq, gk, eps=eps, weight_offset=off or 0, inplace=True)
                            assert qi is qc and ki is kc and torch.equal(qc, qo) and torch.equal(kc, ko), what
    # one gamma alone: the other tensor is only rotated
    q, k, cos, sin = _rope_inputs(gen, dtype, B, 5, 8, 2, D, "view", 1, torch.float32)
    gq = (1.0 + 0.5 * torch.randn(D, generator=gen)).cuda()
    qo, ko = ops.qknorm_rope(q, k, cos, sin, gq, None, eps=eps)
    _qkrope_check(qo, q, cos, sin, gq, eps, 0, dtype, "gamma_q alone")
    _qkrope_check(ko, k, cos, sin, None, eps, 0, dtype, "gamma_q alone")
    print(f"[qknorm_rope {name} D={D}] worst error / bound {worst:.3f}")


def test_qknorm_rope_grid_stride_loop():
    """B = 2, T = 1024, H = 32, Hkv = 8, D = 256: 2 * 1024 * 40 * 16 = 1.31 M lane-items against the 4096 x 256 = 1.05 M
    lanes of the largest grid, so a quarter of the lanes take a second trip through the loop and the rest leave it."""
    from bayeformers_amd import ops

    dtype = torch.bfloat16
    gen = torch.Generator().manual_seed(44)
    q, k, cos, sin = _rope_inputs(gen, dtype, 2, 1024, 32, 8, 256, "view", 1, torch.float32)
    assert q.shape[0] * q.shape[2] * (q.shape[1] + k.shape[1]) * 16 > 4096 * 256
    g = (0.5 * torch.randn(2, 256, generator=gen)).cuda()
    q0, k0 = q.clone(), k.clone()
    qo, ko = ops.qknorm_rope(q, k, cos, sin, g[0], g[1], eps=1e-6, weight_offset=1)
    assert torch.equal(q, q0) and torch.equal(k, k0)
    _qkrope_check(qo, q0, cos, sin, g[0], 1e-6, 1, dtype, "q")
    _qkrope_check(ko, k0, cos, sin, g[1], 1e-6, 1, dtype, "k")
    ops.qknorm_rope(q, k, cos, sin, g[0], g[1], eps=1e-6, weight_offset=1, inplace=True)
    assert torch.equal(q, qo) and torch.equal(k, ko)


def test_qknorm_rope_refuses_what_it_cannot_run():
    from bayeformers_amd import _C, ops

    gen = torch.Generator().manual_seed(45)
    q, k, cos, sin = _rope_inputs(gen, torch.bfloat16, 2, 8, 4, 2, 256, "view", 1, torch.bfloat16)
    g = torch.ones(256, device="cuda", dtype=torch.bfloat16)
    assert ops.qknorm_rope_supported(q, k, cos, sin) and ops.qknorm_rope_supported(q, k, cos, sin, g, g)
    assert not ops.qknorm_rope_supported(q, k, cos, sin, g, g.float())              # gammas of two dtypes
    assert not ops.qknorm_rope_supported(q, k, cos, sin, g[:128], g[:128])          # a gamma of another length
    assert not ops.qknorm_rope_supported(q, k, cos.float(), sin)                    # mixed table dtypes
    assert not ops.qknorm_rope_supported(q[..., :96], k[..., :96], cos[..., :96].contiguous(), sin[..., :96].contiguous())
    with pytest.raises(_C.BayeFormersAMDError, match="unsupported"):
        ops.qknorm_rope(q, k, cos[:, :4], sin[:, :4])


# ------------------------------------------------------------------------------------------------------------- bf_geglu
def _geglu_check(y, gate, up, dtype, what):
    y64 = geglu_ref(gate, up)
    err = (y.double() - y64).abs()
    # one rounding of the result.  The argument 2k of the exponential reaches about 88 before exp overflows, and where the
    # exponential dominates the denominator an absolute error of the argument is a relative error of y: its rounding to fp32
    # costs up to 88 * 2^-23 = 2^-16.5; exp, the quotient and the product in fp32 (2^-20, as for swiglu) fit beside it in 2^-16
    bound = (ULP[dtype] + 2.0 ** -16) * y64.abs() + TINY[dtype]
    assert torch.isfinite(y).all() and bool((err <= bound).all()), (what, float((err / bound).max()))
    nz = y64 != 0
    assert torch.equal(torch.signbit(y)[nz], torch.signbit(y64)[nz]), what  # signed as the float64 result
    return float((err / bound).max())


@pytest.mark.parametrize("name", list(DTYPES))
def test_geglu_matches_float64(name):
    from bayeformers_amd import ops

    dtype = DTYPES[name]
    gen = torch.Generator().manual_seed(46)
    worst = 0.0
    for rows, N in ((1, 64), (7, 2816), (16, 2816), (4096, 2816), (33, 8200)):
        gate, up = _randn(gen, rows, N, dtype=dtype, scale=4.0), _randn(gen, rows, N, dtype=dtype)
        worst = max(worst, _geglu_check(ops.geglu(gate, up), gate, up, dtype, (rows, N)))
        both = torch.cat((gate, up), -1)  # the two halves of one stacked [rows, 2N] buffer
        g2, u2 = both[:, :N], both[:, N:]
        assert not g2.is_contiguous() or rows == 1
        assert torch.equal(ops.geglu(g2, u2), ops.geglu(gate, up)), (rows, N)
    # gates where exp saturates, leaves the normal range (2k = 88 near gate -10.3) or underflows, against every sign of up
    hard = torch.tensor([-100.0, -30.0, -1.0, 0.0, 1.0, 30.0, 100.0, -10.25, 10.25, -10.5, 9.0, -5.0, 5.0, -0.0, -10.375, -11.0])
    gate = hard.repeat(4, 4).to("cuda", dtype)
    up = torch.tensor([1.0, -1.0, 3.5, -0.25]).repeat_interleave(16)[None].repeat(4, 1).to("cuda", dtype)
    worst = max(worst, _geglu_check(ops.geglu(gate, up), gate, up, dtype, "hard gates"))
    y = ops.geglu(gate, up).float()
    assert bool((y[gate.float() == 100.0].abs() >= 25.0).all()) and bool((y[gate.float() == -100.0] == 0).all())
    assert ops.geglu(gate.view(2, 2, 64), up.view(2, 2, 64)).shape == (2, 2, 64)
    if dtype == torch.float32:  # finite wherever gate * up is: gates beyond the range of their own cube
        big = torch.tensor([3e15, -3e15, 1e30, -1e30, 3e38, -3e38, 1e-30, -1e-30], device="cuda").repeat(8)[None]
        y = ops.geglu(big, torch.full_like(big, 0.5))
        assert torch.isfinite(y).all() and bool((y[big < -1] == 0).all()) and torch.equal(y[big > 1], big[big > 1] * 0.5)
    print(f"[geglu {name}] worst error / bound {worst:.3f}")


# ---------------------------------------------------- one rounding must not lose to the framework's chain of roundings
@pytest.mark.parametrize("name", ["bf16", "fp16"])
def test_kernels_are_no_worse_than_the_torch_op_chains(name):
    """On the same 4096 x 1024 16-bit inputs, geglu's and qknorm_rope's maximum error against float64 is not larger than the
    unfused HF op chain's against the same float64 (the chain rounds to the 16-bit dtype after every op, the kernel once).
    The norm kernel is not in this comparison: HF's Gemma norm computes in fp32 and rounds where the kernel rounds."""
    from transformers.models.gemma3.modeling_gemma3 import Gemma3RMSNorm
    from transformers.models.qwen3.modeling_qwen3 import Qwen3RMSNorm, apply_rotary_pos_emb

    from bayeformers_amd import ops

    dtype = DTYPES[name]
    gen = torch.Generator().manual_seed(47)
    gate, up = _randn(gen, 4096, 1024, dtype=dtype, scale=4.0), _randn(gen, 4096, 1024, dtype=dtype)
    chain = torch.nn.functional.gelu(gate, approximate="tanh") * up
    y64 = geglu_ref(gate, up)
    ek, ec = float((ops.geglu(gate, up).double() - y64).abs().max()), float((chain.double() - y64).abs().max())
    print(f"[{name}] geglu max error {ek:.4e}, torch chain {ec:.4e}")
    assert ek <= ec

    q, k, cos, sin = _rope_inputs(gen, dtype, 4, 1024, 16, 4, 64, "view", 1, dtype)  # 4096 rows of 1024 (q) and 256 (k)
    for cls, off in ((Qwen3RMSNorm, 0), (Gemma3RMSNorm, 1)):
        qn, kn = cls(64, eps=1e-6).to("cuda", dtype), cls(64, eps=1e-6).to("cuda", dtype)
        with torch.no_grad():
            for m in (qn, kn):
                m.weight.copy_(((1.0 - off) + 0.5 * torch.randn(64, generator=gen)).to("cuda", dtype))
            cq, ck = apply_rotary_pos_emb(qn(q), kn(k), cos, sin)
            kq, kk = ops.qknorm_rope(q, k, cos, sin, qn.weight, kn.weight, eps=1e-6, weight_offset=off)
        for what, got, chain, src, m in (("q", kq, cq, q, qn), ("k", kk, ck, k, kn)):
            y64 = qknorm_rope_ref(src, cos, sin, m.weight.detach(), 1e-6, off)[0]
            ek, ec = float((got.double() - y64).abs().max()), float((chain.double() - y64).abs().max())
            print(f"[{name}] qknorm_rope {cls.__name__} {what} max error {ek:.4e}, torch chain {ec:.4e}")
            assert ek <= ec


# ------------------------------------------------------------------------------------------------------- whole decoders
@pytest.fixture
def softcap_on():
    import bayeformers_amd as bf

    bf.softcap_attention()
    yield
    bf.softcap_attention(False)


def _model(kind, dtype, fuse):
    """Two-layer Bayesian decoders of the other GPU tests' recipes: Gemma 2 (head size 256, window then full, a cap that
    shapes the logits, eager attention as the framework side), Gemma 3 text (head size 256, window then full, q / k norms)
    and Qwen3 (head size 64, two window layers, q / k norms)."""
    if kind == "gemma2":
        from test_gpu_softcap_attention import _gemma2

        return _gemma2(dtype, fuse)
    if kind == "gemma3":
        from test_gpu_head256_attention import GEMMA3, _gemma

        return _gemma("gemma3_text", dtype, fuse, **GEMMA3)
    from test_gpu_sliding_window import _decoder

    return _decoder("qwen3", dtype, fuse)


def _shake_norms(model):
    """Gemma's norm weights start at zero and Qwen3's at one: give every norm a weight that shows, the same in every mode
    (rounded to bf16, so the fp32 reference has the 16-bit models' weights)"""
    g = torch.Generator().manual_seed(12)
    with torch.no_grad():
        for name, p in sorted(model.named_parameters()):
            if name.endswith("norm.weight"):
                p.add_((0.25 * torch.randn(p.shape, generator=g)).bfloat16().to(p.device, p.dtype))
    return model


L = 2
EXPECT = {  # per forward: (FAMILY_BLOCK_CALLS, BLOCK_CALLS, GQA_CALLS fwd / fwd_window, SOFTCAP_CALLS fwd)
    "gemma2": ({"norm_add_norm": 2 * L + 1, "qknorm_rope": L, "geglu": L}, {"rmsnorm": 0, "rope": 0, "swiglu": 0}, (0, 0), 2),
    "gemma3": ({"norm_add_norm": 2 * L + 1, "qknorm_rope": L, "geglu": L}, {"rmsnorm": 0, "rope": 0, "swiglu": 0}, (1, 1), 0),
    "qwen3": ({"norm_add_norm": 0, "qknorm_rope": L, "geglu": 0}, {"rmsnorm": 2 * L + 1, "rope": 0, "swiglu": L}, (0, 2), 0),
}


@pytest.mark.parametrize("kind", list(EXPECT))
def test_fused_family_logits_match_the_unfused_model(kind, softcap_on):
    """fuse_attention + fuse_decoder_blocks(families="all") in bf16 against the fp32 unfused model on a padded prompt, under
    test_sliding_decoder_logits_match_sdpa's criterion ef <= 2 e16 + 2e-3 (e16: the unfused bf16 model's error); every layer
    made its launches, and the attention kernels still ran on what the rotary launch left."""
    from test_gpu_head256_attention import _prompt

    import bayeformers_amd as bf
    from bayeformers_amd import ops
    from bayeformers_amd.sampling import sample_bayesian

    ids, mask = _prompt()
    S, outs = 2, {}
    for name, dtype, fuse in (("ref", torch.float32, False), ("plain16", torch.bfloat16, False), ("fused", torch.bfloat16, True)):
        model = _shake_norms(_model(kind, dtype, fuse))
        if fuse:
            assert bf.fuse_decoder_blocks(model) == 0  # the default families leave it alone
            assert bf.fuse_decoder_blocks(model, families="all") == L
        f0, b0, g0, c0 = (dict(d) for d in (ops.FAMILY_BLOCK_CALLS, ops.BLOCK_CALLS, ops.GQA_CALLS, ops.SOFTCAP_CALLS))
        bf.manual_seed(SEED)
        with torch.no_grad():
            raw, _, _, _ = sample_bayesian(model, {"input_ids": ids, "attention_mask": mask, "use_cache": False}, S)
        outs[name] = raw[0].float().view(S, *ids.shape, -1)
        fam, old, gqa, cap = EXPECT[kind] if fuse else ({k: 0 for k in f0}, {k: 0 for k in b0}, (0, 0), 0)
        assert _moved(ops.FAMILY_BLOCK_CALLS, f0) == fam and _moved(ops.BLOCK_CALLS, b0) == old
        moved = _moved(ops.GQA_CALLS, g0)
        assert (moved["fwd"], moved["fwd_window"]) == gqa and ops.SOFTCAP_CALLS["fwd"] - c0["fwd"] == cap
    valid = mask.bool()[None, :, :, None].expand_as(outs["ref"])
    ref = outs["ref"][valid]
    e16 = (outs["plain16"][valid] - ref).abs().max().item() / ref.abs().max().item()
    ef = (outs["fused"][valid] - ref).abs().max().item() / ref.abs().max().item()
    print(f"[{kind}] fused blocks bf16 {ef:.3e}, unfused bf16 {e16:.3e} (max |logit - fp32| / max |fp32|)")
    assert ef <= 2 * e16 + 2e-3


# ------------------------------------------------------------------------------ what the attention interface is handed
def _tiny_hf(kind):
    """A plain (not Bayesian) two-layer bf16 HF model of each family on the device"""
    from transformers import AutoConfig, AutoModelForCausalLM

    extra = {"gemma2": dict(sliding_window=8, layer_types=["sliding_attention", "full_attention"], attn_logit_softcapping=30.0),
             "gemma3_text": dict(sliding_window=8, layer_types=["sliding_attention", "full_attention"]),
             "qwen3": dict(sliding_window=8, use_sliding_window=True, max_window_layers=1,
                           layer_types=["full_attention", "sliding_attention"]), "gemma": {}}[kind]
    cfg = AutoConfig.for_model(kind, hidden_size=128, num_attention_heads=2, num_key_value_heads=1, head_dim=64,
                               num_hidden_layers=2, intermediate_size=256, vocab_size=97, max_position_embeddings=64,
                               tie_word_embeddings=False, attention_dropout=0.0, attn_implementation="sdpa", **extra)
    torch.manual_seed(0)
    return _shake_norms(AutoModelForCausalLM.from_config(cfg).eval().to("cuda", torch.bfloat16))


@pytest.mark.parametrize("kind", ["qwen3", "gemma", "gemma2", "gemma3_text"])
def test_the_attention_interface_gets_the_class_own_arguments(kind):
    """A recording attention function under a fresh name: the plain and the rewritten attention forwards hand it the same
    keyword arguments with the same values, and layer 0's q / k agree with the class's own chain (q_norm / k_norm, then
    apply_rotary_pos_emb) on the rewritten run's own projections — the two runs' projections are not the same tensors where
    the input norm in front of them is a kernel too.  The bound: with y64 and mag the float64 restatement on those
    projections, the kernel is within _qkrope_check's ULP |y| + 2^-19 mag; HF's chain in bf16 rounds the normalised value
    (twice in Qwen3RMSNorm: before and after the weight), each of the two products and the sum: ULP |y| + 3 ULP mag.
    Together 2 ULP |y| + (3 ULP + 2^-19) mag + TINY."""
    import sys

    from transformers import AttentionInterface
    from transformers.integrations.sdpa_attention import sdpa_attention_forward
    from transformers.masking_utils import AttentionMaskInterface, sdpa_mask

    import bayeformers_amd as bf
    from bayeformers_amd import ops

    seen = []

    def recording(module, query, key, value, attention_mask, **kwargs):
        seen.append((module.layer_idx, query.clone(), key.clone(), dict(kwargs)))
        return sdpa_attention_forward(module, query, key, value, attention_mask, **kwargs)

    fresh = f"bf_test_recording_{kind}"
    AttentionInterface.register(fresh, recording)
    AttentionMaskInterface.register(fresh, sdpa_mask)
    model = _tiny_hf(kind)
    for m in model.modules():
        if getattr(m, "config", None) is not None and hasattr(m.config, "_attn_implementation"):
            m.config._attn_implementation = fresh
    attn = model.model.layers[0].self_attn
    grabbed = {}
    hooks = [attn.q_proj.register_forward_hook(lambda m, a, o: grabbed.__setitem__("q", o.clone())),
             attn.k_proj.register_forward_hook(lambda m, a, o: grabbed.__setitem__("k", o.clone())),
             attn.register_forward_pre_hook(lambda m, a, kw: grabbed.__setitem__("pe", kw["position_embeddings"]), with_kwargs=True)]
    ids = torch.randint(0, 97, (2, 12), generator=torch.Generator().manual_seed(5)).cuda()
    with torch.no_grad():
        model(input_ids=ids, use_cache=False)
    plain, seen = seen, []
    assert bf.fuse_decoder_blocks(model, families="all") == 2
    before = dict(ops.FAMILY_BLOCK_CALLS)
    with torch.no_grad():
        model(input_ids=ids, use_cache=False)
    for h in hooks:
        h.remove()
    assert ops.FAMILY_BLOCK_CALLS["qknorm_rope"] - before["qknorm_rope"] == 2
    assert [p[0] for p in plain] == [s[0] for s in seen] == [0, 1]
    for (_, _, _, kp), (_, _, _, kf) in zip(plain, seen):
        assert kp.keys() == kf.keys(), (sorted(kp), sorted(kf))
        for name in kp:
            a, b = kp[name], kf[name]
            assert (torch.equal(a, b) if isinstance(a, torch.Tensor) else type(a) is type(b) and a == b), (name, a, b)
    expect = {"qwen3": {"sliding_window"}, "gemma": set(), "gemma2": {"sliding_window", "softcap"}, "gemma3_text": {"sliding_window"}}
    assert {"dropout", "scaling"} | expect[kind] <= plain[0][3].keys() and not ({"sliding_window", "softcap"} - expect[kind]) & plain[0][3].keys()
    cos, sin = grabbed["pe"]
    off = 0 if kind == "qwen3" else 1
    assert plain[0][1].shape == seen[0][1].shape and plain[0][2].shape == seen[0][2].shape
    xq, xk = (grabbed[n].view(2, 12, -1, 64).transpose(1, 2) for n in "qk")
    with torch.no_grad():
        nq, nk = (attn.q_norm(xq), attn.k_norm(xk)) if hasattr(attn, "q_norm") else (xq, xk)
        chain = sys.modules[type(attn).__module__].apply_rotary_pos_emb(nq, nk, cos, sin)
    for x, norm, got_p, got_f in ((xq, getattr(attn, "q_norm", None), chain[0], seen[0][1]),
                                  (xk, getattr(attn, "k_norm", None), chain[1], seen[0][2])):
        gamma = norm.weight.detach() if norm is not None else None
        eps = (norm.eps if hasattr(norm, "eps") else norm.variance_epsilon) if norm is not None else 0.0
        y64, mag = qknorm_rope_ref(x, cos, sin, gamma, eps, off)
        u = ULP[torch.bfloat16]
        bound = 2 * u * y64.abs() + (3 * u + 2.0 ** -19) * mag + TINY[torch.bfloat16]
        err = (got_f.double() - got_p.double()).abs()
        assert bool((err <= bound).all()), (kind, float((err / bound).max()))
        _qkrope_check(got_f, x, cos, sin, gamma, eps, off, torch.bfloat16, kind)


# ------------------------------------------------------------------------------------------------------------ generation
def test_fused_gemma2_graph_generation_is_static_and_matches_teacher_forcing(softcap_on):
    """bf16 with kept weights on the fused Gemma 2: graph=True returns the static_cache=True Generation field by field, bit
    for bit (the three kernels are captured: no allocation, no synchronisation), the greedy tokens are teacher forcing's on
    the same fused model and the statistics within test_generate_bf16_matches_teacher_forcing_and_pins_log_probs' 0.05."""
    from dataclasses import fields

    import bayeformers_amd as bf
    from bayeformers_amd import ops
    from bayeformers_amd.sampling import mc_predictive, sample_bayesian, sample_generate

    bmodel = _shake_norms(_model("gemma2", torch.bfloat16, True))
    assert bf.fuse_decoder_blocks(bmodel, families="all") == L
    bf.set_compute_dtype("bf16")
    ids = torch.randint(0, 512, (2, 96), generator=torch.Generator().manual_seed(11)).cuda()
    S, n, T0 = 3, 8, ids.shape[1]
    out = {}
    for mode in ("static_cache", "graph"):
        bf.manual_seed(SEED)
        f0, c0 = dict(ops.FAMILY_BLOCK_CALLS), dict(ops.SOFTCAP_CALLS)
        with torch.no_grad():
            out[mode] = sample_generate(bmodel, ids, samples=S, max_new_tokens=n, keep_weights=True, **{mode: True})
        moved = _moved(ops.FAMILY_BLOCK_CALLS, f0)
        if mode == "static_cache":  # eager: the prefill and every one of the n - 1 decode steps
            assert moved == {"norm_add_norm": 5 * n, "qknorm_rope": 2 * n, "geglu": 2 * n}, moved
            assert ops.SOFTCAP_CALLS["decode_len"] - c0["decode_len"] == 2 * (n - 1)
        else:  # enqueued under capture (and its warm-up), replayed after that
            assert moved["qknorm_rope"] >= 2 * 2 and moved["geglu"] >= 2 * 2 and moved["norm_add_norm"] >= 5 * 2, moved
    assert all(torch.equal(getattr(out["graph"], f.name), getattr(out["static_cache"], f.name)) for f in fields(out["graph"]))
    gen = out["graph"]
    bf.manual_seed(SEED)
    with torch.no_grad():
        raw, _, _, _ = sample_bayesian(bmodel, {"input_ids": gen.sequences[:, :-1], "use_cache": False}, S)
    pred = mc_predictive(raw[0][:, :, T0 - 1:])
    assert torch.equal(pred.prediction, gen.sequences[:, T0:])
    for ours, ref in ((gen.predictive_entropy, pred.predictive_entropy), (gen.expected_entropy, pred.expected_entropy),
                      (gen.mutual_information, pred.mutual_information)):
        assert (ours - ref).abs().max().item() < 0.05


# --------------------------------------------------------------------------------------------------------------- declines
def test_hooks_still_fire_and_hooked_modules_keep_their_forward():
    """Gemma 3: a hook on layer 1's pre_feedforward_layernorm sends that layer to its own forward (its input norm still
    hands out what layer 0's second launch attached, the final norm launches alone: 3 + 0 + 1 norm launches instead of 5), one
    on its q_norm sends the attention module to its own forward (1 rotary launch instead of 2); the MLP stays fused."""
    from test_gpu_head256_attention import _prompt

    import bayeformers_amd as bf
    from bayeformers_amd import ops

    bmodel = _shake_norms(_model("gemma3", torch.bfloat16, True))
    bmodel.graph_replay = False  # (a forward replayed from a HIP graph runs no Python: every call below is an eager one)
    assert bf.fuse_decoder_blocks(bmodel, families="gemma3") == L
    layer = bmodel.model.model.layers[1]
    ids, mask = _prompt(T=64, pad=9)
    before = dict(ops.FAMILY_BLOCK_CALLS)
    bf.manual_seed(SEED)
    with torch.no_grad():
        out = bmodel(input_ids=ids, attention_mask=mask, use_cache=False).logits
    assert _moved(ops.FAMILY_BLOCK_CALLS, before) == {"norm_add_norm": 5, "qknorm_rope": 2, "geglu": 2}
    hits = []
    h1 = layer.pre_feedforward_layernorm.register_forward_hook(lambda m, a, o: hits.append("pre_ff"))
    h2 = layer.self_attn.q_norm.register_forward_hook(lambda m, a, o: hits.append("q_norm"))
    before = dict(ops.FAMILY_BLOCK_CALLS)
    bf.manual_seed(SEED)
    with torch.no_grad():
        hooked = bmodel(input_ids=ids, attention_mask=mask, use_cache=False).logits
    assert sorted(hits) == ["pre_ff", "q_norm"]
    assert _moved(ops.FAMILY_BLOCK_CALLS, before) == {"norm_add_norm": 4, "qknorm_rope": 1, "geglu": 2}
    h1.remove(), h2.remove()
    h3 = layer.mlp.act_fn.register_forward_hook(lambda m, a, o: hits.append("act_fn"))
    before = dict(ops.FAMILY_BLOCK_CALLS)
    bf.manual_seed(SEED)
    with torch.no_grad():
        bmodel(input_ids=ids, attention_mask=mask, use_cache=False)
    assert hits[-1] == "act_fn" and _moved(ops.FAMILY_BLOCK_CALLS, before) == {"norm_add_norm": 5, "qknorm_rope": 2, "geglu": 1}
    h3.remove()
    assert torch.isfinite(out).all() and torch.isfinite(hooked).all()
    valid = mask.bool()[:, :, None].expand_as(out)
    # the same function either way, to the bf16 model's own precision
    assert (hooked.float()[valid] - out.float()[valid]).abs().max().item() <= 0.05 * out.float()[valid].abs().max().item()


def test_recorded_gradients_run_the_plain_forwards(softcap_on):
    """A training step on the rewritten Gemma 2: with gradients recorded every new fast form steps aside, so the loss and
    every gradient are the unrewritten model's bit for bit and none of the three kernels is launched."""
    from test_gpu_causal_attention import _token_nll
    from test_gpu_head256_attention import _prompt

    import bayeformers_amd as bf
    from bayeformers_amd import ops
    from bayeformers_amd.sampling import elbo, sample_bayesian

    ids, mask = _prompt(T=64, pad=9)
    results = []
    for blocks in (False, True):
        model = _shake_norms(_model("gemma2", torch.bfloat16, True))
        for p in model.parameters():
            p.requires_grad_(p.dtype.is_floating_point)
        if blocks:
            assert bf.fuse_decoder_blocks(model, backward=True, families="all") == L
        before, old = dict(ops.FAMILY_BLOCK_CALLS), dict(ops.BLOCK_CALLS)
        bf.manual_seed(SEED)
        _, mean, lp, lq = sample_bayesian(model, {"input_ids": ids, "attention_mask": mask, "use_cache": False}, 2)
        loss = elbo(lp, lq, _token_nll(mean[0].float(), ids, mask).double(), 4)
        loss.backward()
        assert ops.FAMILY_BLOCK_CALLS == before and ops.BLOCK_CALLS == old
        results.append((loss.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}))
    (loss0, grads0), (loss1, grads1) = results
    assert torch.equal(loss0, loss1) and grads0.keys() == grads1.keys() and len(grads0) > 0
    assert all(torch.equal(grads0[n], grads1[n]) for n in grads0)
