"""bf_add_rmsnorm / bf_rope_qk / bf_swiglu against the float64 restatement of tests/decoder_blocks_ref.py, and
fuse_decoder_blocks on whole decoders: the reference's fixtures, generation, and the cases in which it must step aside.

Tolerances are derived, not measured.  Inputs are the rounded values of the tested dtype, the reference is float64 on
those, and ULP below is half the spacing of the output format relative to a power of two (2^-8 bf16, 2^-11 fp16, 2^-24
fp32): the most a single correct rounding can add, relative to the result.  TINY is the absolute term for results the
format cannot hold to that relative precision: half the fp16 subnormal spacing (2^-25), and for bf16 / fp32 the smallest
normal fp32 (2^-126) — the arithmetic runs in fp32 registers, which is also the exponent range of bf16."""

import numpy as np
import pytest
import torch

from decoder_blocks_ref import add_rmsnorm_ref, rope_ref, swiglu_ref

pytestmark = pytest.mark.gpu

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
ULP = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -24}
TINY = {torch.bfloat16: 2.0 ** -126, torch.float16: 2.0 ** -25, torch.float32: 2.0 ** -126}
SEED = 0x5EED


def _randn(gen, *shape, dtype, scale=1.0):
    return (torch.randn(*shape, generator=gen) * scale).to("cuda", dtype)


# ------------------------------------------------------------------------------------------------------- bf_add_rmsnorm
def _rmsnorm(x, res, gamma, eps, want_sum):
    """bf_add_rmsnorm through the C-ABI with every combination of its two nullable arguments -> (z or None, y)."""
    from bayeformers_amd import _C, ops

    rows, N = x.shape
    z = torch.full_like(x, float("nan")) if want_sum else None
    y = torch.empty_like(x)
    _C.check(_C.lib().bf_add_rmsnorm(x.data_ptr(), res.data_ptr() if res is not None else None, gamma.data_ptr(),
                                     ops._TORCH2BF[gamma.dtype], z.data_ptr() if z is not None else None, y.data_ptr(),
                                     ops._TORCH2BF[x.dtype], rows, N, eps, torch.cuda.current_stream().cuda_stream),
             "bf_add_rmsnorm")
    return z, y


def _rmsnorm_bound(y64, dtype):
    # 16-bit: one ULP (half of it is the single rounding; the fp32 evaluation error, at most (N/64 + 8) 2^-24 relative on
    # the sum of squares at N <= 8192, is orders below the other half).  fp32: 2e-5, above the worst-case accumulation bound
    # at N = 8192.
    if dtype == torch.float32:
        return 2e-5 * y64.abs() + TINY[dtype]
    return ULP[dtype] * y64.abs() + (2.0 ** -24 if dtype == torch.float16 else 0.0)


@pytest.mark.parametrize("name", list(DTYPES))
def test_add_rmsnorm_matches_float64(name):
    dtype = DTYPES[name]
    gen = torch.Generator().manual_seed(21)
    eps = 1e-5
    worst = 0.0
    for rows in (1, 7, 4096):
        for N in (64, 512, 1024, 4096, 8192):
            x = _randn(gen, rows, N, dtype=dtype)
            r = _randn(gen, rows, N, dtype=dtype, scale=3.0)
            g32 = (1.0 + 0.5 * torch.randn(N, generator=gen)).cuda()
            for gamma in (g32, g32.to(dtype)):
                for res in (r, None):
                    for want_sum in (True, False):
                        z, y = _rmsnorm(x, res, gamma, eps, want_sum)
                        z64, y64 = add_rmsnorm_ref(x, res, gamma, eps, dtype)
                        if want_sum:  # one rounding of the fp32 sum: the framework's own add, bit for bit
                            assert torch.equal(z, r + x if res is not None else x), (rows, N)
                        err = (y.double() - y64).abs()
                        bound = _rmsnorm_bound(y64, dtype)
                        assert torch.isfinite(y).all() and bool((err <= bound).all()), \
                            (rows, N, gamma.dtype, res is not None, want_sum, float((err / bound).max()))
                        worst = max(worst, float((err / bound).max()))
    print(f"[add_rmsnorm {name}] worst error / bound {worst:.3f}")


def test_add_rmsnorm_op_and_in_place():
    from bayeformers_amd import ops

    gen = torch.Generator().manual_seed(22)
    x, r = _randn(gen, 3, 5, 512, dtype=torch.bfloat16), _randn(gen, 3, 5, 512, dtype=torch.bfloat16)
    gamma = torch.ones(512, device="cuda")
    before = dict(ops.BLOCK_CALLS)
    z, y = ops.add_rmsnorm(x, r, gamma, 1e-6)
    z0, y0 = ops.add_rmsnorm(x, None, gamma, 1e-6)
    assert ops.BLOCK_CALLS["rmsnorm"] - before["rmsnorm"] == 2 and z0 is x and z.shape == y.shape == x.shape
    assert torch.equal(z, r + x)
    # in place: the sum over the residual, the normalised rows over x
    x2, r2 = x.clone().view(15, 512), r.clone().view(15, 512)
    from bayeformers_amd import _C

    _C.check(_C.lib().bf_add_rmsnorm(x2.data_ptr(), r2.data_ptr(), gamma.data_ptr(), _C.BF_DT_F32, r2.data_ptr(), x2.data_ptr(),
                                     _C.BF_DT_BF16, 15, 512, 1e-6, torch.cuda.current_stream().cuda_stream), "bf_add_rmsnorm")
    assert torch.equal(r2.view_as(z), z) and torch.equal(x2.view_as(y), y)


# ----------------------------------------------------------------------------------------------------------- bf_rope_qk
def _rope_inputs(gen, dtype, B, T, H, Hkv, D, layout, cos_batch, cs_dtype):
    if layout == "view":  # the projections' [B, T, heads * D] outputs seen as [B, heads, T, D]
        q = _randn(gen, B, T, H * D, dtype=dtype).view(B, T, H, D).transpose(1, 2)
        k = _randn(gen, B, T, Hkv * D, dtype=dtype).view(B, T, Hkv, D).transpose(1, 2)
    else:
        q, k = _randn(gen, B, H, T, D, dtype=dtype), _randn(gen, B, Hkv, T, D, dtype=dtype)
    ang = torch.rand(cos_batch, T, D // 2, generator=gen, dtype=torch.float64) * 200.0
    ang = torch.cat((ang, ang), -1)  # what the rotary module returns: the two halves carry the same angles
    return q, k, ang.cos().to("cuda", cs_dtype), ang.sin().to("cuda", cs_dtype)


def _rope_check(got, x, cos, sin, dtype, what):
    y64, mag = rope_ref(x, cos, sin)
    err = (got.double() - y64).abs()
    # one rounding of the result, plus the fp32 rounding of each product before the two can cancel in the sum
    bound = ULP[dtype] * y64.abs() + 2.0 ** -20 * mag + TINY[dtype]
    assert torch.isfinite(got).all() and bool((err <= bound).all()), (what, float((err / bound).max()))
    return float((err / bound).max())


@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("D", [64, 128])
def test_rope_qk_matches_float64(name, D):
    from bayeformers_amd import ops

    dtype = DTYPES[name]
    gen = torch.Generator().manual_seed(23 + D)
    B, worst = 3, 0.0
    for H, Hkv in ((8, 8), (8, 2), (16, 1)):
        for T in (1, 5, 128, 384):
            for layout in ("view", "bhtd"):
                for cos_batch in (1, B):
                    for cs_dtype in (dtype, torch.float32):
                        q, k, cos, sin = _rope_inputs(gen, dtype, B, T, H, Hkv, D, layout, cos_batch, cs_dtype)
                        what = (H, Hkv, T, layout, cos_batch, cs_dtype)
                        q0, k0 = q.clone(), k.clone()
                        qo, ko = ops.rope_qk(q, k, cos, sin)  # out of place: the inputs stay
                        assert torch.equal(q, q0) and torch.equal(k, k0) and qo.shape == q.shape and ko.shape == k.shape
                        worst = max(worst, _rope_check(qo, q0, cos, sin, dtype, what), _rope_check(ko, k0, cos, sin, dtype, what))
                        qi, ki = ops.rope_qk(q, k, cos, sin, inplace=True)
                        assert qi is q and ki is k and torch.equal(q, qo) and torch.equal(k, ko), what
    print(f"[rope_qk {name} D={D}] worst error / bound {worst:.3f}")


def test_rope_qk_refuses_what_it_cannot_run():
    from bayeformers_amd import _C, ops

    gen = torch.Generator().manual_seed(24)
    q, k, cos, sin = _rope_inputs(gen, torch.bfloat16, 2, 8, 4, 2, 64, "view", 1, torch.bfloat16)
    assert ops.rope_supported(q, k, cos, sin)
    assert not ops.rope_supported(q, k, cos[..., :32], sin[..., :32])          # a partial rotary table
    assert not ops.rope_supported(q, k, cos.float(), sin)                      # mixed table dtypes
    assert not ops.rope_supported(q[..., :48], k[..., :48], cos[..., :48].contiguous(), sin[..., :48].contiguous())
    assert not ops.rope_supported(q, k.float(), cos, sin)
    with pytest.raises(_C.BayeFormersAMDError, match="unsupported"):
        ops.rope_qk(q, k, cos[:, :4], sin[:, :4])


# ------------------------------------------------------------------------------------------------------------ bf_swiglu
def _swiglu_check(y, gate, up, dtype, what):
    y64 = swiglu_ref(gate, up)
    err = (y.double() - y64).abs()
    # one rounding of the result; 2^-20 relative for exp, the quotient and the product in fp32
    bound = (ULP[dtype] + 2.0 ** -20) * y64.abs() + TINY[dtype]
    assert torch.isfinite(y).all() and bool((err <= bound).all()), (what, float((err / bound).max()))
    nz = y64 != 0
    assert torch.equal(torch.signbit(y)[nz], torch.signbit(y64)[nz]), what  # signed as the float64 result, zeros included
    return float((err / bound).max())


@pytest.mark.parametrize("name", list(DTYPES))
def test_swiglu_matches_float64(name):
    from bayeformers_amd import ops

    dtype = DTYPES[name]
    gen = torch.Generator().manual_seed(25)
    worst = 0.0
    for rows, N in ((1, 64), (7, 2816), (16, 2816), (4096, 2816), (33, 8200)):
        gate, up = _randn(gen, rows, N, dtype=dtype, scale=4.0), _randn(gen, rows, N, dtype=dtype)
        worst = max(worst, _swiglu_check(ops.swiglu(gate, up), gate, up, dtype, (rows, N)))
        both = torch.cat((gate, up), -1)  # the two halves of one stacked [rows, 2N] buffer
        g2, u2 = both[:, :N], both[:, N:]
        assert not g2.is_contiguous() or rows == 1
        assert torch.equal(ops.swiglu(g2, u2), ops.swiglu(gate, up)), (rows, N)
    # gates where exp saturates or overflows, against every sign of up
    hard = torch.tensor([-100.0, -30.0, -1.0, 0.0, 1.0, 30.0, 100.0, -88.0, 88.0, -104.0, 89.0, -20.0, 20.0, -0.0, 60.0, -60.0])
    gate = hard.repeat(4, 4).to("cuda", dtype)
    up = torch.tensor([1.0, -1.0, 3.5, -0.25]).repeat_interleave(16)[None].repeat(4, 1).to("cuda", dtype)
    worst = max(worst, _swiglu_check(ops.swiglu(gate, up), gate, up, dtype, "hard gates"))
    y = ops.swiglu(gate, up).float()
    assert bool((y[gate.float() == 100.0].abs() >= 25.0).all()) and bool((y[gate.float() == -100.0] == 0).all())
    assert ops.swiglu(gate.view(2, 2, 64), up.view(2, 2, 64)).shape == (2, 2, 64)
    print(f"[swiglu {name}] worst error / bound {worst:.3f}")


# ---------------------------------------------------- one rounding must not lose to the framework's chain of roundings
@pytest.mark.parametrize("name", ["bf16", "fp16"])
def test_kernels_are_no_worse_than_the_torch_op_chains(name):
    """On the same 16-bit inputs each kernel's maximum error against float64 is not larger than the unfused torch op
    chain's against the same float64: the chain rounds to the 16-bit dtype after every op, the kernel once."""
    from transformers.models.llama.modeling_llama import LlamaRMSNorm, apply_rotary_pos_emb

    from bayeformers_amd import ops

    dtype = DTYPES[name]
    gen = torch.Generator().manual_seed(26)
    rows, N = 4096, 1024
    x, r = _randn(gen, rows, N, dtype=dtype), _randn(gen, rows, N, dtype=dtype, scale=3.0)
    norm = LlamaRMSNorm(N, eps=1e-5).to("cuda", dtype)
    with torch.no_grad():
        norm.weight.copy_((1.0 + 0.5 * torch.randn(N, generator=gen)).to("cuda", dtype))
        h = r + x
        chain = norm(h)
        z, y = ops.add_rmsnorm(x, r, norm.weight, norm.variance_epsilon)
    _, y64 = add_rmsnorm_ref(x, r, norm.weight.detach(), norm.variance_epsilon, dtype)
    assert torch.equal(z, h)
    ek, ec = float((y.double() - y64).abs().max()), float((chain.double() - y64).abs().max())
    print(f"[{name}] add_rmsnorm max error {ek:.4e}, torch chain {ec:.4e}")
    assert ek <= ec

    q, k, cos, sin = _rope_inputs(gen, dtype, 4, 384, 16, 4, 64, "view", 1, dtype)
    cq, ck = apply_rotary_pos_emb(q, k, cos, sin)
    kq, kk = ops.rope_qk(q, k, cos, sin)
    for what, got, chain, src in (("q", kq, cq, q), ("k", kk, ck, k)):
        y64 = rope_ref(src, cos, sin)[0]
        ek, ec = float((got.double() - y64).abs().max()), float((chain.double() - y64).abs().max())
        print(f"[{name}] rope_qk {what} max error {ek:.4e}, torch chain {ec:.4e}")
        assert ek <= ec

    gate, up = _randn(gen, rows, 2816, dtype=dtype, scale=4.0), _randn(gen, rows, 2816, dtype=dtype)
    chain = torch.nn.functional.silu(gate) * up
    y64 = swiglu_ref(gate, up)
    ek, ec = float((ops.swiglu(gate, up).double() - y64).abs().max()), float((chain.double() - y64).abs().max())
    print(f"[{name}] swiglu max error {ek:.4e}, torch chain {ec:.4e}")
    assert ek <= ec


# ------------------------------------------------------------------------------------------ whole decoders: the fixtures
def _fixture_run(golden_dir, name, dtype, blocks):
    """test_decoder_matches_reference's run (tests/test_gpu_causal_attention.py), with fuse_decoder_blocks or without."""
    from test_gpu_causal_attention import _decoder, _logits_and_last_hidden, _token_nll

    import bayeformers_amd as bf
    from bayeformers_amd import ops
    from bayeformers_amd.sampling import sample_bayesian

    g, bmodel, inputs, ids, mask = _decoder(golden_dir, name, dtype)
    assert bf.fuse_attention(bmodel)
    layers = int(g["config"][3])
    if blocks:
        assert bf.fuse_decoder_blocks(bmodel) == layers
    before = dict(ops.BLOCK_CALLS)
    gqa = ops.GQA_CALLS["fwd"]
    S = int(g["config"][8])
    bf.manual_seed(SEED)
    bf.set_compute_dtype(dtype)
    try:
        with torch.no_grad():
            raw, mean, lp, lq = sample_bayesian(bmodel, dict(inputs, output_hidden_states=True), S, select=_logits_and_last_hidden)
    finally:
        bf.set_compute_dtype("bf16")
    moved = {k: ops.BLOCK_CALLS[k] - before[k] for k in before}
    B, T = ids.shape
    logits = raw[0].float().view(S, B, T, -1)
    hidden = raw[1].float().view(S, B, T, -1)
    pos = [tuple(p) for p in g["positions"].tolist()]
    got_l = torch.stack([logits[:, b, t] for b, t in pos], 1).cpu().numpy()
    got_h = torch.stack([hidden[:, b, t] for b, t in pos], 1).cpu().numpy()
    assert np.isfinite(got_l).all() and np.isfinite(got_h).all()
    err_l = float(np.abs(got_l - g["logits"]).max() / np.abs(g["logits"]).max())
    err_h = float(np.abs(got_h - g["hidden"]).max() / np.abs(g["hidden"]).max())
    nll = np.array([float(_token_nll(logits[s], ids, mask)) for s in range(S)])
    err_n = float(np.abs(nll - g["token_nll"]).max())
    lps = bmodel.log_prob_samples().cpu().numpy()
    return g, layers, moved, (err_l, err_h, err_n), lps, ops.GQA_CALLS["fwd"] - gqa


def _decoder_cases():
    from test_gpu_causal_attention import DECODER_CASES

    return DECODER_CASES


@pytest.mark.parametrize("name,dtype,tol_logit,tol_hidden,tol_nll", _decoder_cases())
def test_fused_decoder_matches_reference(golden_dir, name, dtype, tol_logit, tol_hidden, tol_nll):
    """The reference's per-sample outputs (decoder_mha64 / decoder_gqa64 / decoder_mqa128) with fuse_attention plus
    fuse_decoder_blocks, held to DECODER_CASES' bounds as they stand; the unfused model's errors are printed beside the
    fused model's.  Every layer made its four launches."""
    _, _, _, plain, _, _ = _fixture_run(golden_dir, name, dtype, blocks=False)
    g, L, moved, fused, lps, gqa = _fixture_run(golden_dir, name, dtype, blocks=True)
    print(f"[{name} {dtype}] fused   logits {fused[0]:.3e}, hidden {fused[1]:.3e}, token nll {fused[2]:.3e}")
    print(f"[{name} {dtype}] unfused logits {plain[0]:.3e}, hidden {plain[1]:.3e}, token nll {plain[2]:.3e}"
          f"   (bounds {tol_logit:.1e}, {tol_hidden:.1e}, {tol_nll:.1e})")
    assert moved == {"rmsnorm": 2 * L + 1, "rope": L, "swiglu": L}
    assert fused[0] < tol_logit and fused[1] < tol_hidden and fused[2] < tol_nll
    np.testing.assert_allclose(lps[:, 0], g["log_prior"], rtol=2e-6)
    np.testing.assert_allclose(lps[:, 1], g["lvp"], rtol=2e-6)
    if dtype == "bf16":
        assert gqa == L  # the causal kernels still read q and k where the rotary launch left them


# ------------------------------------------------------------------------------------------------------------ generation
def test_fused_generate_matches_reference_fixture(golden_dir):
    """generate_gqa64 (fp32 greedy generation against the reference recomputing the whole sequence every step) on fused
    blocks: the same tokens, the statistics within 1e-4; every decode step ran the three kernels."""
    from transformers import LlamaConfig, LlamaForCausalLM

    import bayeformers_amd as bf
    from bayeformers_amd import ops
    from bayeformers_amd.sampling import sample_generate

    g = np.load(f"{golden_dir}/generate_gqa64.npz")
    hidden, heads, kv_heads, layers, ffn, vocab, T0, B, S, n, pad = (int(x) for x in g["config"])
    cfg = LlamaConfig(hidden_size=hidden, num_attention_heads=heads, num_key_value_heads=kv_heads, num_hidden_layers=layers,
                      intermediate_size=ffn, vocab_size=vocab, max_position_embeddings=64, tie_word_embeddings=False,
                      use_cache=False, attention_dropout=0.0, attn_implementation="sdpa")
    torch.manual_seed(int(g["model_seed"]))
    bmodel = bf.to_bayesian(LlamaForCausalLM(cfg).eval(), delta=float(g["delta"]), freeze=True).eval().cuda()
    assert bf.fuse_attention(bmodel) and bf.fuse_decoder_blocks(bmodel) == layers
    before = dict(ops.BLOCK_CALLS)
    bf.set_compute_dtype("fp32")
    bf.manual_seed(SEED)
    try:
        with torch.no_grad():
            gen = sample_generate(bmodel, torch.from_numpy(g["ids"]).cuda(), torch.from_numpy(g["mask"]).cuda(), samples=S,
                                  max_new_tokens=n, temperature=float(g["temperature"]))
    finally:
        bf.set_compute_dtype("bf16")
    # the prefill and n - 1 decode steps, each a whole forward
    assert {k: ops.BLOCK_CALLS[k] - before[k] for k in before} == {"rmsnorm": (2 * layers + 1) * n, "rope": layers * n,
                                                                     "swiglu": layers * n}
    assert np.array_equal(gen.sequences[:, T0:].cpu().numpy(), g["tokens"])
    for name in ("predictive_entropy", "expected_entropy", "mutual_information", "token_prob"):
        np.testing.assert_allclose(getattr(gen, name).cpu().numpy(), g[name], rtol=0, atol=1e-4, err_msg=name)
    np.testing.assert_allclose(gen.log_prior.cpu().numpy(), g["log_prior"], rtol=2e-6)
    np.testing.assert_allclose(gen.log_variational_posterior.cpu().numpy(), g["lvp"], rtol=2e-6)


def test_fused_generate_bf16_graph_is_static_and_matches_teacher_forcing():
    """bf16 with kept weights on fused blocks: graph=True returns the static_cache=True Generation bit for bit (the three
    kernels are captured: no allocation, no synchronisation), and the greedy tokens are teacher forcing's on the fused
    model, the statistics within test_generate_bf16_matches_teacher_forcing_and_pins_log_probs' 0.05."""
    from dataclasses import fields

    from test_gpu_generate import _llama, _prompt

    import bayeformers_amd as bf
    from bayeformers_amd import ops
    from bayeformers_amd.sampling import mc_predictive, sample_bayesian, sample_generate

    bmodel = _llama(torch.bfloat16)
    assert bf.fuse_decoder_blocks(bmodel) == 2
    ids = _prompt()
    S, n, T0 = 3, 8, ids.shape[1]
    out = {}
    for mode in ("static_cache", "graph"):
        bf.manual_seed(SEED)
        before = dict(ops.BLOCK_CALLS)
        with torch.no_grad():
            out[mode] = sample_generate(bmodel, ids, samples=S, max_new_tokens=n, keep_weights=True, **{mode: True})
        moved = {k: ops.BLOCK_CALLS[k] - before[k] for k in before}
        if mode == "static_cache":  # eager: the prefill and every one of the n - 1 decode steps
            assert moved == {"rmsnorm": 5 * n, "rope": 2 * n, "swiglu": 2 * n}, moved
        else:  # enqueued under capture (and its warm-up), replayed after that
            assert moved["rope"] >= 2 * 2 and moved["swiglu"] >= 2 * 2 and moved["rmsnorm"] >= 5 * 2, moved
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
def test_recorded_gradients_run_the_plain_forwards(golden_dir):
    """decoder_train's training step on a fused model: with gradients recorded every fast form steps aside, so the loss
    and every gradient are the unfused model's bit for bit, and none of the three kernels is launched."""
    from test_gpu_causal_attention import _decoder, _token_nll

    import bayeformers_amd as bf
    from bayeformers_amd import ops
    from bayeformers_amd.sampling import elbo, sample_bayesian

    results = []
    for blocks in (False, True):
        g, bmodel, inputs, ids, mask = _decoder(golden_dir, "decoder_train", "bf16")
        assert bf.fuse_attention(bmodel)
        if blocks:
            assert bf.fuse_decoder_blocks(bmodel) == int(g["config"][3])
        before = dict(ops.BLOCK_CALLS)
        bf.manual_seed(SEED)
        raw, mean, lp, lq = sample_bayesian(bmodel, inputs, int(g["config"][8]))
        loss = elbo(lp, lq, _token_nll(mean[0].float(), ids, mask).double(), int(g["n_batches"]))
        loss.backward()
        assert ops.BLOCK_CALLS == before
        results.append((loss.detach().clone(), {n: p.grad.clone() for n, p in bmodel.named_parameters() if p.grad is not None}))
    (loss0, grads0), (loss1, grads1) = results
    assert torch.equal(loss0, loss1) and grads0.keys() == grads1.keys() and len(grads0) > 0
    assert all(torch.equal(grads0[n], grads1[n]) for n in grads0)


def test_hooks_still_fire_and_hooked_modules_keep_their_forward():
    from test_gpu_generate import _llama, _prompt

    import bayeformers_amd as bf
    from bayeformers_amd import ops

    bmodel = _llama(torch.bfloat16)
    bmodel.graph_replay = False  # (a forward replayed from a HIP graph runs no Python: every call below is an eager one)
    assert bf.fuse_decoder_blocks(bmodel) == 2
    layer = bmodel.model.model.layers[1]
    seen = []
    handle = layer.mlp.register_forward_hook(lambda m, a, o: seen.append((a[0].shape, o.shape)))
    ids = _prompt()
    for i in range(3):
        before = dict(ops.BLOCK_CALLS)
        bf.manual_seed(SEED)
        with torch.no_grad():
            out = bmodel(input_ids=ids, use_cache=False).logits
        assert len(seen) == i + 1 and seen[-1][0] == seen[-1][1] == (2, 128, 512)
        assert {k: ops.BLOCK_CALLS[k] - before[k] for k in before} == {"rmsnorm": 5, "rope": 2, "swiglu": 2}
    handle.remove()
    # a hook on a module whose forward the fast form skips: that module runs, the rest stays fused
    hits = []
    h2 = layer.mlp.act_fn.register_forward_hook(lambda m, a, o: hits.append(1))
    h3 = layer.post_attention_layernorm.register_forward_hook(lambda m, a, o: hits.append(2))
    before = dict(ops.BLOCK_CALLS)
    bf.manual_seed(SEED)
    with torch.no_grad():
        hooked = bmodel(input_ids=ids, use_cache=False).logits
    assert sorted(hits) == [1, 2]
    # layer 1 ran its own forward (its input norm and the final norm are still the kernel's), its MLP its own activation
    assert {k: ops.BLOCK_CALLS[k] - before[k] for k in before} == {"rmsnorm": 4, "rope": 2, "swiglu": 1}
    h2.remove(), h3.remove()
    assert torch.isfinite(out).all() and torch.isfinite(hooked).all()


def test_mistral_sliding_window_still_runs_the_window_kernels():
    """A Mistral config with a sliding window on fused blocks: the attention forward keeps the `sliding_window=` argument,
    so the window entries run as before, on q and k rotated by the kernel."""
    from test_gpu_sliding_window import _decoder, _prompt

    import bayeformers_amd as bf
    from bayeformers_amd import ops
    from bayeformers_amd.sampling import sample_bayesian

    ids, mask = _prompt(pad=37, side="right")
    S, outs = 2, {}
    for name, dtype, fuse in (("ref", torch.float32, False), ("sdpa16", torch.bfloat16, False), ("fused", torch.bfloat16, True)):
        model = _decoder("mistral", dtype, fuse)
        if fuse:
            assert bf.fuse_decoder_blocks(model) == 2
        c0, b0 = dict(ops.GQA_CALLS), dict(ops.BLOCK_CALLS)
        bf.manual_seed(SEED)
        with torch.no_grad():
            raw, _, _, _ = sample_bayesian(model, {"input_ids": ids, "attention_mask": mask, "use_cache": False}, S)
        outs[name] = raw[0].float().view(S, *ids.shape, -1)
        if fuse:
            assert ops.GQA_CALLS["fwd_window"] - c0["fwd_window"] == 2 and ops.GQA_CALLS["fwd"] == c0["fwd"]
            assert {k: ops.BLOCK_CALLS[k] - b0[k] for k in b0} == {"rmsnorm": 5, "rope": 2, "swiglu": 2}
    valid = mask.bool()[None, :, :, None].expand_as(outs["ref"])
    ref = outs["ref"][valid]
    e16 = (outs["sdpa16"][valid] - ref).abs().max().item() / ref.abs().max().item()
    ef = (outs["fused"][valid] - ref).abs().max().item() / ref.abs().max().item()
    print(f"[mistral] fused blocks bf16 {ef:.3e}, framework bf16 {e16:.3e} (max |logit - fp32| / max |fp32|)")
    assert ef <= 2 * e16 + 2e-3  # test_sliding_decoder_logits_match_sdpa's criterion
