"""Causal, grouped-query attention (bf_attention_fwd_gqa / bf_attention_bwd_gqa) against a float64 restatement, and the
decoder-only models routed through fuse_attention."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LN2 = math.log(2.0)


def reference(q, k, v, key_mask, scale, causal, go=None):
    """float64 out [B, T, H, D], lse in log2 units [B, H, T] (+inf for a row with no visible key) and, given the output
    gradient go [B, T, H, D], (dq [B, T, H, D], dk / dv [B, T, Hkv, D] summed over each group)."""
    B, H, T, D = q.shape
    Hkv = k.shape[1]
    G = H // Hkv
    q64 = q.double()
    k64 = k.double().repeat_interleave(G, dim=1)
    v64 = v.double().repeat_interleave(G, dim=1)
    s = q64 @ k64.transpose(-1, -2) * scale
    if key_mask is not None:
        s = s + key_mask.double()[:, None, None, :]
    if causal:
        s = s.masked_fill(torch.ones(T, T, dtype=torch.bool, device=q.device).triu(1), float("-inf"))
    m = s.amax(-1, keepdim=True)
    valid = torch.isfinite(m)
    m = torch.where(valid, m, torch.zeros_like(m))
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    p = torch.where(valid, e / torch.where(valid, l, torch.ones_like(l)), torch.zeros_like(e))
    out = p @ v64
    lse = torch.where(valid, (m + torch.log(torch.where(valid, l, torch.ones_like(l)))) / LN2,
                      torch.full_like(m, float("inf")))[..., 0]
    res = [out.transpose(1, 2), lse]
    if go is not None:
        g = go.double().transpose(1, 2)  # [B, H, T, D]
        dp = g @ v64.transpose(-1, -2)
        delta = (g * out).sum(-1, keepdim=True)
        ds = p * (dp - delta)
        dq = scale * ds @ k64
        dk = (scale * ds.transpose(-1, -2) @ q64).view(B, Hkv, G, T, D).sum(2)
        dv = (p.transpose(-1, -2) @ g).view(B, Hkv, G, T, D).sum(2)
        res += [dq.transpose(1, 2), dk.transpose(1, 2), dv.transpose(1, 2)]
    return res


def make_inputs(dtype, B, T, H, Hkv, D, layout, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, T, H * D, generator=g).to("cuda", dtype).view(B, T, H, D).transpose(1, 2)
    if layout == "view":  # the projections' [B, T, Hkv*D] outputs, as the HF decoder hands them over after RoPE
        k, v = (torch.randn(B, T, Hkv * D, generator=g).to("cuda", dtype).view(B, T, Hkv, D).transpose(1, 2) for _ in range(2))
    else:  # K / V as a cache returns them: contiguous [B, Hkv, T, D]
        k, v = (torch.randn(B, Hkv, T, D, generator=g).to("cuda", dtype) for _ in range(2))
    return q, k, v


def make_mask(kind, B, T):
    """row 0 full; row 1 right-padded (kind "right") or left-padded past the first key tile (kind "left": the causal
    rows of the padding have no visible key)."""
    if kind == "none":
        return None, None, None
    keep = torch.ones(B, T, dtype=torch.bool)
    pad = min(T - 8, T // 3 + 17)
    if kind == "right":
        keep[1, T - pad:] = False
    else:
        keep[1, :pad] = False
    m = torch.zeros(B, T).masked_fill_(~keep, float("-inf")).cuda()
    return m, torch.zeros(1, dtype=torch.bool, device="cuda"), keep


def rel_err(a, r):
    return (a.double() - r).abs().max().item() / max(r.abs().max().item(), 1e-30)


# relative to max |reference|; measured on the MI355X and set to 2x the largest measured value per (dtype, quantity)
# (largest over the grid below: bf16 out 3.1e-3, dq 7.2e-3, dk 5.2e-3, dv 3.9e-3; fp16 3.9e-4, 6.7e-4, 6.9e-4, 5.3e-4)
TOL = {torch.bfloat16: {"out": 6.3e-3, "dq": 1.5e-2, "dk": 1.1e-2, "dv": 8e-3},
       torch.float16: {"out": 8e-4, "dq": 1.4e-3, "dk": 1.4e-3, "dv": 1.1e-3}}


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("H,Hkv", [(8, 8), (8, 2), (4, 1)])
@pytest.mark.parametrize("T", [128, 384, 1024])
@pytest.mark.parametrize("mask", ["none", "right", "left"])
@pytest.mark.parametrize("layout", ["view", "cache"])
def test_causal_gqa_matches_float64(dtype, D, H, Hkv, T, mask, layout):
    from bayeformers_amd import ops

    B = 2
    q, k, v = make_inputs(dtype, B, T, H, Hkv, D, layout, seed=T * 31 + H * 7 + Hkv + D)
    assert ops.attention_supported(q, k, v, causal=True, kv_heads=Hkv)
    mk = make_mask(mask, B, T)
    key_mask, mask_off = mk[0], mk[1]
    scale = D ** -0.5
    g = torch.Generator().manual_seed(T + D)
    go = torch.randn(B, T, H, D, generator=g).to("cuda", dtype)
    qr, kr, vr = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    out = ops.AttentionGqaFn.apply(qr, kr, vr, key_mask, mask_off, scale, True)
    out.backward(go)
    out2, lse = ops.attention_forward_gqa(q, k, v, key_mask, scale, True, mask_off, want_lse=True)
    assert torch.equal(out, out2)
    r_out, r_lse, r_dq, r_dk, r_dv = reference(q, k, v, key_mask, scale, True, go)
    dq, dk, dv = qr.grad.transpose(1, 2), kr.grad.transpose(1, 2), vr.grad.transpose(1, 2)
    for t in (out, lse, dq, dk, dv):
        assert t.isnan().sum().item() == 0
    for t in (out, dq, dk, dv):
        assert torch.isfinite(t).all()
    fin = torch.isfinite(r_lse)
    assert torch.equal(torch.isfinite(lse), fin)
    assert (lse[fin].double() - r_lse[fin]).abs().max().item() < 2e-2
    errs = {"out": rel_err(out, r_out), "dq": rel_err(dq, r_dq), "dk": rel_err(dk, r_dk), "dv": rel_err(dv, r_dv)}
    print(f"causal gqa {str(dtype)[6:]} D={D} H={H} Hkv={Hkv} T={T} mask={mask} layout={layout}: "
          + " ".join(f"{n}={e:.2e}" for n, e in errs.items()))
    for n, e in errs.items():
        assert e <= TOL[dtype][n], (n, e)
    if mask == "left":  # rows of the padding that see no key at all: exactly 0, gradients 0
        dead = ~mk[2][1].cuda() & (torch.arange(T, device="cuda") < (~mk[2][1]).sum().item())
        assert dead.any()
        assert (out[1][dead] == 0).all() and (dq[1][dead] == 0).all()
        assert (dk[1][dead] == 0).all() and (dv[1][dead] == 0).all()  # padded keys: seen by no query
        assert (~torch.isfinite(lse[1][:, dead])).all()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("D,H,Hkv", [(64, 8, 2), (128, 4, 4), (128, 4, 1)])
def test_non_causal_gqa_matches_float64(dtype, D, H, Hkv):
    """The new kernels without the causal mask (grouped K/V or head size 128, which the BERT kernels do not take)."""
    from bayeformers_amd import ops

    B, T = 2, 384
    q, k, v = make_inputs(dtype, B, T, H, Hkv, D, "cache", seed=5 + D + Hkv)
    key_mask, mask_off, _ = make_mask("right", B, T)
    scale = D ** -0.5
    go = torch.randn(B, T, H, D, generator=torch.Generator().manual_seed(3)).to("cuda", dtype)
    qr, kr, vr = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    out = ops.AttentionGqaFn.apply(qr, kr, vr, key_mask, mask_off, scale, False)
    out.backward(go)
    r_out, _, r_dq, r_dk, r_dv = reference(q, k, v, key_mask, scale, False, go)
    errs = {"out": rel_err(out, r_out), "dq": rel_err(qr.grad.transpose(1, 2), r_dq),
            "dk": rel_err(kr.grad.transpose(1, 2), r_dk), "dv": rel_err(vr.grad.transpose(1, 2), r_dv)}
    print(f"non-causal gqa {str(dtype)[6:]} D={D} H={H} Hkv={Hkv}: " + " ".join(f"{n}={e:.2e}" for n, e in errs.items()))
    for n, e in errs.items():
        assert e <= TOL[dtype][n], (n, e)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("T", [128, 384])
@pytest.mark.parametrize("masked", [False, True])
def test_gqa_entry_non_causal_group1_d64_is_the_bert_kernel_bitwise(dtype, T, masked):
    """bf_attention_fwd_gqa / bf_attention_bwd_gqa with causal = 0, one K/V head per query head and head size 64 on the
    packed [B, T, H*64] projections give the bits of bf_attention_fwd / bf_attention_bwd."""
    from bayeformers_amd import ops

    B, H = 3, 4
    q, k, v = make_inputs(dtype, B, T, H, H, 64, "view", seed=T + masked)
    key_mask, mask_off = (make_mask("right", B, T)[:2]) if masked else (None, None)
    go = torch.randn(B, T, H, 64, generator=torch.Generator().manual_seed(1)).to("cuda", dtype)
    a, la = ops.attention_forward_gqa(q, k, v, key_mask, 0.125, False, mask_off, want_lse=True)
    b, lb = ops.attention_forward(q, k, v, key_mask, 0.125, mask_off, want_lse=True)
    assert torch.equal(a, b) and torch.equal(la, lb)
    ga = ops.attention_backward_gqa(q, k, v, key_mask, mask_off, a, go, la, 0.125, False)
    gb = ops.attention_backward(q, k, v, key_mask, mask_off, b, go, lb, 0.125)
    for x, y in zip(ga, gb):
        assert torch.equal(x, y)


def test_gqa_entry_refuses_what_it_cannot_run():
    from bayeformers_amd import _C, ops

    q, k, v = make_inputs(torch.bfloat16, 1, 128, 6, 4, 64, "view", seed=0)
    assert not ops.attention_supported(q, k, v, causal=True)  # 4 K/V heads do not divide 6 query heads
    shape = ops._gqa_shape(q, k, v, True)
    out = torch.empty(1, 128, 6, 64, dtype=torch.bfloat16, device="cuda")
    rc = _C.lib().bf_attention_fwd_gqa(q.data_ptr(), k.data_ptr(), v.data_ptr(), None, None, out.data_ptr(), None,
                                       _C.BF_DT_BF16, ctypes_ref(shape), 0.125, None)
    assert rc != 0 and b"divide" in _C.lib().bf_last_error()
    shape = ops._gqa_shape(q[:, :4], k[:, :2], v[:, :2], True)
    shape.head_dim = 96
    rc = _C.lib().bf_attention_fwd_gqa(q.data_ptr(), k.data_ptr(), v.data_ptr(), None, None, out.data_ptr(), None,
                                       _C.BF_DT_BF16, ctypes_ref(shape), 0.125, None)
    assert rc != 0 and b"head size" in _C.lib().bf_last_error()


def ctypes_ref(s):
    import ctypes

    return ctypes.byref(s)


# ---------------------------------------------------------------------------------------------------- decoder-only models
# tests/golden/make_golden_decoder.py: HF LlamaForCausalLM converted by the REAL reference, Philox epsilon injected.

def _decoder(golden_dir, name, dtype):
    """(fixture, converted model on the GPU, inputs, ids, mask) for one fixture; bf16 keeps RoPE's inverse frequencies in
    fp32 (Module.to would round them to bf16 and move every position away from the reference's)."""
    from transformers import LlamaConfig, LlamaForCausalLM

    import bayeformers_amd as bf

    g = np.load(f"{golden_dir}/{name}.npz")
    hidden, heads, kv_heads, layers, ffn, vocab, T, B = (int(x) for x in g["config"][:8])
    cfg = LlamaConfig(hidden_size=hidden, num_attention_heads=heads, num_key_value_heads=kv_heads, num_hidden_layers=layers,
                      intermediate_size=ffn, vocab_size=vocab, max_position_embeddings=T, tie_word_embeddings=False,
                      use_cache=False, attention_dropout=0.0, attn_implementation="sdpa")
    torch.manual_seed(int(g["model_seed"]))
    model = LlamaForCausalLM(cfg).eval()
    bmodel = bf.to_bayesian(model, delta=float(g["delta"]), freeze=True).eval()
    assert float(sum(p.detach().double().abs().sum() for p in bmodel.parameters())) == pytest.approx(float(g["checksum"]), rel=1e-6)
    torch.manual_seed(int(g["input_seed"]))
    ids = torch.randint(0, vocab, (B, T))
    assert int(ids.sum()) == int(g["ids_sum"])
    mask = torch.from_numpy(g["mask"])
    bmodel = bmodel.cuda()
    if dtype == "bf16":
        freqs = {n: b.detach().clone() for n, b in bmodel.named_buffers() if "inv_freq" in n}
        bmodel = bmodel.to(torch.bfloat16)
        for n, b in freqs.items():
            mod, attr = bmodel.get_submodule(n.rsplit(".", 1)[0]), n.rsplit(".", 1)[1]
            setattr(mod, attr, b)
    return g, bmodel, {"input_ids": ids.cuda(), "attention_mask": mask.cuda(), "use_cache": False}, ids.cuda(), mask.cuda()


def _token_nll(logits, ids, mask):
    valid = (mask[:, :-1] * mask[:, 1:]).bool()
    labels = ids[:, 1:].masked_fill(~valid, -100)
    return torch.nn.functional.cross_entropy(logits[:, :-1].reshape(-1, logits.shape[-1]).double(), labels.reshape(-1),
                                             ignore_index=-100)


def _logits_and_last_hidden(out):
    return out.logits, out.hidden_states[-1]


# (fixture, dtype, max |logit - ref| / max |ref|, max |hidden - ref| / max |ref|, |token NLL - ref|): 2x the values measured
# on the MI355X (profiles/causal_attention_tests.txt)
DECODER_CASES = [
    ("decoder_mha64", "fp32", 1.5e-6, 1.6e-6, 5e-8), ("decoder_mha64", "bf16", 1.3e-2, 1e-2, 5.1e-4),
    ("decoder_gqa64", "fp32", 3e-6, 3e-6, 1e-7), ("decoder_gqa64", "bf16", 2.5e-2, 3.2e-2, 3e-4),
    ("decoder_mqa128", "fp32", 6e-6, 3e-6, 7e-8), ("decoder_mqa128", "bf16", 2.1e-2, 1.7e-2, 5.6e-4),
]


@pytest.mark.parametrize("name,dtype,tol_logit,tol_hidden,tol_nll", DECODER_CASES)
def test_decoder_matches_reference(golden_dir, name, dtype, tol_logit, tol_hidden, tol_nll):
    """to_bayesian(LlamaForCausalLM) + fuse_attention against the reference's per-sample outputs.  decoder_mha64 (heads =
    kv heads, head size 64, T = 128, no padding) is the shape the bidirectional BERT kernel used to accept: the
    attention must be causal.  fp32 runs the framework's attention (the kernels are 16-bit); bf16 runs the causal
    kernels, and the test asserts they dispatched."""
    import bayeformers_amd as bf
    from bayeformers_amd.sampling import sample_bayesian

    g, bmodel, inputs, ids, mask = _decoder(golden_dir, name, dtype)
    assert bf.fuse_attention(bmodel)
    from bayeformers_amd import ops

    calls = dict(getattr(ops, "GQA_CALLS", {"fwd": 0}))
    S = int(g["config"][8])
    bf.manual_seed(0x5EED)
    bf.set_compute_dtype(dtype)
    try:
        with torch.no_grad():
            raw, mean, lp, lq = sample_bayesian(bmodel, dict(inputs, output_hidden_states=True), S, select=_logits_and_last_hidden)
    finally:
        bf.set_compute_dtype("bf16")
    B, T = ids.shape
    logits = raw[0].float().view(S, B, T, -1)
    hidden = raw[1].float().view(S, B, T, -1)
    pos = [tuple(p) for p in g["positions"].tolist()]
    got_l = torch.stack([logits[:, b, t] for b, t in pos], 1).cpu().numpy()
    got_h = torch.stack([hidden[:, b, t] for b, t in pos], 1).cpu().numpy()
    err_l = float(np.abs(got_l - g["logits"]).max() / np.abs(g["logits"]).max())
    err_h = float(np.abs(got_h - g["hidden"]).max() / np.abs(g["hidden"]).max())
    nll = np.array([float(_token_nll(logits[s], ids, mask)) for s in range(S)])
    err_n = float(np.abs(nll - g["token_nll"]).max())
    print(f"[{name} {dtype}] logits {err_l:.3e}, hidden {err_h:.3e}, token nll {err_n:.3e} (rel. to max |ref|; nll abs)")
    assert np.isfinite(got_l).all() and np.isfinite(got_h).all()
    assert err_l < tol_logit and err_h < tol_hidden and err_n < tol_nll
    lps = bmodel.log_prob_samples().cpu().numpy()
    np.testing.assert_allclose(lps[:, 0], g["log_prior"], rtol=2e-6)
    np.testing.assert_allclose(lps[:, 1], g["lvp"], rtol=2e-6)
    if dtype == "bf16":
        assert ops.GQA_CALLS["fwd"] - calls["fwd"] == int(g["config"][3])  # one causal launch per layer


def test_decoder_training_step_matches_reference(golden_dir):
    """One training step (tests/golden/decoder_train.npz: the sample loop with gradients, loss = (lvp - log_prior) / NB +
    token NLL of the mean logits, backward) in bf16 through the causal kernels, forward and backward."""
    import bayeformers_amd as bf
    from bayeformers_amd import ops
    from bayeformers_amd.sampling import elbo, sample_bayesian

    g, bmodel, inputs, ids, mask = _decoder(golden_dir, "decoder_train", "bf16")
    params = dict(bmodel.named_parameters())
    assert bf.fuse_attention(bmodel)
    calls = dict(ops.GQA_CALLS)
    S, NB = int(g["config"][8]), int(g["n_batches"])
    bf.manual_seed(0x5EED)
    raw, mean, lp, lq = sample_bayesian(bmodel, inputs, S)
    nll = _token_nll(mean[0].float(), ids, mask)
    loss = elbo(lp, lq, nll.double(), NB)
    loss.backward()
    layers = int(g["config"][3])
    assert ops.GQA_CALLS["fwd"] - calls["fwd"] == layers and ops.GQA_CALLS["bwd"] - calls["bwd"] == layers
    print(f"[decoder_train bf16] loss {float(loss.detach()):.6f} vs {float(g['loss']):.6f}, nll {float(nll):.6f} vs {float(g['nll']):.6f}")
    assert float(loss.detach()) == pytest.approx(float(g["loss"]), rel=1e-6)  # measured 5e-8
    names = [str(n) for n in g["names"]]
    assert sorted(names) == sorted(n for n, p in params.items() if p.grad is not None)
    gmax = max(float(g[f"stat/{n}"][2]) for n in names)
    worst = {}
    for n in names:
        got = params[n].grad.detach().double().cpu().numpy()
        assert np.isfinite(got).all(), n
        ref_sum, ref_abs, ref_max = g[f"stat/{n}"]
        if ref_max < 1e-6 * gmax:
            continue
        worst[n] = abs(np.abs(got).sum() - ref_abs) / ref_abs
        if f"grad/{n}" in g.files:
            ref = g[f"grad/{n}"].astype(np.float64)
            worst[n + " (full)"] = np.abs(got - ref).max() / ref_max
    print("[decoder_train bf16] worst gradient errors: " + ", ".join(f"{k}={v:.2e}" for k, v in sorted(worst.items(), key=lambda x: -x[1])[:6]))
    assert sum(k.endswith("(full)") for k in worst) == 2
    # 2x measured: full rho gradients 1.05e-2 (o_proj), sum |g| of any tensor 1.5e-3
    assert all(v <= (2.1e-2 if k.endswith("(full)") else 3e-3) for k, v in worst.items()), worst


# ---------------------------------------------------------------------------------------------------- graph replay, predictive
# A captured step enqueues its launches once, under capture: GQA_CALLS counts them there.  That the replays then run the
# causal kernels is shown by their bits: replay k equals eager step k, which ran them (counted), and differs from the same
# step on the framework's attention.

def _framework_attention(bmodel):
    """context: the model's attention switched back to the framework's SDPA (the control run)."""
    import contextlib

    @contextlib.contextmanager
    def ctx():
        cfgs = [m.config for m in bmodel.modules() if hasattr(getattr(m, "config", None), "_attn_implementation")]
        saved = [c._attn_implementation for c in cfgs]
        for c in cfgs:
            c._attn_implementation = "sdpa"
        try:
            yield
        finally:
            for c, a in zip(cfgs, saved):
                c._attn_implementation = a
    return ctx()


def test_graphed_sampler_replays_are_the_eager_steps_on_a_padded_gqa_decoder(golden_dir):
    """GraphedSampler on decoder_gqa64 (8 heads / 2 kv heads, left- and right-padded rows): replay k == eager step k, bit
    for bit, for logits, log_prior and lvp — the padding mask's key mask and device flag are rebuilt inside the graph."""
    import bayeformers_amd as bf
    from bayeformers_amd import ops
    from bayeformers_amd.sampling import GraphedSampler, sample_bayesian

    g, bmodel, inputs, ids, mask = _decoder(golden_dir, "decoder_gqa64", "bf16")
    assert bf.fuse_attention(bmodel)
    S, layers = 2, int(g["config"][3])
    # a second batch of the same signature: other ids, the padding moved
    ids2 = torch.randint(0, int(g["config"][5]), ids.shape, generator=torch.Generator().manual_seed(9)).cuda()
    mask2 = mask.flip(1).contiguous()
    batches = [inputs, {"input_ids": ids2, "attention_mask": mask2, "use_cache": False}]
    order = [0, 1, 0, 1]
    host = lambda r: (r[0][0].float().cpu().clone(), float(r[2]), float(r[3]))
    bf.set_compute_dtype("bf16")
    bf.manual_seed(0x5EED)
    c0 = ops.GQA_CALLS["fwd"]
    with torch.no_grad():
        eager = [host(sample_bayesian(bmodel, batches[b], S)) for b in order]
        assert ops.GQA_CALLS["fwd"] - c0 == layers * len(order)
        bf.manual_seed(0x5EED)
        with _framework_attention(bmodel):
            control = host(sample_bayesian(bmodel, batches[0], S))
        assert not torch.equal(control[0], eager[0][0])  # the framework's attention gives other bits
        c1 = ops.GQA_CALLS["fwd"]
        sampler = GraphedSampler(bmodel, batches[0], S)  # warm-up steps and the capture run here
        try:
            captured = ops.GQA_CALLS["fwd"] - c1
            bf.manual_seed(0x5EED)
            for k, b in enumerate(order):
                got = host(sampler(batches[b]) if k else sampler())
                assert torch.equal(got[0], eager[k][0]) and got[1:] == eager[k][1:], k
            assert ops.GQA_CALLS["fwd"] - c1 == captured  # the replays enqueue nothing from Python
        finally:
            sampler.close()
    print(f"[graphed sampler decoder_gqa64] {len(order)} replays bitwise equal to the eager steps; causal forward launches "
          f"enqueued by the warm-up steps and the capture: {captured}")
    assert captured >= layers  # the capture (and its warm-up steps) enqueued the causal kernels


def test_graphed_training_step_replay_matches_reference_decoder_train(golden_dir):
    """decoder_train on a GraphedTrainingStep: the replayed step (samples 0 .. S-1, the fixture's) gives the eager step's
    loss and gradients bit for bit, and those match the reference.  lr = 0 keeps the parameters where the fixture has them."""
    import bayeformers_amd as bf
    from bayeformers_amd import ops
    from bayeformers_amd.training import GraphedTrainingStep, training_step

    g, bmodel, inputs, ids, mask = _decoder(golden_dir, "decoder_train", "bf16")
    params = dict(bmodel.named_parameters())
    assert bf.fuse_attention(bmodel)
    S, NB, layers = int(g["config"][8]), int(g["n_batches"]), int(g["config"][3])
    nll = lambda mean: _token_nll(mean[0].float(), ids, mask)
    train = [p for p in bmodel.parameters() if p.requires_grad]
    opt = torch.optim.AdamW(train, lr=torch.tensor(0.0, device="cuda"), weight_decay=0.0, fused=True, capturable=True)
    bf.set_compute_dtype("bf16")
    bf.manual_seed(0x5EED)
    c0 = dict(ops.GQA_CALLS)
    loss_e = float(training_step(bmodel, inputs, S, nll, opt, NB, max_grad_norm=None))
    assert ops.GQA_CALLS["fwd"] - c0["fwd"] == layers and ops.GQA_CALLS["bwd"] - c0["bwd"] == layers
    grads_e = {n: p.grad.detach().clone() for n, p in params.items() if p.grad is not None}
    step = GraphedTrainingStep(bmodel, inputs, S, nll, opt, NB, max_grad_norm=None, eager_steps=1)
    try:
        step()                      # the eager step GraphedTrainingStep starts with
        bf.manual_seed(0x5EED)      # rewinds the device-resident counter: the replay draws samples 0 .. S-1
        c1 = dict(ops.GQA_CALLS)
        loss_g = float(step())      # capture + replay
        assert step.captures == 1
        captured = (ops.GQA_CALLS["fwd"] - c1["fwd"], ops.GQA_CALLS["bwd"] - c1["bwd"])
        grads_g = {n: p.grad.detach().clone() for n, p in params.items() if p.grad is not None}
    finally:
        step.close()
    print(f"[graphed training step decoder_train] loss {loss_g:.6f} (eager {loss_e:.6f}, reference {float(g['loss']):.6f}); "
          f"causal launches enqueued while capturing (fwd, bwd): {captured}")
    assert captured == (layers, layers)
    assert loss_g == loss_e
    assert grads_g.keys() == grads_e.keys()
    for n in grads_e:
        assert torch.equal(grads_g[n], grads_e[n]), n
    assert loss_g == pytest.approx(float(g["loss"]), rel=1e-6)
    for n in ("model.model.layers.0.self_attn.k_proj.weight.rho", "model.model.layers.0.self_attn.o_proj.weight.rho"):
        ref = g[f"grad/{n}"].astype(np.float64)
        err = np.abs(grads_g[n].double().cpu().numpy() - ref).max() / np.abs(ref).max()
        assert err <= 2.1e-2, (n, err)  # the eager test's bound


def test_sample_predictive_on_decoder_token_logits_matches_float64(golden_dir):
    """sample_predictive on decoder_gqa64's next-token logits (shifted labels, ignore_index on padding) against a float64
    restatement computed from sample_bayesian's per-sample logits of the same step."""
    import bayeformers_amd as bf
    from bayeformers_amd import ops
    from bayeformers_amd.sampling import sample_bayesian, sample_predictive

    g, bmodel, inputs, ids, mask = _decoder(golden_dir, "decoder_gqa64", "bf16")
    assert bf.fuse_attention(bmodel)
    S, V = int(g["config"][8]), int(g["config"][5])
    select = lambda o: (o.logits[:, :-1].reshape(-1, V),)
    labels = ids[:, 1:].masked_fill((mask[:, :-1] * mask[:, 1:]) == 0, -100).reshape(-1)
    bf.set_compute_dtype("bf16")
    c0 = ops.GQA_CALLS["fwd"]
    with torch.no_grad():
        bf.manual_seed(0x5EED)
        raw, mean, lp, lq = sample_bayesian(bmodel, inputs, S, select=select)
        bf.manual_seed(0x5EED)
        (p,) = sample_predictive(bmodel, inputs, S, labels=labels, select=select)
    assert ops.GQA_CALLS["fwd"] - c0 == 2 * int(g["config"][3])
    assert torch.equal(p.mean, mean[0]) and float(p.log_prior) == float(lp) and float(p.log_variational_posterior) == float(lq)
    l = raw[0].double().view(S, -1, V)
    lse = torch.logsumexp(l, -1, keepdim=True)
    pr = torch.exp(l - lse)
    probs = pr.mean(0)
    pe = -(probs * probs.log()).sum(-1)
    ee = -(pr * (l - lse)).sum(-1).mean(0)
    valid = labels != -100
    yc = torch.where(valid, labels, torch.zeros_like(labels))
    py = probs.gather(-1, yc[:, None]).squeeze(-1)
    nll = -py.log()[valid].mean()
    counts = ((l.argmax(-1) == yc) & valid).sum(-1)
    errs = {"probs": (p.probs.double() - probs).abs().max().item(),
            "predictive_entropy": (p.predictive_entropy.double() - pe).abs().max().item(),
            "expected_entropy": (p.expected_entropy.double() - ee).abs().max().item(),
            "mutual_information": (p.mutual_information.double() - (pe - ee).clamp_min(0)).abs().max().item(),
            "nll": abs(float(p.nll) - float(nll))}
    print("[predictive decoder_gqa64 tokens] " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert errs["probs"] <= 2e-6
    for k in ("predictive_entropy", "expected_entropy", "mutual_information", "nll"):
        assert errs[k] <= 1e-5 * max(1.0, float(pe.abs().max())), k
    assert torch.equal(p.correct_per_sample.cpu().reshape(-1), counts.cpu())
