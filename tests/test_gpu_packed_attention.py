"""Banded causal attention on the HIP kernels (bf_attention_fwd_gqa_band / bf_attention_bwd_gqa_band) against a float64
restatement of the contract — key j visible to query i iff lo[i] <= j <= i — the bitwise identities with the plain and
the window entries, no leakage between documents, and packed Llama / Mistral decoders routed through fuse_attention."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

LN2 = math.log(2.0)
SEED = 0x5EED
# tests/test_gpu_causal_attention.py's bounds (relative to max |reference|): the same arithmetic over fewer keys
TOL = {torch.bfloat16: {"out": 6.3e-3, "dq": 1.5e-2, "dk": 1.1e-2, "dv": 8e-3},
       torch.float16: {"out": 8e-4, "dq": 1.4e-3, "dk": 1.4e-3, "dv": 1.1e-3}}


def doc_ids(T):
    """[2, T]: row 0 with document boundaries at 1, 17, 128, 129 and 255, row 1 one long document and five of length 1."""
    ids = torch.zeros(2, T, dtype=torch.long)
    for s in (1, 17, 128, 129, 255):
        ids[0, s:] += 1
    for s in range(T - 5, T):
        ids[1, s:] += 1
    return ids.cuda()


def reference(q, k, v, lo, scale, go=None):
    """float64 of the contract: out [B, T, H, D], lse (log2 units) and, given go, (dq, dk, dv) with dk / dv summed over
    each group.  q [B, H, T, D], k / v [B, Hkv, T, D], lo [B, T]."""
    B, H, T, D = q.shape
    Hkv = k.shape[1]
    G = H // Hkv
    q64, k64, v64 = q.double(), k.double().repeat_interleave(G, 1), v.double().repeat_interleave(G, 1)
    s = q64 @ k64.transpose(-1, -2) * scale
    i = torch.arange(T, device=q.device)[:, None]
    j = torch.arange(T, device=q.device)[None, :]
    seen = (j <= i)[None] & (j[None] >= lo.long()[:, :, None])  # [B, T, T]
    s = s.masked_fill(~seen[:, None], float("-inf"))
    m = s.amax(-1, keepdim=True)  # (every row sees itself: finite)
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    p = e / l
    out = p @ v64
    res = [out.transpose(1, 2), ((m + torch.log(l)) / LN2)[..., 0]]
    if go is not None:
        g = go.double().transpose(1, 2)
        dp = g @ v64.transpose(-1, -2)
        ds = p * (dp - (g * out).sum(-1, keepdim=True))
        res += [(scale * ds @ k64).transpose(1, 2),
                (scale * ds.transpose(-1, -2) @ q64).view(B, Hkv, G, T, D).sum(2).transpose(1, 2),
                (p.transpose(-1, -2) @ g).view(B, Hkv, G, T, D).sum(2).transpose(1, 2)]
    return res


def rel_err(a, r, floor=1e-30):
    """max |a - r| / max |r|; `floor` bounds the denominator from below where the reference is exactly zero"""
    return (a.double() - r).abs().max().item() / max(r.abs().max().item(), floor)


def inputs(dtype, B, T, H, Hkv, D, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, T, H * D, generator=g).to("cuda", dtype).view(B, T, H, D).transpose(1, 2)  # strided, as the
    k, v = (torch.randn(B, T, Hkv * D, generator=g).to("cuda", dtype).view(B, T, Hkv, D).transpose(1, 2)  # projections
            for _ in range(2))                                                                          # hand them over
    go = torch.randn(B, T, H, D, generator=g).to("cuda", dtype)
    return q, k, v, go


CASES = [(torch.bfloat16, D, H, Hkv, T) for T in (384, 300) for D, H, Hkv in ((64, 8, 2), (128, 4, 4), (256, 4, 1))]
CASES += [(torch.float16, 128, 4, 4, 300)]


@pytest.mark.parametrize("W", [None, 37, 130])
@pytest.mark.parametrize("dtype,D,H,Hkv,T", CASES, ids=lambda c: str(c)[6:] if isinstance(c, torch.dtype) else str(c))
def test_band_gqa_matches_float64(dtype, D, H, Hkv, T, W):
    from bayeformers_amd import ops

    B = 2
    q, k, v, go = inputs(dtype, B, T, H, Hkv, D, seed=(W or 0) * 7 + D + H + T)
    lo, hi = ops.band_bounds(doc_ids(T), W)
    scale = D ** -0.5
    c0, g0 = dict(ops.PACKED_CALLS), dict(ops.GQA_CALLS)
    qr, kr, vr = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    out = ops.AttentionGqaBandFn.apply(qr, kr, vr, lo, hi, scale)
    out.backward(go)
    assert ops.PACKED_CALLS["fwd"] - c0["fwd"] == 1 and ops.PACKED_CALLS["bwd"] - c0["bwd"] == 1
    assert ops.GQA_CALLS == g0
    out2, lse = ops.attention_forward_gqa_band(q, k, v, lo, scale, want_lse=True)
    assert torch.equal(out, out2) and torch.equal(out, ops.attention_forward_gqa_band(q, k, v, lo, scale))
    r_out, r_lse, r_dq, r_dk, r_dv = reference(q, k, v, lo, scale, go)
    dq, dk, dv = qr.grad.transpose(1, 2), kr.grad.transpose(1, 2), vr.grad.transpose(1, 2)
    for t in (out, lse, dq, dk, dv):
        assert torch.isfinite(t).all()
    lse_err = (lse.double() - r_lse).abs().max().item()
    floor = 1e-3 * go.abs().max().item()  # a gradient's noise floor, for the exactly-zero dq / dk of length-1 documents
    errs = {"out": rel_err(out, r_out), "dq": rel_err(dq, r_dq, floor), "dk": rel_err(dk, r_dk, floor),
            "dv": rel_err(dv, r_dv, floor)}
    print(f"band gqa {str(dtype)[6:]} D={D} H={H} Hkv={Hkv} T={T} W={W}: lse={lse_err:.2e} "
          + " ".join(f"{n}={e:.2e}" for n, e in errs.items()))
    assert lse_err < 2e-2
    for n, e in errs.items():
        assert e <= TOL[dtype][n], (n, e)
    # a document of one token sees itself only: P = 1, and its output is its value row (its dq and dk are dS = P (dP - delta)
    # = 0 in the reference, and fp32 rounding of dP - delta on the kernels: the floor above)
    alone = (lo.long() == torch.arange(T, device="cuda")) & (hi.long() == torch.arange(T, device="cuda"))
    assert alone[0, 0] and alone[1, T - 1]
    G = H // Hkv
    assert torch.equal(out[alone], v.transpose(1, 2)[alone].repeat_interleave(G, 1))


def _all(fwd, bwd, q, k, v, go):
    out, lse = fwd(q, k, v)
    return (out, lse) + tuple(bwd(q, k, v, out, go, lse))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("D,H,Hkv", [(64, 8, 2), (128, 4, 1), (256, 4, 2)])
@pytest.mark.parametrize("T", [256, 300])
def test_one_document_is_bitwise_the_causal_and_the_window_entries(dtype, D, H, Hkv, T):
    from bayeformers_amd import ops

    B, scale = 2, D ** -0.5
    q, k, v, go = inputs(dtype, B, T, H, Hkv, D, seed=D + H)
    one = torch.zeros(B, T, dtype=torch.long, device="cuda")
    for W in (None, 1, 100, 129):
        lo, hi = ops.band_bounds(one, W)
        band = _all(lambda q, k, v: ops.attention_forward_gqa_band(q, k, v, lo, scale, want_lse=True),
                    lambda q, k, v, out, go, lse: ops.attention_backward_gqa_band(q, k, v, lo, hi, out, go, lse, scale),
                    q, k, v, go)
        plain = _all(lambda q, k, v: ops.attention_forward_gqa(q, k, v, None, scale, True, None, want_lse=True, window=W),
                     lambda q, k, v, out, go, lse: ops.attention_backward_gqa(q, k, v, None, None, out, go, lse, scale,
                                                                              True, window=W),
                     q, k, v, go)
        for name, a, b in zip(("out", "lse", "dq", "dk", "dv"), band, plain):
            assert torch.equal(a, b), (W, name)


@pytest.mark.parametrize("D,H,Hkv", [(64, 8, 2), (128, 4, 4), (256, 4, 1)])
@pytest.mark.parametrize("T,W", [(384, None), (300, 130)])
def test_nothing_leaks_between_documents(D, H, Hkv, T, W):
    from bayeformers_amd import ops

    B, scale, dtype = 2, D ** -0.5, torch.bfloat16
    q, k, v, go = inputs(dtype, B, T, H, Hkv, D, seed=T + D)
    ids = doc_ids(T)
    lo, hi = ops.band_bounds(ids, W)
    inside = torch.stack([ids[0] == 2, ids[1] == 0])  # row 0: the document 17 .. 127; row 1: the long one
    out0, lse0 = ops.attention_forward_gqa_band(q, k, v, lo, scale, want_lse=True)
    k3, v3 = (torch.where(inside[:, None, :, None], 3 * t, t) for t in (k, v))
    go0 = go.masked_fill(inside[:, :, None, None], 0)
    out1, lse1 = ops.attention_forward_gqa_band(q, k3, v3, lo, scale, want_lse=True)
    dq, dk, dv = ops.attention_backward_gqa_band(q, k3, v3, lo, hi, out1, go0, lse1, scale)
    assert torch.equal(out0[~inside], out1[~inside])
    assert torch.equal(lse0.transpose(1, 2)[~inside], lse1.transpose(1, 2)[~inside])
    assert not torch.equal(out0[inside], out1[inside])
    for t in (dq, dk, dv):
        assert torch.isfinite(t).all() and (t[inside] == 0).all()
    assert dk[~inside].abs().max() > 0 and dv[~inside].abs().max() > 0


# ---------------------------------------------------------------------------------------------------- models
FAMILIES = {"llama": {}, "mistral": dict(sliding_window=100)}
DOCS = (100, 28, 128)


def _decoder(kind, dtype, fuse=True):
    from transformers import AutoConfig, AutoModelForCausalLM

    import bayeformers_amd as bf

    cfg = AutoConfig.for_model(kind, hidden_size=256, num_attention_heads=4, num_key_value_heads=2, head_dim=64,
                               num_hidden_layers=2, intermediate_size=512, vocab_size=512, max_position_embeddings=1024,
                               tie_word_embeddings=False, attention_dropout=0.0, attn_implementation="sdpa",
                               **FAMILIES[kind])
    torch.manual_seed(0)
    bmodel = bf.to_bayesian(AutoModelForCausalLM.from_config(cfg).eval(), delta=0.05, freeze=True).eval().cuda()
    if dtype != torch.float32:
        freqs = {n: b.detach().clone() for n, b in bmodel.named_buffers() if "inv_freq" in n}
        bmodel = bmodel.to(dtype)
        for n, b in freqs.items():
            setattr(bmodel.get_submodule(n.rsplit(".", 1)[0]), n.rsplit(".", 1)[1], b)
    if fuse:
        assert bf.fuse_attention(bmodel)
    return bmodel


@pytest.mark.parametrize("kind", list(FAMILIES))
def test_packed_decoder_logits_and_gradients_match_sdpa(kind):
    """T 256 packed as documents of 100, 28 and 128 tokens (position ids that restart, no attention mask).  The fused bf16
    model against the same Bayesian model on the framework's attention in fp32: the logits' error and, per parameter, the
    error of one Monte-Carlo training step's gradients are held to twice the bf16 framework model's own (plus 2e-3 /
    1e-2); every layer ran the band kernels once per direction; and the last document's logits are those of a run of that
    document alone."""
    import bayeformers_amd as bf
    from bayeformers_amd import ops
    from bayeformers_amd.sampling import sample_bayesian

    B, T, S = 2, sum(DOCS), 2
    ids = torch.randint(0, 512, (B, T), generator=torch.Generator().manual_seed(11)).cuda()
    pos = torch.cat([torch.arange(n) for n in DOCS])[None].expand(B, T).contiguous().cuda()
    logits, grads = {}, {}
    for name, dtype, fuse in (("ref", torch.float32, False), ("sdpa16", torch.bfloat16, False),
                              ("fused", torch.bfloat16, True)):
        model = _decoder(kind, dtype, fuse)
        for p in model.parameters():
            p.requires_grad_(p.dtype.is_floating_point)
        c0, g0 = dict(ops.PACKED_CALLS), dict(ops.GQA_CALLS)
        bf.manual_seed(SEED)
        raw, mean, _, _ = sample_bayesian(model, {"input_ids": ids, "position_ids": pos, "use_cache": False}, S)
        logits[name] = raw[0].detach().float().view(S, B, T, -1)
        loss = torch.nn.functional.cross_entropy(mean[0].float()[:, :-1].reshape(-1, 512), ids[:, 1:].reshape(-1))
        loss.backward()
        grads[name] = {n: p.grad.double().clone() for n, p in model.named_parameters() if p.grad is not None}
        if fuse:
            assert ops.PACKED_CALLS["fwd"] - c0["fwd"] == 2 and ops.PACKED_CALLS["bwd"] - c0["bwd"] == 2
            assert ops.GQA_CALLS == g0
            first = T - DOCS[-1]
            bf.manual_seed(SEED)
            with torch.no_grad():
                alone, _, _, _ = sample_bayesian(model, {"input_ids": ids[:, first:].contiguous(), "use_cache": False}, S)
            assert ops.PACKED_CALLS["fwd"] - c0["fwd"] == 2  # (one document, no position ids: the plain entries)
            logits["alone"] = alone[0].float().view(S, B, DOCS[-1], -1)
        else:
            assert ops.PACKED_CALLS == c0
    ref = logits["ref"]
    e16 = (logits["sdpa16"] - ref).abs().max().item() / ref.abs().max().item()
    ef = (logits["fused"] - ref).abs().max().item() / ref.abs().max().item()
    ea = (logits["alone"] - ref[:, :, T - DOCS[-1]:]).abs().max().item() / ref.abs().max().item()
    print(f"[{kind}] packed: fused bf16 {ef:.3e}, framework bf16 {e16:.3e}, last document alone {ea:.3e} "
          f"(max |logit - fp32| / max |fp32|)")
    assert ef <= 2 * e16 + 2e-3
    assert ea <= 2 * e16 + 2e-3
    assert grads["fused"].keys() == grads["ref"].keys() and grads["ref"]
    worst = 0.0
    for n, g in grads["ref"].items():
        scale = max(g.norm().item(), 1e-30)
        g16 = (grads["sdpa16"][n] - g).norm().item() / scale
        gf = (grads["fused"][n] - g).norm().item() / scale
        worst = max(worst, gf - 2 * g16)
        assert gf <= 2 * g16 + 1e-2, (n, gf, g16)
    print(f"[{kind}] packed gradients: max(fused - 2 x framework bf16) = {worst:.3e}")
