"""Sliding-window attention on the HIP kernels (bf_attention_*_window) against a float64 restatement of the contract —
key j visible to query i iff j <= i and i - j < W — the bitwise identity with the plain entries when the window hides
nothing, and the Mistral / Qwen2 / Qwen3 decoders routed through fuse_attention, sample_generate included."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

LN2 = math.log(2.0)
SEED = 0x5EED
# tests/test_gpu_causal_attention.py's bounds (relative to max |reference|)
TOL = {torch.bfloat16: {"out": 6.3e-3, "dq": 1.5e-2, "dk": 1.1e-2, "dv": 8e-3},
       torch.float16: {"out": 8e-4, "dq": 1.4e-3, "dk": 1.4e-3, "dv": 1.1e-3}}
DEC_TOL = {torch.bfloat16: 9.1e-3, torch.float16: 1.2e-3}  # tests/test_gpu_decode_attention.py's


def visible(Tq, Tk, W, device):
    """[Tq, Tk]: query i (index Tk - Tq + i) sees key j iff j <= index and index - j < W."""
    i = (Tk - Tq + torch.arange(Tq, device=device))[:, None]
    j = torch.arange(Tk, device=device)[None, :]
    return (j <= i) & (i - j < W)


def reference(q, k, v, key_mask, scale, W, go=None):
    """float64 of the contract: out [B, Tq, H, D], lse (log2 units, +inf for a row with no visible key) and, given go,
    (dq, dk, dv) with dk / dv summed over each group.  q [B, H, Tq, D], k / v [B, Hkv, Tk, D]."""
    B, H, Tq, D = q.shape
    Hkv, Tk = k.shape[1], k.shape[2]
    G = H // Hkv
    q64, k64, v64 = q.double(), k.double().repeat_interleave(G, 1), v.double().repeat_interleave(G, 1)
    s = q64 @ k64.transpose(-1, -2) * scale
    if key_mask is not None:
        s = s + key_mask.double()[:, None, None, :]
    s = s.masked_fill(~visible(Tq, Tk, W, q.device), float("-inf"))
    m = s.amax(-1, keepdim=True)
    ok = torch.isfinite(m)
    m = torch.where(ok, m, torch.zeros_like(m))
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    p = torch.where(ok, e / torch.where(ok, l, torch.ones_like(l)), torch.zeros_like(e))
    out = p @ v64
    lse = torch.where(ok, (m + torch.log(torch.where(ok, l, torch.ones_like(l)))) / LN2, torch.full_like(m, float("inf")))
    res = [out.transpose(1, 2), lse[..., 0]]
    if go is not None:
        g = go.double().transpose(1, 2)
        dp = g @ v64.transpose(-1, -2)
        ds = p * (dp - (g * out).sum(-1, keepdim=True))
        res += [(scale * ds @ k64).transpose(1, 2),
                (scale * ds.transpose(-1, -2) @ q64).view(B, Hkv, G, Tk, D).sum(2).transpose(1, 2),
                (p.transpose(-1, -2) @ g).view(B, Hkv, G, Tk, D).sum(2).transpose(1, 2)]
    return res


def rel_err(a, r, floor=1e-30):
    """max |a - r| / max |r|; `floor` bounds the denominator from below where the reference is exactly zero (the dq and
    dk of W = 1: a query sees itself only, so dS = P (dP - delta) = 0)."""
    return (a.double() - r).abs().max().item() / max(r.abs().max().item(), floor)


def inputs(dtype, B, T, H, Hkv, D, layout, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, T, H * D, generator=g).to("cuda", dtype).view(B, T, H, D).transpose(1, 2)
    if layout == "view":  # strided, as the projections hand them over
        k, v = (torch.randn(B, T, Hkv * D, generator=g).to("cuda", dtype).view(B, T, Hkv, D).transpose(1, 2)
                for _ in range(2))
    else:
        k, v = (torch.randn(B, Hkv, T, D, generator=g).to("cuda", dtype) for _ in range(2))
    return q, k, v


def left_padding(B, T, pad):
    """row 1 padded: the first `pad` keys (pad > 0) or the last -pad (pad < 0)"""
    keep = torch.ones(B, T, dtype=torch.bool)
    if pad > 0:
        keep[1, :pad] = False
    else:
        keep[1, T + pad:] = False
    return torch.zeros(B, T).masked_fill_(~keep, float("-inf")).cuda(), torch.zeros(1, dtype=torch.bool, device="cuda")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("H,Hkv", [(4, 4), (8, 2)])
@pytest.mark.parametrize("W", [1, 37, 64, 130, 300, 384])
@pytest.mark.parametrize("pad", [0, 150, -100])
@pytest.mark.parametrize("layout", ["view", "cache"])
def test_window_gqa_matches_float64(dtype, D, H, Hkv, W, pad, layout):
    from bayeformers_amd import ops

    B, T = 2, 384
    q, k, v = inputs(dtype, B, T, H, Hkv, D, layout, seed=W * 7 + D + H + pad)
    key_mask, mask_off = left_padding(B, T, pad) if pad else (None, None)
    scale = D ** -0.5
    go = torch.randn(B, T, H, D, generator=torch.Generator().manual_seed(W)).to("cuda", dtype)
    c0 = dict(ops.GQA_CALLS)
    qr, kr, vr = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    out = ops.AttentionGqaFn.apply(qr, kr, vr, key_mask, mask_off, scale, True, W)
    out.backward(go)
    assert ops.GQA_CALLS["fwd_window"] - c0["fwd_window"] == 1 and ops.GQA_CALLS["bwd_window"] - c0["bwd_window"] == 1
    assert ops.GQA_CALLS["fwd"] == c0["fwd"] and ops.GQA_CALLS["bwd"] == c0["bwd"]
    out2, lse = ops.attention_forward_gqa(q, k, v, key_mask, scale, True, mask_off, want_lse=True, window=W)
    assert torch.equal(out, out2)
    r_out, r_lse, r_dq, r_dk, r_dv = reference(q, k, v, key_mask, scale, W, go)
    dq, dk, dv = qr.grad.transpose(1, 2), kr.grad.transpose(1, 2), vr.grad.transpose(1, 2)
    for t in (out, dq, dk, dv):
        assert torch.isfinite(t).all()
    fin = torch.isfinite(r_lse)
    assert torch.equal(torch.isfinite(lse), fin)
    assert (lse[fin].double() - r_lse[fin]).abs().max().item() < 2e-2
    floor = 1e-3 * go.abs().max().item()  # a gradient's noise floor, for the exactly-zero dq / dk of W = 1
    errs = {"out": rel_err(out, r_out), "dq": rel_err(dq, r_dq, floor), "dk": rel_err(dk, r_dk, floor),
            "dv": rel_err(dv, r_dv, floor)}
    print(f"window gqa {str(dtype)[6:]} D={D} H={H} Hkv={Hkv} W={W} pad={pad} {layout}: "
          + " ".join(f"{n}={e:.2e}" for n, e in errs.items()))
    for n, e in errs.items():
        assert e <= TOL[dtype][n], (n, e)
    if pad > 0 and W < pad:  # padding rows whose window holds padding only: exactly 0, lse +inf
        dead = torch.arange(T, device="cuda") < pad
        assert (out[1][dead] == 0).all() and (dq[1][dead] == 0).all() and (~torch.isfinite(lse[1][:, dead])).all()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("D,H,Hkv", [(64, 8, 2), (128, 4, 1)])
@pytest.mark.parametrize("W", [256, 257, 2 ** 31 - 1])
def test_window_at_least_T_is_bitwise_the_causal_entries(dtype, D, H, Hkv, W):
    from bayeformers_amd import ops

    B, T = 2, 256
    q, k, v = inputs(dtype, B, T, H, Hkv, D, "view", seed=D + H)
    key_mask, mask_off = left_padding(B, T, 40)
    go = torch.randn(B, T, H, D, generator=torch.Generator().manual_seed(1)).to("cuda", dtype)
    res = []
    for window in (None, W):
        out, lse = ops.attention_forward_gqa(q, k, v, key_mask, D ** -0.5, True, mask_off, want_lse=True, window=window)
        grads = ops.attention_backward_gqa(q, k, v, key_mask, mask_off, out, go, lse, D ** -0.5, True, window=window)
        res.append((out, lse) + tuple(grads))
    for a, b in zip(*res):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------- decode
def decode_inputs(dtype, N, H, Hkv, Tq, Tk, D, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(N, Tq, H, D, generator=g).to("cuda", dtype).transpose(1, 2)  # strided, as a decoder step hands it
    k, v = (torch.randn(N, Hkv, Tk, D, generator=g).to("cuda", dtype) for _ in range(2))
    return q, k, v


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("D,H,Hkv", [(64, 8, 2), (128, 8, 1), (128, 4, 4)])
@pytest.mark.parametrize("Tq", [1, 5, 16])
@pytest.mark.parametrize("Tk,W", [(40, 7), (1000, 1), (1000, 129), (4100, 1000), (4100, 5000)])
def test_window_decode_matches_float64(dtype, D, H, Hkv, Tq, Tk, W):
    from bayeformers_amd import ops

    N, extra = 2, 77
    q, k, v = decode_inputs(dtype, N, H, Hkv, Tq, Tk, D, seed=Tk + W + Tq)
    keep = torch.ones(N, Tk, dtype=torch.bool)
    keep[1, :Tk // 3] = False
    key_mask = torch.zeros(N, Tk).masked_fill_(~keep, float("-inf")).cuda()
    scale = D ** -0.5
    r = reference(q, k, v, key_mask, scale, W)[0]
    c0 = dict(ops.DECODE_CALLS)
    out = ops.attention_forward_decode(q, k, v, key_mask, scale, window=W)
    # a fixed-capacity cache filled to Tk; the slots past the fill are never read (their values do not matter)
    kc, vc = (torch.cat([t, 100 * torch.randn(N, Hkv, extra, D, device="cuda", dtype=dtype)], 2) for t in (k, v))
    mc = torch.cat([key_mask, torch.zeros(N, extra, device="cuda")], 1)
    out_len = ops.attention_forward_decode_len(q, kc, vc, torch.tensor([Tk], device="cuda"), mc, scale, window=W)
    assert ops.DECODE_CALLS["window"] - c0["window"] == 1 and ops.DECODE_CALLS["len_window"] - c0["len_window"] == 1
    assert ops.DECODE_CALLS["fwd"] == c0["fwd"] and ops.DECODE_CALLS["len"] == c0["len"]
    for got in (out, out_len):
        assert torch.isfinite(got).all()
        assert rel_err(got, r) <= DEC_TOL[dtype], rel_err(got, r)
    print(f"window decode {str(dtype)[6:]} D={D} H={H} Hkv={Hkv} Tq={Tq} Tk={Tk} W={W}: {rel_err(out, r):.2e} "
          f"len {rel_err(out_len, r):.2e}")


@pytest.mark.parametrize("D,H,Hkv,Tq", [(64, 8, 2, 1), (128, 4, 1, 4)])
@pytest.mark.parametrize("Tk", [100, 3000])
def test_window_decode_at_least_L_is_bitwise_the_plain_entries(D, H, Hkv, Tq, Tk):
    from bayeformers_amd import ops

    q, k, v = decode_inputs(torch.bfloat16, 2, H, Hkv, Tq, Tk, D, seed=3)
    key_mask = torch.zeros(2, Tk, device="cuda")
    key_mask[1, :9] = float("-inf")
    L = torch.tensor([Tk - 30], device="cuda")
    for W in (Tk, Tk + 1, 2 ** 31 - 1):
        assert torch.equal(ops.attention_forward_decode(q, k, v, key_mask, 0.1),
                           ops.attention_forward_decode(q, k, v, key_mask, 0.1, window=W))
        assert torch.equal(ops.attention_forward_decode_len(q, k, v, L, key_mask, 0.1),
                           ops.attention_forward_decode_len(q, k, v, L, key_mask, 0.1, window=W))
    # the _len form at W >= L (but W < capacity): the plain _len entry's result too
    assert torch.equal(ops.attention_forward_decode_len(q, k, v, L, key_mask, 0.1),
                       ops.attention_forward_decode_len(q, k, v, L, key_mask, 0.1, window=Tk - 30))


def test_captured_len_window_launch_replays_while_the_fill_crosses_W():
    from bayeformers_amd import ops

    N, H, Hkv, D, cap, W = 2, 8, 2, 128, 2048, 300
    q, k, v = decode_inputs(torch.bfloat16, N, H, Hkv, 1, cap, D, seed=9)
    L = torch.tensor([1], device="cuda")
    ws = torch.empty(max(ops.attention_decode_workspace_bytes(q, k, v), 16), dtype=torch.uint8, device="cuda")
    out = torch.empty(N, 1, H, D, dtype=torch.bfloat16, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        out.copy_(ops.attention_forward_decode_len(q, k, v, L, None, 0.1, workspace=ws, window=W))
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out.copy_(ops.attention_forward_decode_len(q, k, v, L, None, 0.1, workspace=ws, window=W))
    for fill in (1, 64, 299, 300, 301, 700, 1500, 2048):
        L.fill_(fill)
        g.replay()
        eager = ops.attention_forward_decode_len(q, k, v, L, None, 0.1, workspace=ws, window=W)
        assert torch.equal(out, eager), fill
        r = reference(q, k[:, :, :fill], v[:, :, :fill], None, 0.1, W)[0]
        assert rel_err(out, r) <= DEC_TOL[torch.bfloat16]


# ---------------------------------------------------------------------------------------------------- models
FAMILIES = {
    "mistral": dict(sliding_window=100),
    "qwen2": dict(sliding_window=100, use_sliding_window=True, max_window_layers=1,
                  layer_types=["full_attention", "sliding_attention"]),
    "qwen3": dict(sliding_window=100, use_sliding_window=True, max_window_layers=0,
                  layer_types=["sliding_attention", "sliding_attention"]),
}


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


def _sliding_layers(kind):
    return FAMILIES[kind].get("layer_types", ["sliding_attention"] * 2).count("sliding_attention")


def _prompt(B=2, T=256, pad=0, side="left"):
    ids = torch.randint(0, 512, (B, T), generator=torch.Generator().manual_seed(11)).cuda()
    mask = torch.ones_like(ids)
    if side == "left":
        mask[B - 1, :pad] = 0
    else:  # (no query row without a visible key: the framework's reference attention is defined on every row)
        mask[B - 1, T - pad:] = 0
    return ids, mask


@pytest.mark.parametrize("kind", list(FAMILIES))
def test_sliding_decoder_logits_match_sdpa(kind):
    """The fused bf16 model against the same Bayesian model on the framework's attention in fp32: its error is that of
    the bf16 framework model, and every sliding layer ran the window kernel."""
    import bayeformers_amd as bf
    from bayeformers_amd import ops
    from bayeformers_amd.sampling import sample_bayesian

    ids, mask = _prompt(pad=37, side="right")
    S = 2
    outs = {}
    for name, dtype, fuse in (("ref", torch.float32, False), ("sdpa16", torch.bfloat16, False),
                              ("fused", torch.bfloat16, True)):
        model = _decoder(kind, dtype, fuse)
        c0 = dict(ops.GQA_CALLS)
        bf.manual_seed(SEED)
        with torch.no_grad():
            raw, _, _, _ = sample_bayesian(model, {"input_ids": ids, "attention_mask": mask, "use_cache": False}, S)
        outs[name] = raw[0].float().view(S, *ids.shape, -1)
        if fuse:
            assert ops.GQA_CALLS["fwd_window"] - c0["fwd_window"] == _sliding_layers(kind)
            assert ops.GQA_CALLS["fwd"] - c0["fwd"] == 2 - _sliding_layers(kind)
    valid = mask.bool()[None, :, :, None].expand_as(outs["ref"])
    ref = outs["ref"][valid]
    e16 = (outs["sdpa16"][valid] - ref).abs().max().item() / ref.abs().max().item()
    ef = (outs["fused"][valid] - ref).abs().max().item() / ref.abs().max().item()
    print(f"[{kind}] fused bf16 {ef:.3e}, framework bf16 {e16:.3e} (max |logit - fp32| / max |fp32|)")
    assert ef <= 2 * e16 + 2e-3


@pytest.mark.parametrize("kind", ["mistral", "qwen2"])
def test_sliding_decoder_training_gradients_match_sdpa(kind):
    """Gradients of one Monte-Carlo training loss: the fused bf16 model against the same model on the framework's attention
    in fp32, held to twice the bf16 framework model's own error (relative norm per parameter, plus 1e-2)."""
    import bayeformers_amd as bf
    from bayeformers_amd import ops
    from bayeformers_amd.sampling import sample_bayesian

    ids, mask = _prompt(pad=21, side="right")
    grads = {}
    for name, dtype, fuse in (("ref", torch.float32, False), ("sdpa16", torch.bfloat16, False),
                              ("fused", torch.bfloat16, True)):
        model = _decoder(kind, dtype, fuse)
        for p in model.parameters():
            p.requires_grad_(p.dtype.is_floating_point)
        c0 = dict(ops.GQA_CALLS)
        bf.manual_seed(SEED)
        _, mean, _, _ = sample_bayesian(model, {"input_ids": ids, "attention_mask": mask, "use_cache": False}, 2)
        logits = mean[0].float()
        loss = torch.nn.functional.cross_entropy(logits[:, :-1].reshape(-1, 512), ids[:, 1:].reshape(-1))
        loss.backward()
        if fuse:
            assert ops.GQA_CALLS["bwd_window"] - c0["bwd_window"] == _sliding_layers(kind)
        grads[name] = {n: p.grad.double().clone() for n, p in model.named_parameters() if p.grad is not None}
    assert grads["fused"].keys() == grads["ref"].keys() and grads["ref"]
    worst = 0.0
    for n, g in grads["ref"].items():
        scale = max(g.norm().item(), 1e-30)
        e16 = (grads["sdpa16"][n] - g).norm().item() / scale
        ef = (grads["fused"][n] - g).norm().item() / scale
        worst = max(worst, ef - 2 * e16)
        assert ef <= 2 * e16 + 1e-2, (n, ef, e16)
    print(f"[{kind}] gradients: max(fused - 2 x framework bf16) = {worst:.3e}")


def _generate(model, ids, mask, **kw):
    import bayeformers_amd as bf
    from bayeformers_amd.sampling import sample_generate

    bf.manual_seed(SEED)
    with torch.no_grad():
        return sample_generate(model, ids, attention_mask=mask, samples=3, max_new_tokens=24, **kw)


@pytest.mark.parametrize("kind", list(FAMILIES))
def test_sliding_static_and_graph_generation(kind):
    """prompt 96 + 24 new tokens against W = 100: the window is crossed during the decode."""
    from dataclasses import fields

    from bayeformers_amd import ops

    model = _decoder(kind, torch.bfloat16)
    ids, mask = _prompt(T=96, pad=5)
    d0 = dict(ops.DECODE_CALLS)
    dynamic = _generate(model, ids, mask)
    assert ops.DECODE_CALLS["window"] - d0["window"] == _sliding_layers(kind) * 23
    d1 = dict(ops.DECODE_CALLS)
    static = _generate(model, ids, mask, static_cache=True)
    assert ops.DECODE_CALLS["len_window"] - d1["len_window"] == _sliding_layers(kind) * 23
    assert torch.equal(static.sequences, dynamic.sequences)
    for f in ("predictive_entropy", "expected_entropy", "mutual_information", "token_prob"):
        assert (getattr(static, f) - getattr(dynamic, f)).abs().max().item() < 0.05, f
    d2 = dict(ops.DECODE_CALLS)
    graph = _generate(model, ids, mask, graph=True)
    # eager step 1 + the captured step 2: the replays enqueue nothing from Python
    assert ops.DECODE_CALLS["len_window"] - d2["len_window"] == _sliding_layers(kind) * 2
    assert all(torch.equal(getattr(graph, f.name), getattr(static, f.name)) for f in fields(static))
