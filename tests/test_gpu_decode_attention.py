"""bf_attention_decode_gqa (csrc/bf_attention_decode.hip) against a float64 restatement, and the dispatch of cached decode
steps of a decoder routed through fuse_attention."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

# max |out - ref| / max |ref| allowed: 2x the largest error measured over the cases below on the MI355X (bf16 4.55e-3,
# fp16 5.62e-4: profiles/decode_attention.md); the rounding of P to the operand type dominates
TOL = {torch.bfloat16: 9.1e-3, torch.float16: 1.2e-3}
TKS = [1, 127, 128, 129, 1000, 4099]


def _reference(q, k, v, key_mask, scale):
    """float64: q [N, H, Tq, D], k / v [N, Hkv, Tk, D]; query i sees keys 0 .. Tk - Tq + i; [N, Tq, H, D]."""
    N, H, Tq, D = q.shape
    Hkv, Tk = k.shape[1], k.shape[2]
    G = H // Hkv
    kk = k.double().repeat_interleave(G, 1)
    vv = v.double().repeat_interleave(G, 1)
    s = torch.matmul(q.double(), kk.transpose(-1, -2)) * scale
    if key_mask is not None:
        s = s + key_mask.double()[:, None, None, :]
    i = torch.arange(Tq, device=q.device)[:, None]
    j = torch.arange(Tk, device=q.device)[None, :]
    s = s.masked_fill(j > Tk - Tq + i, float("-inf"))
    m = s.amax(-1, keepdim=True)
    p = torch.where(torch.isinf(m), torch.zeros_like(s), torch.exp(s - m.clamp(min=-1e300)))
    l = p.sum(-1, keepdim=True)
    out = torch.matmul(p, vv) / torch.where(l > 0, l, torch.ones_like(l))
    return out.transpose(1, 2)


def _inputs(layout, N, H, Hkv, Tq, Tk, D, dtype, gen):
    dev = "cuda"
    if layout == "contiguous":
        q = torch.randn(N, H, Tq, D, generator=gen, device=dev).to(dtype)
    else:  # HF's [B, T, H, D] projection viewed as [B, H, T, D]
        q = torch.randn(N, Tq, H, D, generator=gen, device=dev).to(dtype).transpose(1, 2)
    if layout == "slice":  # the first Tk positions of a larger preallocated cache
        big = torch.randn(2, N, Hkv, Tk + 40, D, generator=gen, device=dev).to(dtype)
        k, v = big[0][:, :, :Tk], big[1][:, :, :Tk]
    else:
        k = torch.randn(N, Hkv, Tk, D, generator=gen, device=dev).to(dtype)
        v = torch.randn(N, Hkv, Tk, D, generator=gen, device=dev).to(dtype)
    return q, k, v


def _mask(kind, N, Tk, gen):
    if kind == "none":
        return None
    m = torch.zeros(N, Tk, device="cuda")
    for n in range(N):  # left padding of different lengths
        m[n, : (n * 7) % max(Tk // 2, 1)] = float("-inf")
    if kind == "hidden_row":
        m[N - 1] = float("-inf")
    return m


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("H,Hkv", [(8, 8), (16, 4), (8, 1), (32, 8)])
@pytest.mark.parametrize("Tq", [1, 2, 5, 16])
def test_decode_matches_float64(dtype, D, H, Hkv, Tq):
    from bayeformers_amd import ops

    gen = torch.Generator(device="cuda").manual_seed(1000 * Tq + 10 * H + D)
    N, scale = 3, D ** -0.5
    worst = 0.0
    for Tk in sorted({Tq} | {t for t in TKS if t >= Tq}):
        for layout in ("hf", "contiguous", "slice"):
            for kind in ("none", "padded", "hidden_row"):
                q, k, v = _inputs(layout, N, H, Hkv, Tq, Tk, D, dtype, gen)
                m = _mask(kind, N, Tk, gen)
                assert ops.attention_decode_supported(q, k, v)
                out = ops.attention_forward_decode(q, k, v, m, scale)
                ref = _reference(q, k, v, m, scale)
                assert out.shape == (N, Tq, H, D) and out.is_contiguous()
                assert torch.isfinite(out).all()
                if kind == "hidden_row":
                    assert torch.equal(out[N - 1], torch.zeros_like(out[N - 1]))  # no visible key: exactly 0
                err = (out.double() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)
                worst = max(worst, err)
                assert err < TOL[dtype], (Tk, layout, kind, err)
    log = os.environ.get("BF_DECODE_ERR_LOG")
    if log:
        with open(log, "a") as f:
            f.write(f"{dtype} D={D} H={H} Hkv={Hkv} Tq={Tq} max_rel_err={worst:.3e}\n")


def test_mask_off_flag_skips_the_mask():
    from bayeformers_amd import ops

    gen = torch.Generator(device="cuda").manual_seed(5)
    q, k, v = _inputs("hf", 2, 16, 4, 4, 300, 128, torch.bfloat16, gen)
    m = _mask("padded", 2, 300, gen)
    off = torch.ones(1, dtype=torch.bool, device="cuda")
    a = ops.attention_forward_decode(q, k, v, m, 0.1, off)
    b = ops.attention_forward_decode(q, k, v, None, 0.1)
    assert torch.equal(a, b)


@pytest.mark.parametrize("Tk", [200, 16384])
def test_decode_is_deterministic_and_capturable(Tk):
    from bayeformers_amd import ops

    gen = torch.Generator(device="cuda").manual_seed(7)
    q, k, v = _inputs("hf", 8, 32, 8, 4, Tk, 128, torch.bfloat16, gen)
    m = _mask("padded", 8, Tk, gen)
    assert Tk < 1000 or ops.attention_decode_workspace_bytes(q, k, v) > 0  # (the long cache is split)
    a = ops.attention_forward_decode(q, k, v, m, 0.125)
    b = ops.attention_forward_decode(q, k, v, m, 0.125)
    assert torch.equal(a, b)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.attention_forward_decode(q, k, v, m, 0.125)  # warm-up off the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c = ops.attention_forward_decode(q, k, v, m, 0.125)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(a, c)


def test_refusals():
    from bayeformers_amd import _C, ops

    gen = torch.Generator(device="cuda").manual_seed(3)
    q, k, v = _inputs("hf", 2, 8, 2, 1, 64, 64, torch.bfloat16, gen)
    assert ops.attention_decode_supported(q, k, v)
    q96, k96, v96 = _inputs("hf", 2, 8, 2, 1, 64, 96, torch.bfloat16, gen)
    assert not ops.attention_decode_supported(q96, k96, v96)
    with pytest.raises(_C.BayeFormersAMDError):
        ops.attention_forward_decode(q96, k96, v96, None, 0.1)
    q17, k17, v17 = _inputs("hf", 2, 8, 2, 17, 64, 64, torch.bfloat16, gen)
    assert not ops.attention_decode_supported(q17, k17, v17)
    with pytest.raises(_C.BayeFormersAMDError):
        ops.attention_forward_decode(q17, k17, v17, None, 0.1)
    q6, k6, v6 = _inputs("hf", 2, 6, 4, 1, 64, 64, torch.bfloat16, gen)
    assert not ops.attention_decode_supported(q6, k6, v6)
    with pytest.raises(_C.BayeFormersAMDError):
        ops.attention_forward_decode(q6, k6, v6, None, 0.1)
    kt = torch.randn(2, 2, 64, 64, device="cuda").to(torch.bfloat16).transpose(2, 3)  # features strided
    assert not ops.attention_decode_supported(q, kt, v)
    with pytest.raises(_C.BayeFormersAMDError):
        ops.attention_forward_decode(q, kt, v, None, 0.1)


def _tiny_llama(heads=8, kv_heads=2, layers=2, hidden=512, vocab=512):
    from transformers import LlamaConfig, LlamaForCausalLM

    import bayeformers_amd as bf

    cfg = LlamaConfig(hidden_size=hidden, num_attention_heads=heads, num_key_value_heads=kv_heads, num_hidden_layers=layers,
                      intermediate_size=2 * hidden, vocab_size=vocab, max_position_embeddings=512, tie_word_embeddings=False,
                      attention_dropout=0.0, attn_implementation="sdpa")
    torch.manual_seed(0)
    model = LlamaForCausalLM(cfg).eval()
    bmodel = bf.to_bayesian(model, delta=0.05, freeze=True).eval().cuda()
    freqs = {n: b.detach().clone() for n, b in bmodel.named_buffers() if "inv_freq" in n}
    bmodel = bmodel.to(torch.bfloat16)
    for n, b in freqs.items():
        setattr(bmodel.get_submodule(n.rsplit(".", 1)[0]), n.rsplit(".", 1)[1], b)
    return bmodel


def _set_attn(bmodel, name):
    for m in bmodel.model.modules():
        c = getattr(m, "config", None)
        if c is not None and hasattr(c, "_attn_implementation"):
            c._attn_implementation = name


@pytest.mark.parametrize("padded", [False, True])
def test_cached_decode_step_runs_the_kernel(padded):
    """A cached decode step of a fuse_attention decoder bumps DECODE_CALLS (prefill stays on GQA_CALLS) and its logits match
    the framework-attention path under the same pinned weight draws."""
    from transformers import DynamicCache

    import bayeformers_amd as bf
    from bayeformers_amd import ops

    bf.set_compute_dtype("bf16")
    bmodel = _tiny_llama()
    assert bf.fuse_attention(bmodel)
    S, B, T = 2, 2, 128
    torch.manual_seed(1)
    ids = torch.randint(0, 512, (B, T), device="cuda")
    mask = torch.ones(B, T, dtype=torch.long, device="cuda")
    if padded:
        mask[1, :17] = 0
    nxt = torch.randint(0, 512, (B, 1), device="cuda")

    def run(attn):
        _set_attn(bmodel, attn)
        cache = DynamicCache(config=bmodel.model.config)
        m = mask.repeat(S, 1)
        pos = (m.cumsum(-1) - 1).clamp(min=0)
        with torch.no_grad():
            bmodel(input_ids=ids.repeat(S, 1), attention_mask=m, position_ids=pos, past_key_values=cache, use_cache=True)
            gqa, dec = ops.GQA_CALLS["fwd"], ops.DECODE_CALLS["fwd"]
            m2 = torch.cat([m, m.new_ones(S * B, 1)], 1)
            out = bmodel(input_ids=nxt.repeat(S, 1), attention_mask=m2, position_ids=pos[:, -1:] + 1, past_key_values=cache,
                         use_cache=True)
            return out.logits.float(), (gqa, ops.GQA_CALLS["fwd"], dec, ops.DECODE_CALLS["fwd"])

    with bmodel.monte_carlo(S), bmodel.pinned_samples():
        g0, d0 = ops.GQA_CALLS["fwd"], ops.DECODE_CALLS["fwd"]
        ours, (gqa_pre, gqa_post, dec_pre, dec_post) = run("bayeformers_amd")
        assert gqa_pre - g0 == 2 and dec_pre == d0  # prefill: the cache-free kernel, once per layer
        assert gqa_post == gqa_pre and dec_post - dec_pre == 2  # the decode step: the decode kernel, once per layer
        theirs, _ = run("sdpa")
    err = (ours - theirs).abs().max().item() / theirs.abs().max().item()
    assert err < 3e-2, err
