"""Graph-replayed generation over a static KV cache: bf_attention_decode_gqa_len against float64 and against
bf_attention_decode_gqa, bf_generate_step against a torch restatement of sample_generate's loop, and
sample_generate(static_cache=True / graph=True) end to end."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

SEED = 0x5EED
TOL = {torch.bfloat16: 9.1e-3, torch.float16: 1.2e-3}  # tests/test_gpu_decode_attention.py's bounds


# ---- bf_attention_decode_gqa_len -------------------------------------------------------------------------------------
def _reference(q, k, v, L, key_mask, scale):
    """float64 over the first L keys: query i sees keys 0 .. L - Tq + i; [N, Tq, H, D]."""
    N, H, Tq, D = q.shape
    G = H // k.shape[1]
    kk = k[:, :, :L].double().repeat_interleave(G, 1)
    vv = v[:, :, :L].double().repeat_interleave(G, 1)
    s = torch.matmul(q.double(), kk.transpose(-1, -2)) * scale
    if key_mask is not None:
        s = s + key_mask[:, :L].double()[:, None, None, :]
    i = torch.arange(Tq, device=q.device)[:, None]
    j = torch.arange(L, device=q.device)[None, :]
    s = s.masked_fill(j > L - Tq + i, float("-inf"))
    m = s.amax(-1, keepdim=True) if L > 0 else torch.full(s.shape[:-1] + (1,), float("-inf"), device=q.device)
    p = torch.where(torch.isinf(m), torch.zeros_like(s), torch.exp(s - m.clamp(min=-1e300)))
    l = p.sum(-1, keepdim=True)
    out = torch.matmul(p, vv) / torch.where(l > 0, l, torch.ones_like(l))
    return out.transpose(1, 2)


def _cache(N, H, Hkv, Tq, cap, D, dtype, gen, L=None):
    """HF-layout q and a [N, Hkv, cap, D] cache; the slots from L on hold NaN (never read)."""
    q = torch.randn(N, Tq, H, D, generator=gen, device="cuda").to(dtype).transpose(1, 2)
    k = torch.randn(N, Hkv, cap, D, generator=gen, device="cuda").to(dtype)
    v = torch.randn(N, Hkv, cap, D, generator=gen, device="cuda").to(dtype)
    if L is not None:
        k[:, :, L:] = float("nan")
        v[:, :, L:] = float("nan")
    return q, k, v


def _padding(N, cap):
    m = torch.zeros(N, cap, device="cuda")
    for n in range(N):
        m[n, : (n * 7) % 40] = float("-inf")
    return m


def _len(L):
    return torch.tensor([L], dtype=torch.int64, device="cuda")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("H,Hkv", [(8, 8), (16, 4), (8, 1)], ids=["mha", "gqa", "mqa"])
@pytest.mark.parametrize("Tq", [1, 5, 16])
def test_decode_len_matches_float64(dtype, D, H, Hkv, Tq):
    from bayeformers_amd import ops

    gen = torch.Generator(device="cuda").manual_seed(100 * Tq + H + D)
    N, cap, scale = 2, 1000, D ** -0.5
    # the capacity's split: 8 splits of 128 keys at N * Hkv <= 32; L at, around and far below the boundaries
    for L in sorted({Tq, 1, 64, 127, 128, 129, 255, 256, 257, 500, 999, 1000} - {l for l in range(Tq) if l != 1}):
        for padded in (False, True):
            q, k, v = _cache(N, H, Hkv, Tq, cap, D, dtype, gen, L=L)
            m = _padding(N, cap) if padded else None
            out = ops.attention_forward_decode_len(q, k, v, _len(L), m, scale)
            assert out.shape == (N, Tq, H, D) and torch.isfinite(out).all(), (L, padded)
            ref = _reference(q, k, v, L, m, scale)
            err = (out.double() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)
            assert err < TOL[dtype], (L, padded, err)


@pytest.mark.parametrize("N,H,Hkv,Tq,cap,D", [(2, 8, 2, 1, 1000, 64), (3, 16, 4, 4, 300, 128), (1, 32, 8, 1, 4099, 128),
                                               (8, 32, 8, 16, 16384, 128), (4, 8, 8, 1, 77, 64)])
def test_decode_len_at_capacity_is_the_decode_kernel(N, H, Hkv, Tq, cap, D):
    from bayeformers_amd import ops

    gen = torch.Generator(device="cuda").manual_seed(cap)
    q, k, v = _cache(N, H, Hkv, Tq, cap, D, torch.bfloat16, gen)
    for m in (None, _padding(N, cap)):
        a = ops.attention_forward_decode(q, k, v, m, 0.125)
        b = ops.attention_forward_decode_len(q, k, v, _len(cap), m, 0.125)
        assert torch.equal(a, b)


@pytest.mark.parametrize("cap", [200, 3000])
def test_one_captured_launch_follows_the_fill(cap):
    from bayeformers_amd import ops

    gen = torch.Generator(device="cuda").manual_seed(9)
    q, k, v = _cache(4, 16, 4, 1, cap, 128, torch.bfloat16, gen)
    m = _padding(4, cap)
    kv_len = _len(1)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.attention_forward_decode_len(q, k, v, kv_len, m, 0.125)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ops.attention_forward_decode_len(q, k, v, kv_len, m, 0.125)
    for L in sorted({1, 2, 63, 64, 65, 127, 128, 129, cap // 2, cap - 1, cap}):
        kv_len.fill_(L)
        g.replay()
        ref = ops.attention_forward_decode_len(q, k, v, _len(L), m, 0.125)
        torch.cuda.synchronize()
        assert torch.equal(out, ref), L


# ---- bf_generate_step ------------------------------------------------------------------------------------------------
def _buffers(B, S, T0, n, dev="cuda"):
    return dict(state=torch.zeros(2, dtype=torch.long, device=dev),
                sequences=torch.full((B, T0 + n), -5, dtype=torch.long, device=dev),
                stats=torch.zeros((4, B, n), dtype=torch.float32, device=dev),
                finished=torch.zeros(B, dtype=torch.bool, device=dev), lengths=torch.zeros(B, dtype=torch.long, device=dev),
                next_ids=torch.zeros(S * B, dtype=torch.long, device=dev),
                positions=torch.arange(S * B, dtype=torch.long, device=dev))


def _step(pred, S, T0, buf, eos, pad, seed=None):
    from bayeformers_amd import ops

    ops.generate_step(pred.probs, pred.predictive_entropy, pred.expected_entropy, pred.mutual_information, S, buf["state"],
                      buf["sequences"], T0, buf["stats"], buf["finished"], buf["lengths"], buf["next_ids"],
                      buf["positions"], eos, pad, seed)


@pytest.mark.parametrize("V", [50, 1024, 5000])
def test_generate_step_greedy_is_the_prediction(V):
    from bayeformers_amd.sampling import mc_predictive

    gen = torch.Generator(device="cuda").manual_seed(V)
    S, B, T0 = 3, 5, 4
    logits = torch.randn(S, B, V, generator=gen, device="cuda")
    logits[:, 1, :] = 0.0  # a row of ties: the lowest index
    pred = mc_predictive(logits)
    buf = _buffers(B, S, T0, 1)
    _step(pred, S, T0, buf, None, 0)
    tok = buf["sequences"][:, T0]
    assert torch.equal(tok, pred.prediction) and int(tok[1]) == 0
    stats = torch.stack([pred.predictive_entropy, pred.expected_entropy, pred.mutual_information,
                         pred.probs.gather(1, tok[:, None]).squeeze(1)])
    assert torch.equal(buf["stats"][:, :, 0], stats)
    assert buf["state"].tolist() == [1, 0] and torch.equal(buf["next_ids"], tok.repeat(S))


def test_generate_step_matches_the_loop():
    """Finished, lengths, pad and the statistics over several steps: a torch restatement of sample_generate's loop."""
    from bayeformers_amd.sampling import mc_predictive

    gen = torch.Generator(device="cuda").manual_seed(3)
    S, B, T0, n, V, pad = 2, 6, 3, 5, 40, 1
    preds = [mc_predictive(torch.randn(S, B, V, generator=gen, device="cuda") * 3) for _ in range(n)]
    eos = int(preds[0].prediction[0])  # row 0 ends at once; others when they hit it
    buf = _buffers(B, S, T0, n)
    sequences, stats = buf["sequences"].clone(), buf["stats"].clone()
    lengths, finished, positions = buf["lengths"].clone(), buf["finished"].clone(), buf["positions"].clone()
    for t, pred in enumerate(preds):
        _step(pred, S, T0, buf, eos, pad)
        tok = pred.prediction
        st = torch.stack([pred.predictive_entropy, pred.expected_entropy, pred.mutual_information,
                          pred.probs.gather(1, tok[:, None]).squeeze(1)])
        tok = torch.where(finished, torch.full_like(tok, pad), tok)
        st = torch.where(finished[None, :], 0.0, st)
        lengths += (~finished).long()
        finished = finished | (tok == eos)
        sequences[:, T0 + t] = tok
        stats[:, :, t] = st
        positions += 1
        assert torch.equal(buf["next_ids"], tok.repeat(S)), t
    assert bool(finished[0]) and int(lengths[0]) == 1
    assert torch.equal(buf["sequences"], sequences) and torch.equal(buf["stats"], stats)
    assert torch.equal(buf["lengths"], lengths) and torch.equal(buf["finished"], finished)
    assert torch.equal(buf["positions"], positions) and buf["state"].tolist() == [n, 0]
    _step(preds[0], S, T0, buf, eos, pad)  # past the last step: nothing moves
    assert torch.equal(buf["sequences"], sequences) and buf["state"].tolist() == [n, 0]


def _draw(probs, seed, steps=1):
    """Tokens of `steps` sampled epilogue launches on the fixed probability rows; [steps, B]."""
    from bayeformers_amd import ops

    B = probs.shape[0]
    zero = torch.zeros(B, device="cuda")
    buf = _buffers(B, 1, 0, steps)
    s = torch.tensor([seed], dtype=torch.long, device="cuda")
    for _ in range(steps):
        ops.generate_step(probs, zero, zero, zero, 1, buf["state"], buf["sequences"], 0, buf["stats"], None,
                          buf["lengths"], buf["next_ids"], None, None, 0, s)
    return buf["sequences"].T.contiguous()


def test_generate_step_sampling_is_reproducible_and_skips_zeros():
    gen = torch.Generator(device="cuda").manual_seed(4)
    B, V = 64, 3000
    probs = torch.rand(B, V, generator=gen, device="cuda")
    probs[:, ::3] = 0.0  # never drawn
    probs /= probs.sum(-1, keepdim=True)
    a, b = _draw(probs, 123, steps=4), _draw(probs, 123, steps=4)
    assert torch.equal(a, b)
    assert not torch.equal(a, _draw(probs, 124, steps=4))
    assert not torch.equal(a[0], a[1])  # a new uniform every step
    assert (probs.gather(1, a.T) > 0).all()


@pytest.mark.parametrize("V", [10, 2500])
def test_generate_step_frequencies_pass_chi_square(V):
    """2^16 rows of one probability row at a fixed seed: the token frequencies against the probabilities."""
    gen = torch.Generator(device="cuda").manual_seed(V)
    p = torch.rand(V, generator=gen, device="cuda", dtype=torch.float64) + 0.2
    p[V // 3] = 0.0
    p /= p.sum()
    R = 1 << 16
    toks = _draw(p.float()[None, :].repeat(R, 1), 0xC0FFEE)[0]
    counts = torch.bincount(toks, minlength=V).double()
    assert counts[V // 3] == 0
    keep = p > 0
    expected = p[keep] * R
    chi2 = float(((counts[keep] - expected) ** 2 / expected).sum())
    df = int(keep.sum()) - 1
    bound = df + 4.0 * math.sqrt(2.0 * df)  # ~ the 0.9999 quantile (fixed seed: the test is deterministic)
    assert chi2 < bound, (chi2, bound)


# ---- sample_generate end to end --------------------------------------------------------------------------------------
def _llama(dtype, heads=8, kv_heads=2, layers=2, hidden=512, vocab=512):
    from transformers import LlamaConfig, LlamaForCausalLM

    import bayeformers_amd as bf

    cfg = LlamaConfig(hidden_size=hidden, num_attention_heads=heads, num_key_value_heads=kv_heads, num_hidden_layers=layers,
                      intermediate_size=2 * hidden, vocab_size=vocab, max_position_embeddings=512, tie_word_embeddings=False,
                      attention_dropout=0.0, attn_implementation="sdpa")
    torch.manual_seed(0)
    bmodel = bf.to_bayesian(LlamaForCausalLM(cfg).eval(), delta=0.05, freeze=True).eval().cuda()
    if dtype == torch.bfloat16:
        freqs = {n: b.detach().clone() for n, b in bmodel.named_buffers() if "inv_freq" in n}
        bmodel = bmodel.to(dtype)
        for n, b in freqs.items():
            setattr(bmodel.get_submodule(n.rsplit(".", 1)[0]), n.rsplit(".", 1)[1], b)
    assert bf.fuse_attention(bmodel)
    bf.set_compute_dtype("bf16" if dtype == torch.bfloat16 else "fp32")
    return bmodel


def _prompt(B=2, T=64, vocab=512, pad=0):
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(0, vocab, (B, T), generator=g).cuda()
    mask = torch.ones_like(ids)
    mask[B - 1, :pad] = 0
    return ids, (mask if pad else None)


def _gen(bmodel, ids, mask, **kw):
    import bayeformers_amd as bf
    from bayeformers_amd.sampling import sample_generate

    bf.manual_seed(SEED)
    gen = kw.pop("gen_seed", None)
    with torch.no_grad():
        return sample_generate(bmodel, ids, attention_mask=mask, samples=3,
                               generator=torch.Generator(device="cuda").manual_seed(gen) if gen is not None else None, **kw)


def _settle(bmodel, ids, mask, **kw):
    """A first generation on a fresh model: its prefill runs before any layer was seen with a few rows per sample (the
    sampling plan then covers every layer, and the log-probs are summed in another order than in every later prefill)."""
    return _gen(bmodel, ids, mask, max_new_tokens=2, **kw)


def _equal(a, b):
    from dataclasses import fields

    return all(torch.equal(getattr(a, f.name), getattr(b, f.name)) for f in fields(a))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("do_sample", [False, True], ids=["greedy", "sample"])
@pytest.mark.parametrize("keep", [False, True], ids=["draw", "keep"])
def test_graph_equals_static_eager(dtype, do_sample, keep):
    import bayeformers_amd as bf

    bmodel = _llama(dtype)
    try:
        ids, mask = _prompt(pad=9)
        kw = dict(max_new_tokens=20, do_sample=do_sample, temperature=0.8, keep_weights=keep,
                  gen_seed=5 if do_sample else None)
        _settle(bmodel, ids, mask)
        static = _gen(bmodel, ids, mask, static_cache=True, **kw)
        graph = _gen(bmodel, ids, mask, graph=True, **kw)
        assert _equal(static, graph)
        assert torch.equal(graph.lengths, torch.full((2,), 20, device="cuda")) and (graph.token_prob > 0).all()
        if do_sample:  # another generator seed, another text
            assert not torch.equal(_gen(bmodel, ids, mask, graph=True, **dict(kw, gen_seed=6)).sequences, graph.sequences)
    finally:
        bf.set_compute_dtype("bf16")


@pytest.mark.parametrize("do_sample", [False, True], ids=["greedy", "sample"])
def test_graph_eos_stops_rows_like_static(do_sample):
    bmodel = _llama(torch.bfloat16)
    ids, mask = _prompt(B=3, pad=5)
    kw = dict(max_new_tokens=24, do_sample=do_sample, gen_seed=2 if do_sample else None)
    free = _gen(bmodel, ids, mask, static_cache=True, **kw)
    eos = int(free.sequences[0, 64 + 2])
    first = int((free.sequences[0, 64:] == eos).nonzero()[0])
    static = _gen(bmodel, ids, mask, static_cache=True, eos_token_id=eos, pad_token_id=7, **kw)
    graph = _gen(bmodel, ids, mask, graph=True, eos_token_id=eos, pad_token_id=7, **kw)
    assert _equal(static, graph)
    assert int(graph.lengths[0]) == first + 1 and (graph.sequences[0, 65 + first:] == 7).all()
    assert (graph.predictive_entropy[0, first + 1:] == 0).all() and (graph.token_prob[0, :first + 1] > 0).all()


def test_static_greedy_matches_teacher_forcing_and_pins_log_probs():
    import bayeformers_amd as bf
    from bayeformers_amd import ops
    from bayeformers_amd.sampling import mc_predictive, sample_bayesian

    bmodel = _llama(torch.bfloat16)
    ids, _ = _prompt(T=128)
    S, n, T0 = 3, 8, 128
    bf.manual_seed(SEED)
    with torch.no_grad():
        sample_bayesian(bmodel, {"input_ids": ids, "use_cache": False}, S)
    lp_ref = bmodel.log_prob_samples().clone()
    d0 = ops.DECODE_CALLS["len"]
    for graph in (False, True):
        bf.manual_seed(SEED)
        with torch.no_grad():
            from bayeformers_amd.sampling import sample_generate

            gen = sample_generate(bmodel, ids, samples=S, max_new_tokens=n, static_cache=True, graph=graph)
        assert torch.equal(lp_ref[:, 0], gen.log_prior) and torch.equal(lp_ref[:, 1], gen.log_variational_posterior)
        bf.manual_seed(SEED)
        with torch.no_grad():
            raw, _, _, _ = sample_bayesian(bmodel, {"input_ids": gen.sequences[:, :-1], "use_cache": False}, S)
        pred = mc_predictive(raw[0][:, :, T0 - 1:])
        assert torch.equal(pred.prediction, gen.sequences[:, T0:])
        for ours, ref in ((gen.predictive_entropy, pred.predictive_entropy), (gen.expected_entropy, pred.expected_entropy),
                          (gen.mutual_information, pred.mutual_information)):
            assert (ours - ref).abs().max().item() < 0.05
    assert ops.DECODE_CALLS["len"] - d0 == 2 * (n - 1) + 2 * 2  # eager: every step; graph: warm-up + capture


def test_graph_matches_reference_fixture(golden_dir):
    """fp32 greedy through the graph path against tests/golden/generate_gqa64.npz: the same tokens, statistics within 1e-4."""
    import numpy as np
    from transformers import LlamaConfig, LlamaForCausalLM

    import bayeformers_amd as bf
    from bayeformers_amd.sampling import sample_generate

    g = np.load(f"{golden_dir}/generate_gqa64.npz")
    hidden, heads, kv_heads, layers, ffn, vocab, T0, B, S, n, pad = (int(x) for x in g["config"])
    cfg = LlamaConfig(hidden_size=hidden, num_attention_heads=heads, num_key_value_heads=kv_heads, num_hidden_layers=layers,
                      intermediate_size=ffn, vocab_size=vocab, max_position_embeddings=64, tie_word_embeddings=False,
                      use_cache=False, attention_dropout=0.0, attn_implementation="sdpa")
    torch.manual_seed(int(g["model_seed"]))
    bmodel = bf.to_bayesian(LlamaForCausalLM(cfg).eval(), delta=float(g["delta"]), freeze=True).eval().cuda()
    assert bf.fuse_attention(bmodel)
    bf.set_compute_dtype("fp32")
    bf.manual_seed(SEED)
    try:
        with torch.no_grad():
            gen = sample_generate(bmodel, torch.from_numpy(g["ids"]).cuda(), torch.from_numpy(g["mask"]).cuda(), samples=S,
                                  max_new_tokens=n, temperature=float(g["temperature"]), graph=True)
    finally:
        bf.set_compute_dtype("bf16")
    assert np.array_equal(gen.sequences[:, T0:].cpu().numpy(), g["tokens"])
    for name in ("predictive_entropy", "expected_entropy", "mutual_information", "token_prob"):
        np.testing.assert_allclose(getattr(gen, name).cpu().numpy(), g[name], rtol=0, atol=1e-4, err_msg=name)
    np.testing.assert_allclose(gen.log_prior.cpu().numpy(), g["log_prior"], rtol=2e-6)
    np.testing.assert_allclose(gen.log_variational_posterior.cpu().numpy(), g["lvp"], rtol=2e-6)


@pytest.mark.parametrize("keep", [False, True], ids=["draw", "keep"])
def test_graph_replays_and_leaves_the_model_alone(keep):
    """The Python-level launches grow by the warm-up and the capture only, whatever max_new_tokens; the model's own graph
    cache and a later default-path generation are unaffected."""
    from bayeformers_amd import ops
    from bayeformers_amd.sampling import graphed_samplers

    bmodel = _llama(torch.bfloat16)
    ids, mask = _prompt(pad=4)
    _settle(bmodel, ids, mask, keep_weights=keep)
    before = _gen(bmodel, ids, mask, max_new_tokens=6, keep_weights=keep)
    samplers = list(graphed_samplers(bmodel))
    counts = []
    for n in (6, 30):
        d, k, e = ops.DECODE_CALLS["len"], ops.SKINNY_CALLS[0], ops.GENERATE_CALLS[0]
        _gen(bmodel, ids, mask, max_new_tokens=n, keep_weights=keep, graph=True)
        counts.append((ops.DECODE_CALLS["len"] - d, ops.SKINNY_CALLS[0] - k, ops.GENERATE_CALLS[0] - e))
    assert counts[0] == counts[1] and counts[0][0] == 2 * 2 and counts[0][2] == 3, counts
    assert (counts[0][1] > 0) == keep
    assert list(graphed_samplers(bmodel)) == samplers
    assert _equal(before, _gen(bmodel, ids, mask, max_new_tokens=6, keep_weights=keep))
