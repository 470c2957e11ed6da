"""pinned_samples(keep_weights=True): the skinny decode GEMM (bf_gemm_nt_skinny) and generation on weights drawn once."""
import numpy as np
import pytest
import torch

from bayeformers_amd import _C, ops

pytestmark = pytest.mark.gpu

SEED = 0x5EED
TOL = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}  # test_gemm_nt_against_torch's, relative to max |ref|

# the decoder of DESIGN 4.5 (q/o, k/v, gate/up, down, lm_head), small and ragged shapes, and (200, 4128): split K, uneven
KERNEL_SHAPES = [(16, 32), (100, 64), (1024, 1024), (256, 1024), (2816, 1024), (1024, 2816), (32000, 1024), (200, 4128)]


def _gelu64(v):
    return 0.5 * v * (1.0 + torch.erf(v / np.sqrt(2.0)))


def _skinny(x, w, b, S, N, K, act, stride=None):
    return ops.skinny_linear_forward(x, w, b, S, N, K, act, x_sample_stride=stride)


@pytest.mark.parametrize("N,K", KERNEL_SHAPES)
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_skinny_against_float64(N, K, dt):
    g = torch.Generator(device="cuda").manual_seed(N * 7919 + K)
    Smax, Mmax = 10, 64
    w = torch.randn(Smax, N, K, device="cuda", generator=g).to(dt)
    # rows of x live in a [S, Mmax + 3, K] buffer: the sample stride is larger than M * K
    xbuf = torch.randn(Smax, Mmax + 3, K, device="cuda", generator=g).to(dt)
    bias = torch.randn(Smax, N, device="cuda", generator=g)
    w64 = w.double()
    for S in (1, 4, 10):
        for i, M in enumerate((1, 2, 4, 16, 17, 33, 64)):
            x = xbuf[:S, :M]
            ref = torch.einsum("smk,snk->smn", x.double(), w64[:S])
            for with_bias, act in ((True, 0), (False, 1)) if i % 2 == 0 else ((False, 0), (True, 1)):
                r = ref + bias[:S, None, :].double() if with_bias else ref
                r = _gelu64(r) if act else r
                b = bias[:S].contiguous() if with_bias else None
                y = _skinny(x, w[:S], b, S, N, K, act, stride=(Mmax + 3) * K).view(S, M, N)
                err = (y.double() - r).abs().max().item()
                assert err <= TOL[dt] * r.abs().max().item() + 1e-5 * np.sqrt(K), (S, M, with_bias, act, err)
            # contiguous x (sample stride M * K) and a second call: bitwise equal
            xc = x.contiguous()
            y1 = _skinny(xc.view(S * M, K), w[:S], bias[:S].contiguous(), S, N, K, 0)
            y2 = _skinny(xc.view(S * M, K), w[:S], bias[:S].contiguous(), S, N, K, 0)
            assert torch.equal(y1, y2)
            err = (y1.view(S, M, N).double() - ref - bias[:S, None, :].double()).abs().max().item()
            assert err <= TOL[dt] * (ref.abs().max().item() + 4.0) + 1e-5 * np.sqrt(K)


@pytest.mark.parametrize("S,M,N,K", [(4, 4, 1024, 1024), (4, 4, 200, 4128), (10, 33, 100, 64)])
def test_skinny_graph_replay_is_bitwise_eager(S, M, N, K):
    dt = torch.bfloat16
    g = torch.Generator(device="cuda").manual_seed(S + M + N + K)
    w = torch.randn(S, N, K, device="cuda", generator=g).to(dt)
    x = torch.randn(S * M, K, device="cuda", generator=g).to(dt)
    b = torch.randn(S, N, device="cuda", generator=g)
    eager = _skinny(x, w, b, S, N, K, 1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _skinny(x, w, b, S, N, K, 1)  # this stream's workspace exists before capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = _skinny(x, w, b, S, N, K, 1)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_skinny_refuses_bad_arguments():
    w = torch.zeros(2, 64, 48, dtype=torch.bfloat16, device="cuda")
    x = torch.zeros(2, 48, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(_C.BayeFormersAMDError, match="K % 32"):
        _skinny(x, w, None, 2, 64, 48, 0)
    w = torch.zeros(2, 64, 64, dtype=torch.bfloat16, device="cuda")
    x = torch.zeros(2 * 65, 64, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(_C.BayeFormersAMDError, match="M <= 64"):
        _skinny(x, w, None, 2, 64, 64, 0)
    assert not ops.skinny_supported(x, w, 2, 64)
    assert ops.skinny_supported(x[:2 * ops.SKINNY_ROWS], w, 2, 64)


# ---------------------------------------------------------------------------------------------------------- generation
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


def _prompt(B=2, T=128, vocab=512):
    g = torch.Generator().manual_seed(11)
    return torch.randint(0, vocab, (B, T), generator=g).cuda()


def _count_launches(monkeypatch):
    lib = _C.lib()
    counts = {"bf_sample_logprob_table": 0, "bf_linear_fwd": 0, "bf_sample_logprob": 0}
    for name in counts:
        real = getattr(lib, name)

        def wrapper(*a, _real=real, _name=name):
            counts[_name] += 1
            return _real(*a)

        monkeypatch.setattr(lib, name, wrapper)
    return counts


def test_kept_draws_equal_plan_draws_and_log_probs():
    import bayeformers_amd as bf
    from bayeformers_amd.nn.layers.linear import Linear
    from bayeformers_amd.sampling import sample_bayesian

    bmodel = _llama(torch.bfloat16)
    ids = _prompt()
    S = 3
    bf.manual_seed(SEED)
    with torch.no_grad():
        sample_bayesian(bmodel, {"input_ids": ids, "use_cache": False}, S)
    lp_ref = bmodel.log_prob_samples().clone()
    bf.manual_seed(SEED)
    with torch.no_grad(), bmodel.monte_carlo(S), bmodel.pinned_samples(keep_weights=True):
        bmodel(input_ids=ids.repeat(S, 1), use_cache=False)
        lp = bmodel.log_prob_samples().clone()
        base, plan = bmodel._last_base, bmodel._kept.plan
        linears = [l for l in bmodel.fused_children() if isinstance(l, Linear)]
        assert len(plan.layers) == len(linears)
        for layer in (linears[0], linears[5], linears[-1]):
            (w_ref,), _ = ops.sample_logprob([layer.weight], [layer.weight_prior], [2 * layer.layer_id], S, bf.random.STATE.seed,
                                             base, out_dtype=torch.bfloat16)
            assert torch.equal(plan.views[id(layer)][0], w_ref)
    assert torch.equal(lp, lp_ref)
    assert bmodel.__dict__.get("_kept") is None


def test_generate_keep_weights_bf16_matches_teacher_forcing(monkeypatch):
    import bayeformers_amd as bf
    from bayeformers_amd.sampling import mc_predictive, sample_bayesian, sample_generate

    bmodel = _llama(torch.bfloat16)
    ids = _prompt()
    S, n, T0 = 3, 8, ids.shape[1]
    bf.manual_seed(SEED)
    with torch.no_grad():
        sample_bayesian(bmodel, {"input_ids": ids, "use_cache": False}, S)
    lp_ref = bmodel.log_prob_samples().clone()
    counts = _count_launches(monkeypatch)
    k0, d0 = ops.SKINNY_CALLS[0], ops.DECODE_CALLS["fwd"]
    bf.manual_seed(SEED)
    with torch.no_grad():
        gen = sample_generate(bmodel, ids, samples=S, max_new_tokens=n, keep_weights=True)
    # one sampling launch for the whole generation, no per-layer forward (fused_small lives in bf_linear_fwd)
    assert counts == {"bf_sample_logprob_table": 1, "bf_linear_fwd": 0, "bf_sample_logprob": 0}, counts
    assert ops.SKINNY_CALLS[0] - k0 == 15 * (n - 1)  # 7 Linear layers per decoder layer and the head, every decode step
    assert ops.DECODE_CALLS["fwd"] - d0 == 2 * (n - 1)
    monkeypatch.undo()
    assert torch.equal(lp_ref[:, 0], gen.log_prior) and torch.equal(lp_ref[:, 1], gen.log_variational_posterior)
    assert torch.equal(bmodel.log_prob_samples()[:, 0], gen.log_prior)
    bf.manual_seed(SEED)
    with torch.no_grad():
        raw, _, _, _ = sample_bayesian(bmodel, {"input_ids": gen.sequences[:, :-1], "use_cache": False}, S)
    pred = mc_predictive(raw[0][:, :, T0 - 1:])
    assert torch.equal(pred.prediction, gen.sequences[:, T0:])
    for ours, ref in ((gen.predictive_entropy, pred.predictive_entropy), (gen.expected_entropy, pred.expected_entropy),
                      (gen.mutual_information, pred.mutual_information)):
        assert (ours - ref).abs().max().item() < 0.05  # test_generate_bf16_matches_teacher_forcing_and_pins_log_probs's bound


def test_generate_keep_weights_matches_reference_fixture(golden_dir):
    """fp32 (the kept fp32 weights on the fp32 GEMM) against tests/golden/generate_gqa64.npz, as
    test_generate_matches_reference_fixture."""
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
                                  max_new_tokens=n, temperature=float(g["temperature"]), keep_weights=True)
    finally:
        bf.set_compute_dtype("bf16")
    assert np.array_equal(gen.sequences[:, T0:].cpu().numpy(), g["tokens"])
    for name in ("predictive_entropy", "expected_entropy", "mutual_information", "token_prob"):
        np.testing.assert_allclose(getattr(gen, name).cpu().numpy(), g[name], rtol=0, atol=1e-4, err_msg=name)
    np.testing.assert_allclose(gen.log_prior.cpu().numpy(), g["log_prior"], rtol=2e-6)
    np.testing.assert_allclose(gen.log_variational_posterior.cpu().numpy(), g["lvp"], rtol=2e-6)


def test_generate_keep_weights_device_counter_padding_and_eos():
    import bayeformers_amd as bf
    from bayeformers_amd.sampling import sample_generate

    bmodel = _llama(torch.bfloat16)
    ids = _prompt()
    mask = torch.ones_like(ids)
    mask[1, :7] = 0
    S, n = 2, 6
    with torch.no_grad():
        bf.manual_seed(SEED)
        host = sample_generate(bmodel, ids, attention_mask=mask, samples=S, max_new_tokens=n, keep_weights=True)
        bf.manual_seed(SEED)
        alone = sample_generate(bmodel, ids[1:, 7:], samples=S, max_new_tokens=n, keep_weights=True)
    assert torch.equal(host.sequences[1, 128:], alone.sequences[0, 121:])
    bf.manual_seed(SEED)
    bf.use_device_counter(True)
    try:
        with torch.no_grad():
            dev = sample_generate(bmodel, ids, attention_mask=mask, samples=S, max_new_tokens=n, keep_weights=True)
        assert int(bf.random.STATE.device_counter.item()) == S  # committed once
    finally:
        bf.use_device_counter(False)
    assert torch.equal(host.sequences, dev.sequences) and torch.equal(host.log_prior, dev.log_prior)
    # EOS: row 0 ends at the token it emits at step 2
    eos = int(host.sequences[0, 128 + 2])
    first = (host.sequences[0, 128:] == eos).nonzero()[0].item()
    with torch.no_grad():
        bf.manual_seed(SEED)
        g = sample_generate(bmodel, ids, attention_mask=mask, samples=S, max_new_tokens=n, eos_token_id=eos, pad_token_id=7,
                            keep_weights=True)
    assert int(g.lengths[0]) == first + 1
    assert torch.equal(g.sequences[0, 128:129 + first], host.sequences[0, 128:129 + first])
    assert (g.sequences[0, 129 + first:] == 7).all() and (g.token_prob[0, first + 1:] == 0).all()


def test_keep_weights_refusals(monkeypatch):
    import bayeformers_amd as bf
    from bayeformers_amd.plan import kept_weight_bytes

    bmodel = _llama(torch.bfloat16)
    ids = _prompt(T=16)
    S = 2
    need = kept_weight_bytes(bmodel, S, torch.bfloat16)
    counts = _count_launches(monkeypatch)
    bf.manual_seed(SEED)
    with torch.no_grad(), bmodel.monte_carlo(S), pytest.raises(ValueError, match=str(need)):
        with bmodel.pinned_samples(keep_weights=True, max_bytes=need - 1):
            bmodel(input_ids=ids.repeat(S, 1), use_cache=False)
    assert sum(counts.values()) == 0 and bf.random.STATE.next_sample == 0
    with bmodel.monte_carlo(S), pytest.raises(RuntimeError, match="no_grad"):
        with bmodel.pinned_samples(keep_weights=True):
            pass
    # parameters are read once: an in-place edit of mu inside the block makes the next forward raise
    layer = bmodel.model.model.layers[0].mlp.up_proj
    with torch.no_grad(), bmodel.monte_carlo(S), bmodel.pinned_samples(keep_weights=True):
        bmodel(input_ids=ids.repeat(S, 1), use_cache=False)
        layer.weight.mu.mul_(1.0)
        with pytest.raises(RuntimeError, match="changed inside the block"):
            bmodel(input_ids=ids.repeat(S, 1), use_cache=False)
        # ... and grad enabled inside the block
    with torch.no_grad(), bmodel.monte_carlo(S), bmodel.pinned_samples(keep_weights=True):
        with torch.enable_grad(), pytest.raises(RuntimeError, match="without gradients"):
            bmodel(input_ids=ids.repeat(S, 1), use_cache=False)
