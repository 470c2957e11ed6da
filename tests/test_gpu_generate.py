"""sample_generate: Monte-Carlo generation of a Bayesian decoder on one pinned reservation of sample indices."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SEED = 0x5EED


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


def test_generate_bf16_matches_teacher_forcing_and_pins_log_probs():
    import bayeformers_amd as bf
    from bayeformers_amd import ops
    from bayeformers_amd.sampling import mc_predictive, sample_bayesian, sample_generate

    bmodel = _llama(torch.bfloat16)
    ids = _prompt()
    S, n, T0 = 3, 8, ids.shape[1]
    bf.manual_seed(SEED)
    with torch.no_grad():
        sample_bayesian(bmodel, {"input_ids": ids, "use_cache": False}, S)
    lp_ref = bmodel.log_prob_samples().clone()
    bf.manual_seed(SEED)
    d0 = ops.DECODE_CALLS["fwd"]
    with torch.no_grad():
        gen = sample_generate(bmodel, ids, samples=S, max_new_tokens=n)
    assert ops.DECODE_CALLS["fwd"] - d0 == 2 * (n - 1)  # every decode step of both layers on the kernel
    assert gen.sequences.shape == (2, T0 + n) and torch.equal(gen.sequences[:, :T0], ids)
    assert torch.equal(gen.lengths, torch.full((2,), n, device="cuda"))
    # unchanged by the decode steps: the pinned block keeps the log-probs of its first forward
    assert torch.equal(bmodel.log_prob_samples()[:, 0], gen.log_prior)
    assert torch.equal(bmodel.log_prob_samples()[:, 1], gen.log_variational_posterior)
    # sample_bayesian's log-probs at the same base (on the prompt, the path the prefill took), bit for bit
    assert torch.equal(lp_ref[:, 0], gen.log_prior) and torch.equal(lp_ref[:, 1], gen.log_variational_posterior)
    # the same base, one forward over the whole sequence without a cache (teacher forcing)
    bf.manual_seed(SEED)
    with torch.no_grad():
        raw, _, _, _ = sample_bayesian(bmodel, {"input_ids": gen.sequences[:, :-1], "use_cache": False}, S)
    pred = mc_predictive(raw[0][:, :, T0 - 1:])
    assert torch.equal(pred.prediction, gen.sequences[:, T0:])
    for ours, ref in ((gen.predictive_entropy, pred.predictive_entropy), (gen.expected_entropy, pred.expected_entropy),
                      (gen.mutual_information, pred.mutual_information)):
        # bf16 activations through two attention paths (cached kernel vs cache-free): 2x the measured difference
        assert (ours - ref).abs().max().item() < 0.05


def test_generate_padded_rows_match_alone_and_eos():
    import bayeformers_amd as bf
    from bayeformers_amd.sampling import sample_generate

    bmodel = _llama(torch.float32)
    ids = _prompt(T=40)
    short = ids[1, 13:]
    mask = torch.ones_like(ids)
    mask[1, :13] = 0
    S, n = 2, 6
    with torch.no_grad():
        bf.manual_seed(SEED)
        both = sample_generate(bmodel, ids, attention_mask=mask, samples=S, max_new_tokens=n)
        bf.manual_seed(SEED)
        alone0 = sample_generate(bmodel, ids[:1], samples=S, max_new_tokens=n)
        bf.manual_seed(SEED)
        alone1 = sample_generate(bmodel, short[None], samples=S, max_new_tokens=n)
    assert torch.equal(both.sequences[0, 40:], alone0.sequences[0, 40:])
    assert torch.equal(both.sequences[1, 40:], alone1.sequences[0, 27:])
    torch.testing.assert_close(both.predictive_entropy[1], alone1.predictive_entropy[0], rtol=1e-4, atol=1e-4)
    # EOS: the token row 0 emits at step 2 ends that row there
    eos = int(alone0.sequences[0, 40 + 2])
    first = (alone0.sequences[0, 40:] == eos).nonzero()[0].item()
    with torch.no_grad():
        bf.manual_seed(SEED)
        g = sample_generate(bmodel, ids[:1], samples=S, max_new_tokens=n, eos_token_id=eos, pad_token_id=7)
    assert int(g.lengths[0]) == first + 1
    assert torch.equal(g.sequences[0, 40:41 + first], alone0.sequences[0, 40:41 + first])
    assert (g.sequences[0, 41 + first:] == 7).all()
    assert (g.predictive_entropy[0, first + 1:] == 0).all() and (g.token_prob[0, first + 1:] == 0).all()
    assert (g.token_prob[0, :first + 1] > 0).all()


def test_generate_do_sample_with_generator_is_reproducible():
    import bayeformers_amd as bf
    from bayeformers_amd.sampling import sample_generate

    bmodel = _llama(torch.bfloat16)
    ids = _prompt()
    outs = []
    for _ in range(2):
        bf.manual_seed(SEED)
        with torch.no_grad():
            outs.append(sample_generate(bmodel, ids, samples=2, max_new_tokens=4, do_sample=True, temperature=0.7,
                                        generator=torch.Generator(device="cuda").manual_seed(3)))
    assert torch.equal(outs[0].sequences, outs[1].sequences)
    assert (outs[0].token_prob > 0).all()


def test_generate_with_device_counter():
    import bayeformers_amd as bf
    from bayeformers_amd.sampling import sample_generate

    bmodel = _llama(torch.bfloat16)
    ids = _prompt()
    bf.manual_seed(SEED)
    with torch.no_grad():
        host = sample_generate(bmodel, ids, samples=2, max_new_tokens=3)
    bf.manual_seed(SEED)
    bf.use_device_counter(True)
    try:
        with torch.no_grad():
            dev = sample_generate(bmodel, ids, samples=2, max_new_tokens=3)
        assert int(bf.random.STATE.device_counter.item()) == 2  # committed once
    finally:
        bf.use_device_counter(False)
    assert torch.equal(host.sequences, dev.sequences) and torch.equal(host.log_prior, dev.log_prior)


def test_generate_matches_reference_fixture(golden_dir):
    """fp32 greedy BMA generation against the reference's to_bayesian model recomputing the whole sequence every step
    (tests/golden/make_golden_generate.py): the same tokens, the statistics within 1e-4."""
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
    bmodel = bf.to_bayesian(LlamaForCausalLM(cfg).eval(), delta=float(g["delta"]), freeze=True).eval()
    assert float(sum(p.detach().double().abs().sum() for p in bmodel.parameters())) == pytest.approx(float(g["checksum"]), rel=1e-6)
    bmodel = bmodel.cuda()
    assert bf.fuse_attention(bmodel)
    bf.set_compute_dtype("fp32")
    bf.manual_seed(SEED)
    try:
        with torch.no_grad():
            gen = sample_generate(bmodel, torch.from_numpy(g["ids"]).cuda(), torch.from_numpy(g["mask"]).cuda(), samples=S,
                                  max_new_tokens=n, temperature=float(g["temperature"]))
    finally:
        bf.set_compute_dtype("bf16")
    assert np.array_equal(gen.sequences[:, T0:].cpu().numpy(), g["tokens"])
    for name in ("predictive_entropy", "expected_entropy", "mutual_information", "token_prob"):
        np.testing.assert_allclose(getattr(gen, name).cpu().numpy(), g[name], rtol=0, atol=1e-4, err_msg=name)
    np.testing.assert_allclose(gen.log_prior.cpu().numpy(), g["log_prior"], rtol=2e-6)
    np.testing.assert_allclose(gen.log_variational_posterior.cpu().numpy(), g["lvp"], rtol=2e-6)


def test_pinned_samples_outside_monte_carlo_is_not_replayed():
    """Eval-mode no_grad forwards of one signature are replayed from a HIP graph from their third call on — but not inside
    pinned_samples(): at S = 1 every forward draws the same weights, and the counter moves once, at the end."""
    import bayeformers_amd as bf
    import bayeformers_amd.nn as bnn

    model = bnn.Model(torch.nn.Sequential(bnn.Linear(256, 256), bnn.Linear(256, 128))).eval().cuda()
    x = torch.randn(200, 256, device="cuda")
    bf.manual_seed(SEED, next_sample=5)
    outs, lps = [], []
    with torch.no_grad(), model.pinned_samples():
        for _ in range(5):
            outs.append(model(x).clone())
            lps.append(model.log_prob_samples().clone())
    assert all(torch.equal(o, outs[0]) for o in outs) and all(torch.equal(l, lps[0]) for l in lps)
    assert bf.random.STATE.next_sample == 6
    bf.manual_seed(SEED, next_sample=5)
    with torch.no_grad():
        assert torch.equal(model(x), outs[0])  # index 5, drawn eagerly


def test_plan_is_not_rebuilt_per_decode_step(monkeypatch):
    """The layers leave the sampling plan for the fused small-M kernel at the first decode step: the plan is built for the
    prefill, dropped once, and no decode step builds another."""
    import bayeformers_amd as bf
    from bayeformers_amd import plan as bplan
    from bayeformers_amd.nn import model as bmodel_mod
    from bayeformers_amd.sampling import sample_generate

    builds = []
    real = bplan.SamplePlan.__init__

    def counting(self, *a, **kw):
        builds.append(1)
        return real(self, *a, **kw)

    monkeypatch.setattr(bmodel_mod.SamplePlan, "__init__", counting)
    bmodel = _llama(torch.bfloat16)
    bf.manual_seed(SEED)
    with torch.no_grad():
        sample_generate(bmodel, _prompt(), samples=2, max_new_tokens=12)
    assert len(builds) == 1, len(builds)


def test_generate_bf16_padded_rows_match_alone():
    """The decode kernel's key-mask path inside sample_generate: a left-padded row gets the tokens it gets alone."""
    import bayeformers_amd as bf
    from bayeformers_amd import ops
    from bayeformers_amd.sampling import sample_generate

    bmodel = _llama(torch.bfloat16)
    ids = _prompt(T=128)
    mask = torch.ones_like(ids)
    mask[1, :7] = 0
    d0 = ops.DECODE_CALLS["fwd"]
    with torch.no_grad():
        bf.manual_seed(SEED)
        both = sample_generate(bmodel, ids, attention_mask=mask, samples=2, max_new_tokens=6)
        assert ops.DECODE_CALLS["fwd"] - d0 == 2 * 5
        bf.manual_seed(SEED)
        alone = sample_generate(bmodel, ids[1:, 7:], samples=2, max_new_tokens=6)
    assert torch.equal(both.sequences[1, 128:], alone.sequences[0, 121:])
