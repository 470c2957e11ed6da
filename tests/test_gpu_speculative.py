"""sample_generate(speculative=γ) on the GPU: bf_spec_accept against tests/speculative_ref.py, Model.posterior_mean(), and
the generation end to end — greedy exactness against a teacher-forced forward under the same pinned draws, agreement with
the one-token loop, the acceptance boundary cases, a collapsed posterior, eager against graph and the FP8 cache."""
import functools
import math

import pytest
import torch

import speculative_ref as ref

pytestmark = pytest.mark.gpu

SEED = 0x5EED
S, B, T0, N = 3, 2, 11, 13
VOCAB = 512
# A random-initialised head gives near-uniform rows (top-two gaps of 1e-5: every token a tie).  Its weight times 8 gives
# logits of standard deviation ~4, a predictive peaked like a trained model's, on which "the argmax" means something.
HEAD_GAIN = 8.0

# The exactness bounds.  Speculation and the one-token loop are two 16-bit routes of one function (other GEMM row counts, γ + 1
# queries through the decode kernels), so neither is bitwise a teacher-forced forward.  MEASURED holds the largest gaps of the
# EXISTING graph=True generation (no speculation: the code as it was) against that forward, at every generated position of
# the shapes and models these tests use (Llama-style seeds 0 and AGREEMENT_SEEDS, Mistral-style seed 0; MI355X, see
# profiles/speculative_decoding.md), kept apart by unit so that neither bound is wider than one bound for all would be:
#   "p": differences of probabilities — max probability − the emitted token's, and |token_prob − teacher-forced|;
#   "h": differences of entropies in nats — predictive, expected, mutual information.
# Each bound is twice the measured gap: the extra route.  The FP8 cache has its own (its prompt is attended in bf16 and
# handed over, the teacher-forced pass reads every row dequantised).
MEASURED = {"bf16": {"p": 5.30e-3, "h": 3.07e-2}, "kv8": {"p": 2.08e-2, "h": 6.95e-2}}
TOL = {k: {u: 2.0 * v for u, v in m.items()} for k, m in MEASURED.items()}
# Model seeds of the agreement test.  Scanned on the MI355X (seeds 24 .. 223; 14 have every gap at 1.2e-2 or more): four whose one-token graph=True run has
# every teacher-forced top-two gap at least 1.8e-2, above TOL["bf16"]["p"] = 1.06e-2, so that all 13 positions are compared — and for which
# the existing static-against-dynamic comparison (graph=True against the default path) gives the same text under the same rule.
AGREEMENT_SEEDS = (31, 51, 74, 139)
CLEAR_SEED = 139  # the widest of them (every top-two gap at least 3.1e-2): the model of the tests that compare texts exactly


# ---- bf_spec_accept against the reference ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ref.hand_cases()))
def test_accept_kernel_matches_the_reference(name):
    from bayeformers_amd import ops

    args0, _ = ref.hand_cases()[name]
    want, got = ref.clone_args(args0), ref.clone_args(args0, "cuda")
    ref.speculative_accept(**want)
    ops.speculative_accept(**got)
    torch.cuda.synchronize()
    for k, v in want.items():
        if isinstance(v, torch.Tensor):
            assert torch.equal(got[k].cpu(), v), (name, k)  # integers equal; statistics bitwise: copies and gathers


def test_accept_kernel_replays_from_a_graph():
    """One captured launch follows the device step: replayed until the n tokens are out, it equals the reference run as
    often, and past n it only rewinds."""
    from bayeformers_amd import ops

    args0, _ = ref.hand_cases()["minimum_rules"]
    want, got = ref.clone_args(args0), ref.clone_args(args0, "cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.speculative_accept(**ref.clone_args(args0, "cuda"))  # (warm-up on scratch copies)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.speculative_accept(**got)
    for _ in range(6):
        g.replay()
        ref.speculative_accept(**want)
    torch.cuda.synchronize()
    assert int(want["state"][0]) == ref.N_NEW and int(want["rewind"][0]) == ref.G + 1
    for k, v in want.items():
        if isinstance(v, torch.Tensor):
            assert torch.equal(got[k].cpu(), v), k


# ---- models ------------------------------------------------------------------------------------------------------------
def _to_bf16(bmodel):
    freqs = {n: b.detach().clone() for n, b in bmodel.named_buffers() if "inv_freq" in n}
    bmodel = bmodel.to(torch.bfloat16)
    for n, b in freqs.items():
        setattr(bmodel.get_submodule(n.rsplit(".", 1)[0]), n.rsplit(".", 1)[1], b)
    return bmodel


def _plain(family, seed):
    """The frequentist model (test_gpu_generate_graph's Llama shapes, test_gpu_kv8's Mistral shapes with W = 8)."""
    from transformers import AutoConfig, AutoModelForCausalLM

    if family == "llama":
        kw = dict(hidden_size=512, num_attention_heads=8, num_key_value_heads=2, intermediate_size=1024)
    else:
        kw = dict(hidden_size=256, num_attention_heads=4, num_key_value_heads=2, head_dim=64, intermediate_size=512,
                  sliding_window=8)
    cfg = AutoConfig.for_model(family, num_hidden_layers=2, vocab_size=VOCAB, max_position_embeddings=512,
                               tie_word_embeddings=False, attention_dropout=0.0, attn_implementation="sdpa", **kw)
    torch.manual_seed(seed)
    model = AutoModelForCausalLM.from_config(cfg).eval()
    with torch.no_grad():
        model.lm_head.weight.mul_(HEAD_GAIN)
    return model


@functools.lru_cache(maxsize=None)
def _model(family="llama", seed=0):
    import bayeformers_amd as bf

    bf.set_compute_dtype("bf16")
    bmodel = _to_bf16(bf.to_bayesian(_plain(family, seed), delta=0.05, freeze=True).eval().cuda())
    assert bf.fuse_attention(bmodel)
    return bmodel


def _prompt(b=B, t=T0, pad=3):
    ids = torch.randint(0, VOCAB, (b, t), generator=torch.Generator().manual_seed(11)).cuda()
    mask = torch.ones_like(ids)
    mask[b - 1, :pad] = 0  # one left-padded row
    return ids, mask


def _generate(model, ids, mask, n=N, **kw):
    import bayeformers_amd as bf
    from bayeformers_amd.sampling import sample_generate

    bf.manual_seed(SEED)
    kw.setdefault("keep_weights", True)
    with torch.no_grad():
        return sample_generate(model, ids, attention_mask=mask, samples=S, max_new_tokens=n, **kw)


def _teacher(model, gen, mask, n=N, kv8=False, monkeypatch=None):
    """The predictive of every generated position from ONE ordinary forward over gen.sequences under the same pinned draws
    (kv8: against a static cache whose layers store the dequantised e4m3 rows, test_gpu_kv8's oracle layer)."""
    import bayeformers_amd as bf
    from bayeformers_amd import sampling
    from bayeformers_amd.sampling import mc_predictive

    seq = gen.sequences[:, :-1]
    t0 = seq.shape[1] - (n - 1)
    full = torch.cat([mask, mask.new_ones((mask.shape[0], n - 1))], 1)
    pos = (full.cumsum(-1) - 1).clamp(min=0)
    kw = dict(use_cache=False)
    if kv8:
        from test_gpu_kv8 import _oracle_layer

        with monkeypatch.context() as mp:
            mp.setattr(sampling, "_STATIC_LAYER_HOOK", _oracle_layer())
            kw = dict(use_cache=True, past_key_values=sampling._static_cache(model, seq.shape[1]))
    bf.manual_seed(SEED)
    with torch.no_grad(), model.monte_carlo(S), model.pinned_samples():
        out = model(input_ids=seq.repeat(S, 1), attention_mask=full.repeat(S, 1), position_ids=pos.repeat(S, 1), **kw)
    logits = out.logits[:, t0 - 1:].reshape(S, seq.shape[0], n, -1)
    return mc_predictive(logits)


def _gaps(gen, pred, n=N):
    """(greedy gap, token_prob gap, entropy gap, top-two gap [B, n]) of a generation against its teacher-forced predictive,
    over the positions a row generated (its EOS included).  The first two are differences of probabilities, the third of
    entropies in nats."""
    t0 = gen.sequences.shape[1] - n
    toks = gen.sequences[:, t0:]
    live = torch.arange(n, device=toks.device)[None, :] < gen.lengths[:, None]
    p_tok = pred.probs.gather(-1, toks.clamp(0, pred.probs.shape[-1] - 1)[..., None]).squeeze(-1)
    top2 = pred.probs.topk(2, -1).values
    greedy = ((top2[..., 0] - p_tok) * live).max().item()
    prob = ((gen.token_prob - p_tok).abs() * live).max().item()
    entropy = max(((a - b).abs() * live).max().item()
                  for a, b in ((gen.predictive_entropy, pred.predictive_entropy),
                               (gen.expected_entropy, pred.expected_entropy), (gen.mutual_information, pred.mutual_information)))
    return greedy, prob, entropy, top2[..., 0] - top2[..., 1]


# ---- posterior_mean() --------------------------------------------------------------------------------------------------
def test_posterior_mean_is_the_plain_model_on_mu():
    """Logits of a forward inside posterior_mean() against the frequentist nn.Module carrying μ cast to bf16 (MOPED: μ is
    the pretrained weight), on the framework's ops.  Bound: DESIGN §5's 16-bit GEMM tolerance 2^-7 ‖x‖ ‖W‖ at the head."""
    from bayeformers_amd import ops

    model = _model("llama", 0)
    plain = _plain("llama", 0).cuda().to(torch.bfloat16)
    ids, mask = _prompt()
    pos = (mask.cumsum(-1) - 1).clamp(min=0)
    with torch.no_grad():
        want = plain(input_ids=ids, attention_mask=mask, position_ids=pos, use_cache=False, output_hidden_states=True)
        k0 = ops.SKINNY_CALLS[0]
        with model.posterior_mean():
            got = model(input_ids=ids, attention_mask=mask, position_ids=pos, use_cache=False).logits
            assert ops.SKINNY_CALLS[0] == k0  # 22 rows: the tiled GEMM
            few = model(input_ids=ids[:1, -4:], use_cache=False).logits
            assert ops.SKINNY_CALLS[0] > k0  # 4 rows: bf_gemm_nt_skinny with S = 1
    assert got.shape == want.logits.shape and few.shape == (1, 4, VOCAB)
    bound = 2.0 ** -7 * want.hidden_states[-1].float().norm(dim=-1).max().item() \
        * plain.lm_head.weight.float().norm(dim=-1).max().item()
    err = (got.float() - want.logits.float())[mask.bool()].abs().max().item()
    print(f"[posterior_mean] max |logit - plain| {err:.3e}, bound {bound:.3e}, largest logit {want.logits.abs().max().item():.3f}")
    assert err < bound
    with torch.no_grad():
        want_few = plain(input_ids=ids[:1, -4:], use_cache=False).logits
    assert (few.float() - want_few.float()).abs().max().item() < bound


@pytest.mark.parametrize("keep", [False, True, "fp8"], ids=["draw", "keep", "keep_fp8"])
def test_posterior_mean_nests_inside_pinned_samples(keep):
    """A mean forward between two sampled forwards of one pinned block: the second is bitwise what it is without it, and
    the log-probs and the sample counter do not move."""
    import bayeformers_amd as bf
    from bayeformers_amd import random as bfr

    model = _model("llama", 0)
    ids, _ = _prompt()
    x = ids.repeat(S, 1)

    def run(with_mean):
        bf.manual_seed(SEED)
        with torch.no_grad(), model.monte_carlo(S), model.pinned_samples(keep_weights=keep):
            first = model(input_ids=x, use_cache=False).logits.clone()
            lp = model.log_prob_samples().clone()
            if with_mean:
                before = bfr.get_state()
                with model.posterior_mean():
                    mean = model(input_ids=ids, use_cache=False).logits
                    assert bfr.STATE.mean is not None
                assert bfr.STATE.mean is None and bfr.get_state() == before and mean.shape[0] == B
                assert torch.equal(model.log_prob_samples(), lp)
            second = model(input_ids=x[:, -3:], use_cache=False).logits.clone()
            return first, second, model.log_prob_samples().clone(), bfr.get_state()

    a, b = run(False), run(True)
    for u, v in zip(a[:3], b[:3]):
        assert torch.equal(u, v)
    assert a[3] == b[3]


# ---- greedy exactness --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["llama", "mistral"])
@pytest.mark.parametrize("gamma", [1, 3, 7])
def test_speculative_text_is_the_greedy_text_of_the_posterior(family, gamma):
    """Teacher-force the returned sequences through one ordinary forward under the same pinned draws: at every generated
    position the emitted token's model-average probability is within TOL's "p" of the row's maximum, token_prob within
    "p" and the three entropies within "h" of the teacher-forced ones.  γ = 7 verifies 16 rows per sample; Mistral's window of 8 is
    crossed inside a span.  Measured (MI355X, every γ, both families): greedy gap 0,
    token_prob and entropy gaps those of the one-token loop to every printed digit — MEASURED above — because the largest gap
    is the prefill's first token, which both share; profiles/speculative_decoding.md."""
    from bayeformers_amd import ops

    model = _model(family, 0)
    ids, mask = _prompt()
    c0 = ops.SPEC_ACCEPT_CALLS[0]
    gen = _generate(model, ids, mask, speculative=gamma)
    assert ops.SPEC_ACCEPT_CALLS[0] > c0
    assert gen.sequences.shape == (B, T0 + N) and bool((gen.lengths == N).all())
    verify, proposed, accepted = gen.speculation.tolist()
    assert 0 <= accepted <= proposed <= gamma * verify and verify + accepted == N - 1
    greedy, prob, entropy, _ = _gaps(gen, _teacher(model, gen, mask))
    tol = TOL["bf16"]
    print(f"[speculative {family} γ={gamma}] greedy gap {greedy:.3e}, token_prob gap {prob:.3e} (bound {tol['p']:.2e}), "
          f"entropy gap {entropy:.3e} (bound {tol['h']:.2e}); verify steps {verify}, accepted {accepted} of {proposed}")
    assert greedy <= tol["p"] and prob <= tol["p"] and entropy <= tol["h"]


def test_speculative_exactness_on_the_fp8_cache(monkeypatch):
    """kv_cache="fp8": the samples' cache holds e4m3 rows (the draft's stays bf16); the teacher-forced pass reads the
    dequantised rows, as test_gpu_kv8's oracle does."""
    from bayeformers_amd import ops

    model = _model("llama", 0)
    ids, mask = _prompt()
    k0 = ops.KV8_CALLS["decode"]
    gen = _generate(model, ids, mask, speculative=3, kv_cache="fp8")
    assert ops.KV8_CALLS["decode"] > k0 and bool((gen.lengths == N).all())
    greedy, prob, entropy, _ = _gaps(gen, _teacher(model, gen, mask, kv8=True, monkeypatch=monkeypatch))
    tol = TOL["kv8"]
    print(f"[speculative kv8 γ=3] greedy gap {greedy:.3e}, token_prob gap {prob:.3e} (bound {tol['p']:.2e}), entropy gap "
          f"{entropy:.3e} (bound {tol['h']:.2e})")
    assert greedy <= tol["p"] and prob <= tol["p"] and entropy <= tol["h"]


def test_speculative_agrees_with_the_one_token_loop():
    """sequences equal graph=True's without speculation up to the first position whose teacher-forced top-two gap (of the
    one-token run) is below TOL["bf16"]["p"] — past it either token is a valid greedy choice.  The compared share of all generated
    positions over AGREEMENT_SEEDS must be at least 90 %: a condition on the test's power, not a measurement."""
    compared = total = 0
    for seed in AGREEMENT_SEEDS:
        model = _model("llama", seed)
        ids, mask = _prompt()
        base = _generate(model, ids, mask, graph=True)
        _, _, _, top2 = _gaps(base, _teacher(model, base, mask))
        close = (top2 < TOL["bf16"]["p"]).any(0)
        first = int(close.nonzero()[0]) if bool(close.any()) else N
        spec = _generate(model, ids, mask, graph=True, speculative=3)
        assert torch.equal(spec.sequences[:, :T0 + first], base.sequences[:, :T0 + first]), seed
        compared, total = compared + first, total + N
        print(f"[speculative agreement] seed {seed}: {first} of {N} positions compared, smallest top-two gap "
              f"{top2.min().item():.3e}")
    assert compared >= 0.9 * total, (compared, total)


# ---- boundary cases, a collapsed posterior, eager against graph -----------------------------------------------------------
def _same(a, b):
    from dataclasses import fields

    return all(torch.equal(getattr(a, f.name), getattr(b, f.name)) for f in fields(a)) \
        and (a.speculation is None) == (b.speculation is None) \
        and (a.speculation is None or torch.equal(a.speculation, b.speculation))


@pytest.mark.parametrize("n", [1, 2, 4])
def test_short_generations(n):
    """n of 1 (no iteration at all), 2 and γ + 1 at γ = 3: lengths, padding and statistics against the one-token loop."""
    model = _model("llama", CLEAR_SEED)
    ids, mask = _prompt()
    base = _generate(model, ids, mask, n=n, graph=True)
    for graph in (False, True):
        spec = _generate(model, ids, mask, n=n, graph=graph, speculative=3)
        assert spec.sequences.shape == (B, T0 + n) and torch.equal(spec.lengths, base.lengths)
        assert torch.equal(spec.sequences, base.sequences)  # (seed 139: every top-two gap is at least 3.1e-2, three times the bound)
        for name in ("predictive_entropy", "expected_entropy", "mutual_information", "token_prob"):
            bound = TOL["bf16"]["p" if name == "token_prob" else "h"]
            assert (getattr(spec, name) - getattr(base, name)).abs().max().item() <= bound, name
        verify, proposed, accepted = spec.speculation.tolist()
        assert verify + accepted == n - 1 and accepted <= proposed <= 3 * verify
        if n == 1:
            assert spec.speculation.tolist() == [0, 0, 0]


def test_eos_inside_an_accepted_span():
    """A collapsed posterior accepts every draft, so the EOS of row 0 falls inside an accepted span: lengths, padding and
    zero statistics as the one-token loop leaves them."""
    model = _collapsed()
    ids, mask = _prompt()
    free = _generate(model, ids, mask, graph=True)
    eos = int(free.sequences[0, T0 + 5])
    first = int((free.sequences[0, T0:] == eos).nonzero()[0])
    base = _generate(model, ids, mask, graph=True, eos_token_id=eos, pad_token_id=7)
    for graph in (False, True):
        spec = _generate(model, ids, mask, graph=graph, speculative=3, eos_token_id=eos, pad_token_id=7)
        assert torch.equal(spec.lengths, base.lengths) and int(spec.lengths[0]) == first + 1
        assert torch.equal(spec.sequences, base.sequences) and bool((spec.sequences[0, T0 + first + 1:] == 7).all())
        for name in ("predictive_entropy", "expected_entropy", "mutual_information", "token_prob"):
            got, want = getattr(spec, name), getattr(base, name)
            bound = TOL["bf16"]["p" if name == "token_prob" else "h"]
            assert bool((got[0, first + 1:] == 0).all()) and (got - want).abs().max().item() <= bound, name


@functools.lru_cache(maxsize=None)
def _collapsed():
    """ρ pushed very negative: every draw is the mean to the last bit of bf16, so the draft is the model average."""
    import bayeformers_amd as bf
    import bayeformers_amd.nn as bnn

    bf.set_compute_dtype("bf16")
    bmodel = _to_bf16(bf.to_bayesian(_plain("llama", CLEAR_SEED), delta=0.05, freeze=True).eval().cuda())
    with torch.no_grad():
        for layer in bmodel.fused_children():
            assert isinstance(layer, bnn.Linear)
            layer.weight.rho.fill_(-30.0)
    assert bf.fuse_attention(bmodel)
    return bmodel


@pytest.mark.parametrize("gamma,n", [(3, 13), (3, 11), (7, 13), (1, 6)])
def test_collapsed_posterior_accepts_every_draft(gamma, n):
    model = _collapsed()
    ids, mask = _prompt()
    gen = _generate(model, ids, mask, n=n, graph=True, speculative=gamma)
    verify, proposed, accepted = gen.speculation.tolist()
    assert accepted == proposed and verify == math.ceil((n - 1) / (gamma + 1)) and verify + accepted == n - 1
    assert torch.equal(gen.sequences, _generate(model, ids, mask, n=n, graph=True).sequences)


@pytest.mark.parametrize("variant", ["llama", "mistral", "kv8", "keep_fp8", "temperature", "prefill_chunk"])
def test_eager_and_graph_are_bitwise_equal(variant):
    kw = {"kv8": dict(kv_cache="fp8"), "keep_fp8": dict(keep_weights="fp8"), "temperature": dict(temperature=0.7),
          "prefill_chunk": dict(prefill_chunk=17)}.get(variant, {})
    model = _model("mistral" if variant == "mistral" else "llama", 0)
    ids, mask = _prompt(t=40, pad=5) if variant == "prefill_chunk" else _prompt()
    eager = _generate(model, ids, mask, speculative=3, **kw)
    graph = _generate(model, ids, mask, speculative=3, graph=True, **kw)
    assert _same(eager, graph) and eager.speculation is not None
    assert bool((graph.lengths == N).all()) and bool((graph.token_prob > 0).all())


def test_none_changes_nothing():
    model = _model("llama", 0)
    ids, mask = _prompt()
    for kw in (dict(), dict(graph=True), dict(static_cache=True, keep_weights=False)):
        a, b = _generate(model, ids, mask, **kw), _generate(model, ids, mask, speculative=None, **kw)
        assert _same(a, b) and b.speculation is None
