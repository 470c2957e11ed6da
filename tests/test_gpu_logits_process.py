"""bf_logits_process (ops.process_logits) against transformers' processor chain bit for bit, its replay under capture
at a device step, and sample_generate's repetition_penalty / no_repeat_ngram_size / min_new_tokens end to end."""
import numpy as np
import pytest
import torch

from logits_process_ref import process_hf, process_ref
from test_gpu_generate_graph import SEED, _equal, _gen, _llama, _prompt, _settle

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _compute_dtype():
    yield
    import bayeformers_amd as bf

    bf.set_compute_dtype("bf16")  # the fp32 models below switch it


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _history(B, L, V, seed):
    """[B, L + 4] histories with many repeats: ids from a small pool, a run of one id, a left-padded row."""
    g = torch.Generator().manual_seed(seed)
    pool = torch.randint(0, V, (min(V, 6),), generator=g)
    seq = pool[torch.randint(0, len(pool), (B, L + 4), generator=g)]
    seq[0, 3:7] = pool[0]
    if B > 1:
        seq[1, :3] = 0
    return seq


@pytest.mark.parametrize("V", [7, 1000, 32000, 128256, 151936])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "fp16", "fp32"])
def test_kernel_matches_transformers_chain_bitwise(V, dtype):
    from bayeformers_amd import ops

    S, B, T0 = 2, 3, 9
    g = torch.Generator().manual_seed(V)
    full = (torch.randn(S * B, 3, V + 8, generator=g) * 3).to(dtype)
    dfull = full.cuda()
    seq = _history(B, T0 + 6, V, V)
    dseq = seq.cuda()
    cases = [(theta, n, T) for theta in (0.5, 1.3) for n in (0, 1, 2, 3, 4) for T in (1.0, 0.7)]
    for i, (theta, n, T) in enumerate(cases):
        step = i % 7
        m, eos = (step + i % 2, int(seq[0, 0])) if i % 3 else (0, None)
        # contiguous rows, strided rows (the prefill's out.logits[:, -1, :]) and rows off 16-byte alignment
        for sl in (None, (-1, 0), (1, 1)):
            dev = dfull[:, 0, :V].contiguous() if sl is None else dfull[:, sl[0], sl[1]:sl[1] + V]
            out = ops.process_logits(dev, dseq, T0, step, S, theta, n, m, eos, T)
            hf = process_hf(dev.cpu(), seq, T0, step, S, theta, n, m, eos, T)
            assert np.array_equal(_bits(out.cpu().numpy()), _bits(hf)), (theta, n, T, step, m)


def test_kernel_ids_out_of_range_and_the_all_banned_row():
    from bayeformers_amd import ops
    from bayeformers_amd.sampling import mc_predictive

    S, B, V, T0 = 2, 2, 7, 8
    logits = torch.randn(S * B, V).cuda()
    seq = torch.tensor([[0, 1, 2, 3, 4, 5, 6, 0], [-3, 9, 7, 2, 1 << 40, 2, -1, 2]])
    out = ops.process_logits(logits, seq.cuda(), T0, 0, S, 1.5, 1)
    ref = process_ref(logits, seq, T0, 0, S, 1.5, 1)
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(ref))
    assert torch.isneginf(out[0::B]).all() and torch.isfinite(out[1::B, [0, 3, 4, 5, 6]]).all()
    pred = mc_predictive(out.view(S, B, V))
    assert (pred.probs[0] == 0).all() and pred.prediction[0].item() == 0 and torch.isfinite(pred.probs).all()


def test_one_captured_launch_follows_the_device_step():
    from bayeformers_amd import ops

    S, B, V, T0, n = 3, 2, 32000, 16, 12
    logits = torch.randn(S * B, V, device="cuda").to(torch.bfloat16)
    seq = _history(B, T0 + n, V, 3).cuda()
    kw = dict(repetition_penalty=1.3, no_repeat_ngram_size=3, min_new_tokens=5, eos_token_id=int(seq[0, 1]),
              temperature=0.7)
    state = torch.zeros(2, dtype=torch.long, device="cuda")
    out = torch.empty(S * B, V, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.process_logits(logits, seq, T0, state, S, out=out, **kw)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.process_logits(logits, seq, T0, state, S, out=out, **kw)
    calls = ops.PROCESS_CALLS[0]
    for t in range(n):
        state[0] = t
        out.zero_()
        g.replay()
        eager = ops.process_logits(logits, seq, T0, t, S, **kw)
        assert torch.equal(out.view(torch.int32), eager.view(torch.int32)), t
    assert ops.PROCESS_CALLS[0] - calls == n  # the eager launches only


# ---- sample_generate end to end (the tiny Llama of the generate tests) -----------------------------------------------
PROC = dict(repetition_penalty=1.3, no_repeat_ngram_size=3)


def _ngram_repeats(row, n):
    grams = [tuple(row[i:i + n]) for i in range(len(row) - n + 1)]
    return len(grams) - len(set(grams))


def test_greedy_matches_teacher_forced_processors():
    import bayeformers_amd as bf
    from bayeformers_amd.sampling import mc_predictive, sample_bayesian

    bmodel = _llama(torch.float32)
    ids, _ = _prompt()
    S, n, T0 = 3, 10, ids.shape[1]
    _settle(bmodel, ids, None)
    eos = int(_gen(bmodel, ids, None, max_new_tokens=1).sequences[0, T0])  # greedy's first token of row 0
    kw = dict(PROC, min_new_tokens=n, eos_token_id=eos)
    gen = _gen(bmodel, ids, None, max_new_tokens=n, **kw)
    assert gen.sequences[0, T0].item() != eos and torch.equal(gen.lengths, torch.full((2,), n, device="cuda"))
    bf.manual_seed(SEED)
    with torch.no_grad():
        raw, _, _, _ = sample_bayesian(bmodel, {"input_ids": gen.sequences[:, :-1], "use_cache": False}, S)
    logits = raw[0][:, :, T0 - 1:]  # [S, B, n, V]
    plain = mc_predictive(logits)
    seq = gen.sequences.cpu()
    for t in range(n):
        lt = logits[:, :, t].reshape(S * 2, -1).cpu()
        processed = torch.from_numpy(process_hf(lt, seq, T0, t, S, 1.3, 3, n, eos)).cuda()
        tok = mc_predictive(processed.view(S, 2, -1)).prediction
        assert torch.equal(tok, gen.sequences[:, T0 + t]), t
    for ours, ref in ((gen.predictive_entropy, plain.predictive_entropy), (gen.expected_entropy, plain.expected_entropy),
                      (gen.mutual_information, plain.mutual_information)):
        assert (ours - ref).abs().max().item() < 0.05
    p_tok = plain.probs.gather(-1, gen.sequences[:, T0:, None])[..., 0]
    torch.testing.assert_close(gen.token_prob, p_tok, rtol=1e-3, atol=1e-5)
    assert not torch.equal(gen.sequences[:, T0:], plain.prediction)  # the processors changed the text


@pytest.mark.parametrize("path", ["eager", "graph"])
@pytest.mark.parametrize("n", [2, 3])
def test_no_repeat_ngram_holds_where_greedy_repeats(path, n):
    """A repetition_penalty below 1 draws greedy decoding back to the tokens it has seen: the control repeats an n-gram;
    with no_repeat_ngram_size=n no n-gram occurs twice in any row, prompt included."""
    bmodel = _llama(torch.bfloat16)
    g = torch.Generator().manual_seed(n)
    ids = torch.stack([torch.randperm(512, generator=g)[:32] for _ in range(2)]).cuda()  # no n-gram repeats in it
    kw = dict(max_new_tokens=48, repetition_penalty=0.5, graph=path == "graph")
    _settle(bmodel, ids, None)
    control = _gen(bmodel, ids, None, **kw)
    assert all(_ngram_repeats(row, n) > 0 for row in control.sequences.tolist())
    banned = _gen(bmodel, ids, None, no_repeat_ngram_size=n, **kw)
    assert all(_ngram_repeats(row, n) == 0 for row in banned.sequences.tolist())


@pytest.mark.parametrize("path", ["eager", "static", "graph"])
def test_min_new_tokens_keeps_rows_going(path):
    bmodel = _llama(torch.float32)
    ids, mask = _prompt(pad=5)
    T0, n, m = ids.shape[1], 16, 6
    kw = dict(max_new_tokens=n, static_cache=path == "static", graph=path == "graph")
    _settle(bmodel, ids, mask)
    eos = int(_gen(bmodel, ids, mask, **kw).sequences[0, T0])
    control = _gen(bmodel, ids, mask, eos_token_id=eos, **kw)
    assert control.lengths[0].item() == 1
    gen = _gen(bmodel, ids, mask, eos_token_id=eos, min_new_tokens=m, **kw)
    new = gen.sequences[:, T0:]
    assert (gen.lengths > m).all() and not (new[:, :m] == eos).any()  # banned at steps 0 .. m - 1
    for b in range(2):
        hit = (new[b] == eos).nonzero()
        L = int(hit[0]) + 1 if len(hit) else n
        assert gen.lengths[b].item() == L and (new[b, L:] == eos).all()  # pad defaults to eos
    if path == "graph":  # eager steps until the ban lifts, then a captured step without the launch
        assert _equal(gen, _gen(bmodel, ids, mask, eos_token_id=eos, min_new_tokens=m, max_new_tokens=n,
                                static_cache=True))


@pytest.mark.parametrize("do_sample,trunc", [(False, {}), (True, {}), (True, dict(top_k=50, top_p=0.9))],
                         ids=["greedy", "sample", "sample-topk-topp"])
@pytest.mark.parametrize("keep", [False, True], ids=["draw", "keep"])
def test_graph_equals_static(do_sample, trunc, keep):
    from bayeformers_amd import ops

    bmodel = _llama(torch.bfloat16)
    ids, mask = _prompt(pad=9)
    n = 20
    kw = dict(PROC, min_new_tokens=4, eos_token_id=7, max_new_tokens=n, do_sample=do_sample, temperature=0.8,
              keep_weights=keep, gen_seed=5 if do_sample else None, **trunc)
    _settle(bmodel, ids, mask)
    calls = ops.PROCESS_CALLS[0]
    static = _gen(bmodel, ids, mask, static_cache=True, **kw)
    assert ops.PROCESS_CALLS[0] - calls == int(static.lengths.max())
    graph = _gen(bmodel, ids, mask, graph=True, **kw)
    assert _equal(static, graph) and (graph.token_prob > 0).all()
    plain = _gen(bmodel, ids, mask, graph=True, **dict(kw, repetition_penalty=None, no_repeat_ngram_size=None,
                                                       min_new_tokens=None))
    assert not torch.equal(plain.sequences, graph.sequences)


@pytest.mark.parametrize("path", ["eager", "graph"])
def test_no_op_settings_launch_nothing(path):
    from bayeformers_amd import ops

    bmodel = _llama(torch.bfloat16)
    ids, mask = _prompt(pad=4)
    kw = dict(max_new_tokens=8, eos_token_id=3, graph=path == "graph")
    _settle(bmodel, ids, mask)
    for extra in (dict(), dict(do_sample=True, gen_seed=9)):
        plain = _gen(bmodel, ids, mask, **kw, **extra)
        calls = ops.PROCESS_CALLS[0]
        for noop in (dict(repetition_penalty=1.0), dict(no_repeat_ngram_size=0), dict(min_new_tokens=0),
                     dict(repetition_penalty=None, no_repeat_ngram_size=None, min_new_tokens=None),
                     dict(repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0)):
            assert _equal(plain, _gen(bmodel, ids, mask, **noop, **kw, **extra)), noop
        assert ops.PROCESS_CALLS[0] == calls


def test_graph_replays_add_no_launches():
    from bayeformers_amd import ops

    bmodel = _llama(torch.bfloat16)
    ids, mask = _prompt(pad=4)
    _settle(bmodel, ids, mask)
    counts = []
    for n in (6, 30):
        p, e = ops.PROCESS_CALLS[0], ops.GENERATE_CALLS[0]
        _gen(bmodel, ids, mask, max_new_tokens=n, graph=True, **PROC)
        counts.append((ops.PROCESS_CALLS[0] - p, ops.GENERATE_CALLS[0] - e))
    assert counts[0] == counts[1] == (3, 3), counts
