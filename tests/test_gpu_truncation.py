"""bf_probs_truncate (ops.truncate_probs) against the numpy restatement of its contract, its determinism under capture,
its draws through bf_generate_step, and sample_generate's top_k / top_p / min_p end to end."""
import math

import numpy as np
import pytest
import torch

from test_gpu_generate_graph import _equal, _gen, _llama, _prompt, _settle
from truncation_ref import softmax_rows, truncate_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _compute_dtype():
    yield
    import bayeformers_amd as bf

    bf.set_compute_dtype("bf16")  # the fp32 models below switch it


CRITERIA = [dict(top_k=50), dict(top_p=0.9), dict(min_p=0.05), dict(top_k=50, top_p=0.9, min_p=0.05)]


def _rows(R, V, seed):
    """R rows cycling through the kinds the filter must handle: peaked and flat softmax rows, heavy ties (a few
    quantised values), zeros, a one-hot row, a NaN row and an all-zero row."""
    rng = np.random.default_rng(seed)
    rows = []
    for r in range(R):
        kind = (r + seed) % 7
        if kind == 0:
            p = softmax_rows(rng.standard_normal(V) * 6.0)
        elif kind == 1:
            p = softmax_rows(rng.standard_normal(V) * 0.2)
        elif kind == 2:
            q = rng.integers(1, 5, V).astype(np.float64)
            p = (q / q.sum()).astype(np.float32)
        elif kind == 3:
            p = softmax_rows(rng.standard_normal(V) * 2.0)
            p[rng.random(V) < 0.4] = 0.0
        elif kind == 4:
            p = np.zeros(V, np.float32)
            p[rng.integers(V)] = 1.0
        elif kind == 5:
            p = softmax_rows(rng.standard_normal(V))
            p[rng.integers(V)] = np.nan
        else:
            p = np.zeros(V, np.float32)
        rows.append(p)
    return np.stack(rows)


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("V", [7, 1000, 32000, 128256, 151936, 524288])
@pytest.mark.parametrize("R", [1, 5, 64])
def test_kept_set_matches_the_restatement(R, V):
    from bayeformers_amd import ops

    probs = _rows(R, V, seed=R + V)
    d = torch.from_numpy(probs).cuda()
    for kw in CRITERIA:
        kw = dict(kw, top_k=min(kw["top_k"], max(1, V // 2))) if "top_k" in kw else kw
        out = ops.truncate_probs(d, **kw)
        ref = torch.from_numpy(truncate_ref(probs, **kw)).cuda()
        assert torch.equal(_bits(out), _bits(ref)), (kw, (_bits(out) != _bits(ref)).sum().item())
    # in place (out = probs) is the same launch
    kw = dict(top_k=min(50, max(1, V // 2)), top_p=0.9, min_p=0.05)
    inplace = d.clone()
    ops.truncate_probs(inplace, **kw, out=inplace)
    assert torch.equal(_bits(inplace), _bits(ops.truncate_probs(d, **kw)))


@pytest.mark.parametrize("V", [7, 1001, 151936])
def test_launches_are_bitwise_equal_and_replay_under_capture(V):
    from bayeformers_amd import ops

    d = torch.from_numpy(_rows(16, V, seed=V)).cuda()
    kw = dict(top_k=min(50, V - 1), top_p=0.9, min_p=0.02)
    a, b = ops.truncate_probs(d, **kw), ops.truncate_probs(d, **kw)
    assert torch.equal(_bits(a), _bits(b))
    out = torch.empty_like(d)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.truncate_probs(d, **kw, out=out)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.truncate_probs(d, **kw, out=out)
    out.zero_()
    calls = ops.TRUNCATE_CALLS[0]
    g.replay()
    torch.cuda.synchronize()
    assert ops.TRUNCATE_CALLS[0] == calls and torch.equal(_bits(out), _bits(a))


def _draw(probs, seed):
    """The token of one sampled bf_generate_step launch per row of probs [R, V]."""
    from bayeformers_amd import ops

    R = probs.shape[0]
    dev = probs.device
    zero = torch.zeros(R, device=dev)
    seq = torch.zeros(R, 1, dtype=torch.long, device=dev)
    ops.generate_step(probs, zero, zero, zero, 1, torch.zeros(2, dtype=torch.long, device=dev), seq, 0,
                      torch.zeros(4, R, 1, device=dev), None, torch.zeros(R, dtype=torch.long, device=dev),
                      torch.zeros(R, dtype=torch.long, device=dev), None, None, 0,
                      torch.tensor([seed], dtype=torch.long, device=dev))
    return seq[:, 0]


@pytest.mark.parametrize("V,kw", [(2000, dict(top_k=40)), (2500, dict(top_p=0.8)),
                                  (3000, dict(top_k=200, top_p=0.9, min_p=0.05))])
def test_filtered_draws_pass_chi_square(V, kw):
    """60000 draws from one filtered row: the frequencies against the renormalised kept distribution; nothing outside it."""
    from bayeformers_amd import ops

    p = torch.from_numpy(softmax_rows(np.random.default_rng(V).standard_normal(V) * 1.5)).cuda()
    R = 60000
    filtered = ops.truncate_probs(p[None, :].repeat(R, 1), **kw)
    keep = filtered[0] > 0
    assert 1 < int(keep.sum()) < V
    toks = _draw(filtered, 0xC0FFEE)
    counts = torch.bincount(toks, minlength=V).double()
    assert counts[~keep].sum() == 0
    q = filtered[0].double()[keep]
    expected = q / q.sum() * R
    chi2 = float(((counts[keep] - expected) ** 2 / expected).sum())
    df = int(keep.sum()) - 1
    bound = df + 4.0 * math.sqrt(2.0 * df)  # ~ the 0.9999 quantile (fixed seed: the test is deterministic)
    assert chi2 < bound, (chi2, bound)


# ---- sample_generate end to end (the tiny Llama of the generate tests) -----------------------------------------------
@pytest.mark.parametrize("path", ["eager", "static", "graph"])
def test_top_k_1_is_greedy(path):
    bmodel = _llama(torch.float32)
    ids, mask = _prompt(pad=5)
    kw = dict(max_new_tokens=12, static_cache=path == "static", graph=path == "graph")
    _settle(bmodel, ids, mask)
    greedy = _gen(bmodel, ids, mask, **kw)
    top1 = _gen(bmodel, ids, mask, do_sample=True, top_k=1, gen_seed=3, **kw)
    assert _equal(greedy, top1)


def test_graph_equals_static_with_all_three():
    from bayeformers_amd import ops

    bmodel = _llama(torch.bfloat16)
    ids, mask = _prompt(pad=9)
    kw = dict(max_new_tokens=20, do_sample=True, temperature=0.8, top_k=50, top_p=0.9, min_p=0.05, gen_seed=5)
    _settle(bmodel, ids, mask)
    calls = ops.TRUNCATE_CALLS[0]
    static = _gen(bmodel, ids, mask, static_cache=True, **kw)
    assert ops.TRUNCATE_CALLS[0] - calls == 20
    graph = _gen(bmodel, ids, mask, graph=True, **kw)
    assert _equal(static, graph) and (graph.token_prob > 0).all()


@pytest.mark.parametrize("path", ["eager", "graph"])
def test_top_k_tokens_are_in_the_teacher_forced_top_k(path):
    import bayeformers_amd as bf
    from bayeformers_amd.sampling import mc_predictive, sample_bayesian

    from test_gpu_generate_graph import SEED

    bmodel = _llama(torch.float32)
    ids, _ = _prompt()
    k, n, S, T0 = 4, 10, 3, ids.shape[1]
    _settle(bmodel, ids, None)
    gen = _gen(bmodel, ids, None, max_new_tokens=n, do_sample=True, top_k=k, gen_seed=7, graph=path == "graph")
    bf.manual_seed(SEED)
    with torch.no_grad():
        raw, _, _, _ = sample_bayesian(bmodel, {"input_ids": gen.sequences[:, :-1], "use_cache": False}, S)
    probs = mc_predictive(raw[0][:, :, T0 - 1:]).probs  # [B, n, V]
    tok = gen.sequences[:, T0:]
    p_tok = probs.gather(-1, tok[..., None])[..., 0]
    kth = probs.topk(k, dim=-1).values[..., -1]
    assert (p_tok >= kth * (1 - 1e-4)).all()
    torch.testing.assert_close(gen.token_prob, p_tok, rtol=1e-4, atol=1e-6)
    assert not torch.equal(tok, probs.argmax(-1))  # it did sample


@pytest.mark.parametrize("path", ["eager", "graph"])
def test_no_op_settings_launch_nothing(path):
    from bayeformers_amd import ops

    bmodel = _llama(torch.bfloat16)
    ids, mask = _prompt(pad=4)
    kw = dict(max_new_tokens=8, do_sample=True, gen_seed=9, graph=path == "graph")
    _settle(bmodel, ids, mask)
    plain = _gen(bmodel, ids, mask, **kw)
    calls = ops.TRUNCATE_CALLS[0]
    for noop in (dict(top_k=512), dict(top_k=10 ** 6), dict(top_p=1.0), dict(min_p=0.0),
                 dict(top_k=512, top_p=1.0, min_p=0.0)):
        assert _equal(plain, _gen(bmodel, ids, mask, **noop, **kw)), noop
    assert ops.TRUNCATE_CALLS[0] == calls


def test_graph_replays_add_no_launches():
    from bayeformers_amd import ops

    bmodel = _llama(torch.bfloat16)
    ids, mask = _prompt(pad=4)
    _settle(bmodel, ids, mask)
    counts = []
    for n in (6, 30):
        t, e = ops.TRUNCATE_CALLS[0], ops.GENERATE_CALLS[0]
        _gen(bmodel, ids, mask, max_new_tokens=n, graph=True, do_sample=True, top_k=50, top_p=0.9, gen_seed=1)
        counts.append((ops.TRUNCATE_CALLS[0] - t, ops.GENERATE_CALLS[0] - e))
    assert counts[0] == counts[1] == (3, 3), counts
