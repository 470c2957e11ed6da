"""Monte-Carlo predictive statistics on the GPU (bf_mc_predictive_*): the kernels against a float64 torch restatement of
the same logits, and the model-level paths (sample_predictive, GraphedSampler(predictive=True), two ranks sharing the GPU)
against sample_bayesian and the single-process step."""
import os
import socket
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
SEED = 0x5EED


def restate(raw, labels=None, ignore_index=-100):
    """float64 restatement: raw [S, R, C], labels [R]."""
    l = raw.double()
    lse = torch.logsumexp(l, -1, keepdim=True)
    p = torch.exp(l - lse)
    H = -torch.where(p > 0, p * (l - lse), torch.zeros_like(p)).sum(-1)
    probs = p.mean(0)
    pe = -torch.where(probs > 0, probs * probs.log(), torch.zeros_like(probs)).sum(-1)
    ee = H.mean(0)
    out = {"probs": probs, "predictive_entropy": pe, "expected_entropy": ee, "mutual_information": (pe - ee).clamp_min(0)}
    if labels is not None:
        C = raw.shape[-1]
        y = labels.long()
        in_range = (y >= 0) & (y < C)
        valid = (y != ignore_index) & in_range
        yc = torch.where(valid, y, torch.zeros_like(y))
        arg = torch.argmax(raw, -1)  # the raw logits, as the reference's loop
        counts = ((arg == yc) & valid).sum(-1)
        py = p.gather(-1, yc.view(1, -1, 1).expand(p.shape[0], -1, 1)).squeeze(-1).mean(0)
        ll = torch.where(valid, py.log(), torch.full_like(py, float("nan")))
        out.update(correct_per_sample=counts, acc_std=float(np.std(counts.cpu().numpy())), log_likelihood=ll,
                   nll=-ll[valid].mean(), valid=valid, invalid=int(((y != ignore_index) & ~in_range).sum()), yc=yc)
    return out


def check(got, want, raw, labels, C):
    tol = 1e-5 if C <= 1024 else 1e-4
    assert torch.isfinite(got.probs).all() and torch.isfinite(got.predictive_entropy).all()
    assert torch.isfinite(got.expected_entropy).all() and torch.isfinite(got.mutual_information).all()
    np.testing.assert_allclose(got.probs.double().cpu().reshape(want["probs"].shape), want["probs"].cpu(), rtol=0, atol=2e-6)
    for k in ("predictive_entropy", "expected_entropy", "mutual_information"):
        np.testing.assert_allclose(getattr(got, k).double().cpu().reshape(-1), want[k].cpu(), rtol=tol, atol=tol, err_msg=k)
    # prediction: the float64 argmax, except where the top two float64 means are closer than 1e-6
    pred = got.prediction.cpu().reshape(-1)
    top2 = want["probs"].topk(min(2, C), -1).values.cpu()
    close = (top2[:, 0] - top2[:, -1] < 1e-6) if C > 1 else torch.zeros(len(pred), dtype=torch.bool)
    wanted = want["probs"].argmax(-1).cpu()
    assert torch.equal(pred[~close], wanted[~close])
    if labels is None:
        assert got.acc_std is None and got.correct_per_sample is None
        return
    assert torch.equal(got.correct_per_sample.cpu(), want["correct_per_sample"].cpu())
    assert float(got.acc_std) == pytest.approx(want["acc_std"], rel=1e-12, abs=1e-12)
    valid = want["valid"].cpu()
    ll = got.log_likelihood.cpu().reshape(-1)
    assert torch.isnan(ll[~valid]).all() and not torch.isnan(ll[valid]).any()
    np.testing.assert_allclose(ll[valid], want["log_likelihood"].cpu()[valid], rtol=tol, atol=tol)
    if valid.any():
        assert float(got.nll) == pytest.approx(float(want["nll"]), rel=tol, abs=tol)
    else:
        assert np.isnan(float(got.nll))
    bma = int(((want["probs"].argmax(-1).cpu() == want["yc"].cpu()) & valid).sum())
    # (a row whose top two means are within 1e-6 may go either way)
    slack = int((close & valid).sum())
    assert abs(int(got.bma_correct) - bma) <= slack
    assert int(got.invalid_labels) == want["invalid"]


def make_logits(S, R, C, dtype, strided, gen):
    scale = 3.0
    if strided:  # sample stride and row stride larger than the data they hold
        big = torch.randn(S, R + 3, C + 5, generator=gen) * scale
        x = big.to(dtype)[:, 1:R + 1, 2:C + 2]
    else:
        x = (torch.randn(S, R, C, generator=gen) * scale).to(dtype)
    x = x.clone() if not strided else x
    if C >= 3:
        x[:, 0, 1::2] = float("-inf")  # row 0: -inf entries (every other class)
        x[:, 1, :] = x[:, 1, :].clamp(max=3.0)
        x[:, 1, 0] = 4.0                  # row 1: exact ties (representable in bf16 / fp16) -> first index
        x[:, 1, C - 1] = 4.0
    if C == 2:
        x[:, 1, :] = 1.5                  # a tie in every sample
    return x


def make_labels(R, C, gen):
    y = torch.randint(0, C, (R,), generator=gen)
    y[2 % R] = -100                      # ignored
    if R > 4:
        y[3], y[4] = C, -5               # out of range: treated as ignored, counted
    if R > 5:
        y[5] = 10 ** 6
    return y


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("S", [1, 10, 64])
@pytest.mark.parametrize("C", [1, 2, 3, 384, 1001, 30522])
def test_mc_predictive_matches_float64(C, S, dtype):
    from bayeformers_amd.sampling import mc_predictive

    gen = torch.Generator().manual_seed(C * 131 + S)
    R = 5 if C > 2048 else 37
    strided = (C + S) % 2 == 1
    x = make_logits(S, R, C, dtype, strided, gen).cuda() if not strided else None
    if strided:
        big = make_logits(S, R, C, dtype, False, gen)
        holder = torch.full((S, R + 3, C + 5), -7.0, dtype=dtype).cuda()
        holder[:, 1:R + 1, 2:C + 2] = big.cuda()
        x = holder[:, 1:R + 1, 2:C + 2]
        assert x.stride(0) == (R + 3) * (C + 5) and x.stride(1) == C + 5
    y = make_labels(R, C, gen).cuda()
    for labels in (None, y):
        got = mc_predictive(x, labels)
        torch.cuda.synchronize()
        check(got, restate(x, labels), x, labels, C)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("C", [64, 30522])
def test_mc_predictive_logit_gaps_beyond_fp32_range(C, dtype):
    """Finite logits 90 and more nats below the row's top: p_s and the mean q fall to fp32 subnormals (or 0), whose
    contribution to the entropies is below 1e-36 — the statistics stay finite and match float64."""
    from bayeformers_amd.sampling import mc_predictive

    gen = torch.Generator().manual_seed(C)
    S, R = 10, 6
    span = 60.0 if dtype == torch.float16 else 150.0  # (fp16 logits: at most 65504, and its steps at 100 are 0.06)
    x = torch.linspace(0.0, -span, C).repeat(S, R, 1) + torch.randn(S, R, C, generator=gen) * 0.5
    x[:, 0, :3] = torch.tensor([0.0, -90.0, -95.0])  # the gaps of the review, explicitly
    x[:, 1, 1:] = -100.0 + torch.randn(S, C - 1, generator=gen)  # one class on top, every other about 100 nats below
    x = x.to(dtype).cuda()
    y = torch.randint(0, C, (R,), generator=gen).cuda()
    y[1] = C - 1  # a label deep in the tail: its log-likelihood is finite in fp64
    for labels in (None, y):
        got = mc_predictive(x, labels)
        torch.cuda.synchronize()
        check(got, restate(x, labels), x, labels, C)
        assert torch.isfinite(got.predictive_entropy).all() and torch.isfinite(got.mutual_information).all()
        if labels is not None:
            assert torch.isfinite(got.log_likelihood).all()


@pytest.mark.parametrize("S,R,C", [(10, 3000, 9), (10, 2100, 384), (4, 1100, 30522)])
def test_mc_predictive_more_rows_than_workgroups(S, R, C):
    """R above the 1024-workgroup grid: a workgroup takes several rows (LDS reused row to row, per-sample counts summed
    over its rows before the cross-workgroup reduction); staged (C = 9, 384) and re-read (C = 30522) paths."""
    from bayeformers_amd.sampling import mc_predictive

    gen = torch.Generator().manual_seed(R)
    x = (torch.randn(S, R, C, generator=gen) * 3).to(torch.bfloat16).cuda()
    y = make_labels(R, C, gen).cuda()
    for labels in (y, None):
        got = mc_predictive(x, labels)
        torch.cuda.synchronize()
        check(got, restate(x, labels), x, labels, C)


def test_mc_predictive_graphs_own_workspaces():
    """Two captured graphs replayed on two streams at once: each graph has its own workspace (its own tickets)."""
    from bayeformers_amd.sampling import mc_predictive

    gen = torch.Generator().manual_seed(11)
    xs = [(torch.randn(10, 2000, 9, generator=gen) * 2).cuda() for _ in range(2)]
    ys = [torch.randint(0, 9, (2000,), generator=gen).cuda() for _ in range(2)]
    mc_predictive(xs[0], ys[0])
    torch.cuda.synchronize()
    graphs, outs = [], []
    for x, y in zip(xs, ys):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            outs.append(mc_predictive(x, y))
        graphs.append(g)
    streams = [torch.cuda.Stream() for _ in range(2)]
    for _ in range(3):
        for g, st in zip(graphs, streams):
            with torch.cuda.stream(st):
                g.replay()
        torch.cuda.synchronize()
        for x, y, o in zip(xs, ys, outs):
            check(o, restate(x, y), x, y, 9)


def test_mc_predictive_token_rows_and_ignore_index():
    from bayeformers_amd.sampling import mc_predictive

    gen = torch.Generator().manual_seed(3)
    x = (torch.randn(6, 3, 7, 9, generator=gen) * 2).to(torch.bfloat16).cuda()
    y = torch.randint(0, 9, (3, 7), generator=gen)
    y[0, :3] = -1
    got = mc_predictive(x, y.cuda(), ignore_index=-1)
    assert got.probs.shape == (3, 7, 9) and got.prediction.shape == (3, 7) and got.log_likelihood.shape == (3, 7)
    check(got, restate(x.reshape(6, 21, 9), y.reshape(-1).cuda(), -1), x, y, 9)
    assert int(got.invalid_labels) == 0


def test_mc_predictive_is_two_launches_and_replayable():
    """Captured in a HIP graph (no synchronisation or allocation inside the kernels), replayed on new logits."""
    from bayeformers_amd.sampling import mc_predictive

    gen = torch.Generator().manual_seed(5)
    x = (torch.randn(10, 32, 2, generator=gen) * 2).cuda()
    y = torch.randint(0, 2, (32,), generator=gen).cuda()
    mc_predictive(x, y)  # warm-up: workspace
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static = mc_predictive(x, y)
    for k in range(3):
        x.copy_(torch.randn(10, 32, 2, generator=gen) * 2)
        g.replay()
        torch.cuda.synchronize()
        check(static, restate(x, y), x, y, 2)
        eager = mc_predictive(x, y)
        for f in ("probs", "predictive_entropy", "expected_entropy", "correct_per_sample", "acc_std", "nll", "log_likelihood"):
            assert torch.equal(getattr(static, f), getattr(eager, f)), f


# ----------------------------------------------------------------------------------------------------- model level
def _bert(qa=False):
    import bayeformers_amd as bf
    from transformers import BertConfig, BertForQuestionAnswering, BertForSequenceClassification

    cfg = BertConfig(hidden_size=128, num_hidden_layers=2, num_attention_heads=4, intermediate_size=512, vocab_size=1000,
                     max_position_embeddings=64)
    torch.manual_seed(0)
    model = (BertForQuestionAnswering if qa else BertForSequenceClassification)(cfg).eval()
    bmodel = bf.to_bayesian(model, delta=0.05, freeze=True).eval().cuda().to(torch.bfloat16)
    bf.fuse_activations(bmodel), bf.fuse_residual_layernorm(bmodel), bf.fuse_shared_inputs(bmodel)
    bf.fuse_attention(bmodel), bf.fuse_embeddings(bmodel)
    torch.manual_seed(7)
    ids = torch.randint(0, cfg.vocab_size, (4, 32)).cuda()
    inputs = {"input_ids": ids, "attention_mask": torch.ones(4, 32, dtype=torch.long, device="cuda")}
    if qa:
        labels = (torch.tensor([3, 0, 17, 31]).cuda(), torch.tensor([5, 0, 20, -100]).cuda())
    else:
        labels = torch.randint(0, 2, (4,)).cuda()
    return bmodel, inputs, labels


@pytest.mark.parametrize("qa", [False, True])
def test_sample_predictive_matches_sample_bayesian(qa):
    import bayeformers_amd as bf
    from bayeformers_amd.sampling import sample_bayesian, sample_predictive

    bmodel, inputs, labels = _bert(qa)
    bf.set_compute_dtype("bf16")
    S = 10
    bf.manual_seed(SEED)
    with torch.no_grad():
        raw, mean, lp, lq = sample_bayesian(bmodel, inputs, S)
    bf.manual_seed(SEED)
    preds = sample_predictive(bmodel, inputs, S, labels=labels)
    labs = labels if qa else (labels,)
    assert len(preds) == len(raw) == len(labs)
    for k, p in enumerate(preds):
        assert torch.equal(p.mean, mean[k]) and torch.equal(p.log_prior, lp) and torch.equal(p.log_variational_posterior, lq)
        assert not p.probs.requires_grad
        C = raw[k].shape[-1]
        check(p, restate(raw[k].reshape(S, -1, C), labs[k]), raw[k], labs[k], C)


def test_graphed_predictive_replays_equal_eager_steps():
    import bayeformers_amd as bf
    from bayeformers_amd.sampling import GraphedSampler, sample_predictive

    bmodel, inputs, labels = _bert()
    bf.set_compute_dtype("bf16")
    S, steps = 10, 3
    label_seq = [labels, 1 - labels, torch.zeros_like(labels)]
    with torch.no_grad():
        sampler = GraphedSampler(bmodel, inputs, S, predictive=True, labels=labels)
        bf.manual_seed(SEED)
        got = [[p.clone() for p in sampler(labels=label_seq[k])] for k in range(steps)]
        sampler.close()
        bf.manual_seed(SEED)
        want = [sample_predictive(bmodel, inputs, S, labels=label_seq[k]) for k in range(steps)]
        # the default sampler is untouched: the same four results as before
        plain = GraphedSampler(bmodel, inputs, S)
        assert len(plain()) == 4
        plain.close()
        bf.manual_seed(SEED)
        cached = [sample_predictive(bmodel, inputs, S, labels=label_seq[k], graph=True) for k in range(steps)]
    for k in range(steps):
        for g, c, w in zip(got[k], cached[k], want[k]):
            for f in ("mean", "probs", "predictive_entropy", "expected_entropy", "mutual_information", "prediction",
                      "correct_per_sample", "acc_std", "bma_correct", "log_likelihood", "nll", "invalid_labels",
                      "log_prior", "log_variational_posterior"):
                assert torch.equal(getattr(g, f), getattr(w, f)), (k, f)
                assert torch.equal(getattr(c, f), getattr(w, f)), (k, f)


# ----------------------------------------------------------------------------------------------------- two ranks
FIELDS = ("mean", "probs", "predictive_entropy", "expected_entropy", "mutual_information", "prediction",
          "correct_per_sample", "acc_std", "bma_correct", "log_likelihood", "nll", "invalid_labels")


def _numpy(preds):
    return [{f: getattr(p, f).float().cpu().numpy() if getattr(p, f).is_floating_point() else getattr(p, f).cpu().numpy()
             for f in FIELDS} for p in preds]


def _worker(rank, world, port, S, q):
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import bayeformers_amd as bf
        from bayeformers_amd.sampling import GraphedSampler, sample_predictive

        calls = {"all_reduce": 0}
        real = dist.all_reduce

        def counted(*a, **k):
            calls["all_reduce"] += 1
            return real(*a, **k)

        def refused(*a, **k):
            raise AssertionError("sample_predictive issued an all-gather")

        dist.all_reduce, dist.all_gather, dist.all_gather_into_tensor = counted, refused, refused
        bmodel, inputs, labels = _bert()
        bf.set_compute_dtype("bf16")
        bf.manual_seed(SEED)
        eager = _numpy(sample_predictive(bmodel, inputs, S, labels=labels))
        n_eager = calls["all_reduce"]
        with torch.no_grad():
            sampler = GraphedSampler(bmodel, inputs, S, predictive=True, labels=labels)
            bf.manual_seed(SEED)
            graphed = _numpy(sampler())
            sampler.close()
        q.put((rank, eager, graphed, n_eager))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_ranks_predictive_match_single_process():
    import torch.multiprocessing as mp

    import bayeformers_amd as bf
    from bayeformers_amd.sampling import sample_predictive

    S, world = 5, 2  # 3 + 2 samples
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, S, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = []
    deadline = time.monotonic() + 500
    while len(res) < len(procs):
        try:
            res.append(q.get(timeout=2))
        except Exception:
            dead = [p.exitcode for p in procs if p.exitcode not in (None, 0)]
            assert not dead, f"a rank exited with {dead}"
            assert time.monotonic() < deadline, "timed out"
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    bmodel, inputs, labels = _bert()
    bf.set_compute_dtype("bf16")
    bf.manual_seed(SEED)
    want = _numpy(sample_predictive(bmodel, inputs, S, labels=labels))[0]
    for rank, eager, graphed, n_eager in sorted(res, key=lambda r: r[0]):
        assert n_eager == 1, n_eager  # one collective: the partials ride in the step's one buffer
        for got in (eager[0], graphed[0]):
            for f in ("correct_per_sample", "acc_std", "bma_correct", "invalid_labels", "prediction"):
                assert np.array_equal(got[f], want[f]), (rank, f)
            np.testing.assert_allclose(got["mean"], want["mean"], rtol=1e-2, atol=1e-3)
            for f in ("probs", "predictive_entropy", "expected_entropy", "mutual_information", "log_likelihood", "nll"):
                np.testing.assert_allclose(got[f], want[f], rtol=1e-5, atol=1e-5, err_msg=f)
        assert all(np.array_equal(eager[0][f], res[0][1][0][f]) for f in FIELDS)  # every rank holds the same statistics
