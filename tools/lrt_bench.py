#!/usr/bin/env python
"""Measure the local reparameterisation estimator (bnn.Linear with local = True) against the default one on one MI355X.

    python tools/lrt_bench.py [--out profiles/local_reparameterization.json] [--quick] [--skip-bert]

What is timed (device events around `iters` calls, after a warm-up of every shape; the two sides of a comparison alternate
round by round in one process, and the median with the min .. max spread over the rounds is reported):
  layers    forward (no_grad) and forward+backward of ONE layer inside a bnn.Model, local against default: the BERT-base shapes
            (S 10, M 4096; 768->768, 768->3072 with the fused GELU, 3072->768) and a few-rows class (S 10, M 16 / 64 / 256;
            4096->4096)
  forms     the two moments [m; v] as ONE bf_gemm_nt_act launch (pair axis = sample axis) against two S = 1 launches
  kernels   every new pass alone, with the bytes it must move and the bytes/s it reaches
  combine   bf_lrt_combine against the framework op chain it replaces (zeta, sqrt, multiply-add, GELU, casts)
  routes    the kernel route against the framework composite of the same layer (what ops.lrt_kernel_wins decides)
  bert      a BERT-base training step (bench.py's model, batch 32 x 128, AdamW) at S 10 and S 2, local against default:
            time per step and the allocator's peak
Nothing is compared with a number from another run.  Needs a ROCm device; there is no CPU path."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bayeformers_amd as bf  # noqa: E402
import bayeformers_amd.nn as bnn  # noqa: E402
from bayeformers_amd import ops  # noqa: E402

BF = torch.bfloat16


def time_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def alternate(fns, iters, rounds, warm=3):
    """{name: (median ms, min ms, max ms)} of each callable, the callables taking turns round by round."""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    got = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            got[k].append(time_ms(fn, iters))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in got.items()}


def fmt(t):
    return f"{t[0] * 1e3:9.1f} us ({t[1] * 1e3:.1f} .. {t[2] * 1e3:.1f})"


def make_layer(K, N, act, local):
    torch.manual_seed(1)
    lin = torch.nn.Linear(K, N)
    layer = bnn.Linear.from_frequentist(lin, delta=0.05)  # MOPED: sigma = 0.05 |w|, Gaussian priors
    layer.activation = "gelu" if act else None
    layer.local = local
    return bnn.Model(layer).cuda().to(BF)


def bench_layers(shapes, iters, rounds):
    rows = []
    for (S, M, K, N, act) in shapes:
        x = torch.randn(M, K, generator=torch.Generator().manual_seed(2)).to(BF).cuda()
        xs = x.repeat(S, 1)
        dy = torch.randn(S * M, N, generator=torch.Generator().manual_seed(3)).to(BF).cuda()
        models = {"default": make_layer(K, N, act, False), "local": make_layer(K, N, act, True)}

        def fwd(m):
            def run():
                with torch.no_grad(), m.monte_carlo(S):
                    m(xs)
            return run

        def fwd_bwd(m):
            xin = xs.clone().requires_grad_(True)

            def run():
                for p in m.parameters():
                    p.grad = None
                xin.grad = None
                with m.monte_carlo(S):
                    y = m(xin)
                y.backward(dy)
            return run

        f = alternate({k: fwd(m.eval()) for k, m in models.items()}, iters, rounds)
        fb = alternate({k: fwd_bwd(m.train()) for k, m in models.items()}, iters, rounds)
        normals = {"default": S * N * K, "local": S * M * N}
        row = {"S": S, "M": M, "K": K, "N": N, "gelu": bool(act), "forward_ms": f, "forward_backward_ms": fb,
               "normals_drawn": normals, "forward_local_over_default": f["local"][0] / f["default"][0],
               "forward_backward_local_over_default": fb["local"][0] / fb["default"][0]}
        rows.append(row)
        print(f"layer S={S} M={M} {K}->{N}{' +gelu' if act else ''}: fwd default {fmt(f['default'])} local {fmt(f['local'])} "
              f"({row['forward_local_over_default']:.2f}x) | fwd+bwd default {fmt(fb['default'])} local {fmt(fb['local'])} "
              f"({row['forward_backward_local_over_default']:.2f}x)", flush=True)
    return rows


def bench_forms(shapes, iters, rounds):
    rows = []
    for (S, M, K, N, act) in shapes:
        model = make_layer(K, N, act, True).eval()
        xs = torch.randn(S * M, K, generator=torch.Generator().manual_seed(2)).to(BF).cuda()

        def form(one):
            def run():
                ops.LRT_ONE_LAUNCH = one
                with torch.no_grad(), model.monte_carlo(S):
                    model(xs)
            return run

        keep = ops.LRT_ONE_LAUNCH
        try:
            t = alternate({"one_launch": form(True), "two_launches": form(False)}, iters, rounds)
        finally:
            ops.LRT_ONE_LAUNCH = keep
        rows.append({"S": S, "M": M, "K": K, "N": N, "forward_ms": t})
        print(f"forms S={S} M={M} {K}->{N}: one launch {fmt(t['one_launch'])}, two launches {fmt(t['two_launches'])}", flush=True)
    return rows


def bench_kernels(S, M, K, N, iters, rounds):
    """Every pass alone at one layer shape; bytes = what the pass must read and write once."""
    R = S * M
    R_pad = (R + 63) // 64 * 64
    g = torch.Generator().manual_seed(4)
    model = make_layer(K, N, False, True)
    layer = model.model
    x = torch.randn(R, K, generator=g).to(BF).cuda()
    m = torch.randn(R, N, generator=g).cuda()
    v = torch.rand(R, N, generator=g).cuda()
    dy = torch.randn(R, N, generator=g).to(BF).cuda()
    sd = torch.rand(R, N, generator=g).to(BF).cuda()
    pre = torch.randn(R, N, generator=g).to(BF).cuda()
    ab = torch.randn(2, R_pad, K, generator=g).to(BF).cuda()
    dsig2 = torch.randn(N, K, generator=g).cuda()
    passes = {
        "bf_lrt_operands": (lambda: ops.lrt_operands(layer), N * K * (8 + 4) + N * (8 + 8)),
        "bf_lrt_square (pair)": (lambda: ops.lrt_square(x, R_pad), R * K * 2 + 2 * R_pad * K * 2),
        "bf_lrt_square (x^2 alone)": (lambda: ops.lrt_square(x, R, pair=False), R * K * 2 * 2),
        "bf_lrt_combine (inference)": (lambda: ops.lrt_combine(m, v, S, 1, 0, 0), R * N * (8 + 2)),
        "bf_lrt_combine (training, gelu)": (lambda: ops.lrt_combine(m, v, S, 1, 0, 0, 1, True, True), R * N * (8 + 6)),
        "bf_lrt_grad_prepare": (lambda: ops.lrt_grad_prepare(dy, None, sd, S, R_pad, 1, 0, 0), R * N * 4 + 2 * R_pad * N * 2),
        "bf_lrt_grad_prepare (gelu)": (lambda: ops.lrt_grad_prepare(dy, pre, sd, S, R_pad, 1, 0, 0), R * N * 6 + 2 * R_pad * N * 2),
        "bf_lrt_dx": (lambda: ops.lrt_dx(ab, x), R * K * 2 * 4),
        "bf_lrt_drho": (lambda: ops.lrt_drho(dsig2, layer.weight.rho), N * K * 12),
    }
    if all(isinstance(p, bnn.Gaussian) for p in (layer.weight_prior,)):
        passes["bf_kl_gaussian"] = (lambda: ops.kl_gaussian(layer.weight, layer.weight_prior), N * K * 16)
    t = alternate({k: f for k, (f, _) in passes.items()}, iters, rounds)
    rows = []
    for k, (_, nbytes) in passes.items():
        rate = nbytes / (t[k][0] * 1e-3) / 1e12
        rows.append({"pass": k, "bytes": nbytes, "ms": t[k], "TB_per_s": rate})
        print(f"kernel {k:34s} {fmt(t[k])}  {nbytes / 1e6:9.1f} MB  {rate:6.2f} TB/s", flush=True)
    # the framework chain bf_lrt_combine replaces, on the same fp32 moments, zeta included
    def chain(act):
        def run():
            z = ops.lrt_zeta(S, M, N, 1, 0, 0)
            p = (m + torch.sqrt(v) * z).to(BF)
            return torch.nn.functional.gelu(p) if act else p
        return run

    c = alternate({"kernel": lambda: ops.lrt_combine(m, v, S, 1, 0, 0), "framework": chain(False),
                   "kernel_gelu": lambda: ops.lrt_combine(m, v, S, 1, 0, 0, 1), "framework_gelu": chain(True)}, iters, rounds)
    print(f"combine: kernel {fmt(c['kernel'])} framework chain {fmt(c['framework'])} | gelu: kernel {fmt(c['kernel_gelu'])} "
          f"framework chain {fmt(c['framework_gelu'])}", flush=True)
    return {"S": S, "M": M, "K": K, "N": N, "passes": rows, "combine_vs_framework_ms": c}


def bench_routes(shapes, iters, rounds):
    rows = []
    supported = ops.lrt_supported
    for (S, M, K, N, act) in shapes:
        model = make_layer(K, N, act, True).train()
        xs = torch.randn(S * M, K, generator=torch.Generator().manual_seed(2)).to(BF).cuda()
        dy = torch.randn(S * M, N, generator=torch.Generator().manual_seed(3)).to(BF).cuda()

        def route(kernel):
            xin = xs.clone().requires_grad_(True)

            def run():
                ops.lrt_supported = supported if kernel else (lambda *a, **k: False)
                for p in model.parameters():
                    p.grad = None
                xin.grad = None
                with model.monte_carlo(S):
                    y = model(xin)
                y.backward(dy)
            return run

        try:
            t = alternate({"kernels": route(True), "composite": route(False)}, iters, rounds)
        finally:
            ops.lrt_supported = supported
        rows.append({"S": S, "M": M, "K": K, "N": N, "forward_backward_ms": t})
        print(f"routes S={S} M={M} {K}->{N}: kernels {fmt(t['kernels'])}, framework composite {fmt(t['composite'])}", flush=True)
    return rows


def bench_bert(samples, steps, rounds):
    import bench
    from bayeformers_amd.training import release_training_buffers, training_step

    rows = []
    for S in samples:
        res = {}
        for name in ("default", "local"):
            bmodel, _, inputs, _, labels, _ = bench.build_bert("cuda", "bf16")
            if name == "local":
                bf.local_reparameterization(bmodel)
            labels_d = labels.cuda()
            params = [p for p in bmodel.parameters() if p.requires_grad]
            opt = torch.optim.AdamW(params, lr=2e-5, eps=1e-8, weight_decay=0.0, fused=True)
            nll = lambda mean: torch.nn.functional.cross_entropy(mean[0].float(), labels_d)  # noqa: E731
            step = lambda: training_step(bmodel, inputs, S, nll, opt, 2105, max_grad_norm=1.0)  # noqa: E731
            bf.manual_seed(7)
            for _ in range(3):
                step()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            times = [time_ms(step, steps) for _ in range(rounds)]
            res[name] = {"ms": (statistics.median(times), min(times), max(times)),
                         "peak_allocated_GB": torch.cuda.max_memory_allocated() / 2 ** 30}
            release_training_buffers(bmodel)
            del bmodel, opt, params
            torch.cuda.empty_cache()
        rows.append({"S": S, **res})
        print(f"bert-base training step S={S}: default {fmt(res['default']['ms'])} peak {res['default']['peak_allocated_GB']:.2f} GB | "
              f"local {fmt(res['local']['ms'])} peak {res['local']['peak_allocated_GB']:.2f} GB", flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="fewer iterations and rounds")
    ap.add_argument("--skip-bert", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lrt_bench.py needs a ROCm device")
    bf.set_compute_dtype("bf16")
    iters, rounds = (5, 3) if args.quick else (20, 5)
    bert_base = [(10, 4096, 768, 768, False), (10, 4096, 768, 3072, True), (10, 4096, 3072, 768, False)]
    few_rows = [(10, 16, 4096, 4096, False), (10, 64, 4096, 4096, False), (10, 256, 4096, 4096, False)]
    out = {"device": torch.cuda.get_device_name(0), "iters": iters, "rounds": rounds,
           "ms_fields": "(median, min, max) over the rounds"}
    out["layers"] = bench_layers(bert_base + few_rows, iters, rounds)
    out["forms"] = bench_forms(bert_base + few_rows[1:2], iters, rounds)
    out["kernels"] = bench_kernels(10, 4096, 768, 3072, iters, rounds)
    out["routes"] = bench_routes(bert_base[:2] + few_rows[1:2], max(iters // 2, 3), rounds)
    if not args.skip_bert:
        out["bert_training_step"] = bench_bert((10, 2), 3 if args.quick else 5, 3)
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
