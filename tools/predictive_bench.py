"""Time the Monte-Carlo predictive statistics (bf_mc_predictive_partial + _finish, two launches) with device events,
and the graphed BERT-base evaluation step (bench.py's model and batch, S = 10) with and without predictive=True.

    python tools/predictive_bench.py [--iters N] [--skip-model]

Bytes per call are the least the statistics can move: the S x R x C logits read once, the R x C fp32 probabilities
written once (the fp32 partial sums in between are not counted); GB/s against the 6.3 TB/s measured HBM rate of MI355X
(MI355X_MICROARCH.md).  Kernel times under rocprofv3: `rocprofv3 --kernel-trace --stats -- python tools/predictive_bench.py`."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

HBM_GBS = 6300.0
SHAPES = [(10, 32, 2), (10, 32, 384), (10, 4096, 9), (10, 4096, 30522)]


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def kernels(iters):
    from bayeformers_amd.sampling import mc_predictive

    g = torch.Generator(device="cuda").manual_seed(1)
    for S, R, C in SHAPES:
        x = (torch.randn(S, R, C, device="cuda", generator=g) * 3).to(torch.bfloat16)
        y = torch.randint(0, C, (R,), device="cuda", generator=g)
        ms = timed(lambda: mc_predictive(x, y), iters if R * C < 1 << 24 else max(3, iters // 10))
        nbytes = x.numel() * x.element_size() + R * C * 4
        gbs = nbytes / ms / 1e6
        print(json.dumps({"what": "mc_predictive bf16 + labels", "S": S, "R": R, "C": C, "us": round(ms * 1e3, 2),
                          "GB": round(nbytes / 1e9, 4), "GB_per_s": round(gbs, 1), "frac_of_6.3TBps": round(gbs / HBM_GBS, 3)}),
              flush=True)
        del x, y


def model(iters):
    import bayeformers_amd as bf
    from bench import build_bert
    from bayeformers_amd.sampling import GraphedSampler

    S = 10
    bmodel, _, inputs, _, labels, _ = build_bert("cuda", "bf16")
    bf.set_compute_dtype("bf16")
    labels = labels.cuda()
    res = {}
    with torch.no_grad():
        for name, kw in (("graphed eval step", {}), ("graphed eval step + predictive", {"predictive": True, "labels": labels})):
            sampler = GraphedSampler(bmodel, inputs, S, **kw)
            res[name] = timed(sampler, iters)
            sampler.close()
    for name, ms in res.items():
        print(json.dumps({"what": name, "model": "BERT-base seq-cls B=32 L=128 bf16", "S": S, "ms": round(ms, 4)}), flush=True)
    a, b = res["graphed eval step"], res["graphed eval step + predictive"]
    print(json.dumps({"what": "predictive overhead of the graphed eval step", "us": round((b - a) * 1e3, 2),
                      "fraction": round((b - a) / a, 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--skip-model", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("predictive_bench: needs a GPU (there is nothing to time on the CPU)")
    kernels(args.iters)
    if not args.skip_model:
        model(args.iters)


if __name__ == "__main__":
    main()
