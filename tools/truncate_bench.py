"""bf_probs_truncate kernel time over the shapes sample_generate feeds it: R model-average rows of V probabilities.

    python tools/truncate_bench.py run [--calls 200] [--out T.json]       (under rocprofv3 --kernel-trace --stats)
    python tools/truncate_bench.py analyze <kernel_trace.csv> [--calls 200]

run: for R in {4, 16, 64} x V in {32000, 128256, 151936} (in that order), rows = softmax(3 * N(0, 1)) logits, truncated
with top_k=50, top_p=0.9, min_p=0.05 (every pass the kernel has) `calls` times after 10 warm-up calls; prints the device-event
time per call (median of 5 windows, launch gaps included).  analyze: the kernel trace's probs_truncate launches, in launch
order, split per shape (warm-ups dropped): the median kernel duration of each.
"""
import argparse
import csv
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(R, V) for R in (4, 16, 64) for V in (32000, 128256, 151936)]
WARMUP = 10
KW = dict(top_k=50, top_p=0.9, min_p=0.05)


def run(calls):
    from bayeformers_amd import ops

    res = {}
    g = torch.Generator(device="cuda").manual_seed(0)
    for R, V in SHAPES:
        probs = torch.softmax(3.0 * torch.randn(R, V, device="cuda", generator=g), -1)
        out = torch.empty_like(probs)
        for _ in range(WARMUP):
            ops.truncate_probs(probs, out=out, **KW)
        per = calls // 5
        times = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(per):
                ops.truncate_probs(probs, out=out, **KW)
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b) * 1e3 / per)
        for _ in range(calls - 5 * per):
            ops.truncate_probs(probs, out=out, **KW)
        kept = int((out > 0).sum()) / R
        res[f"R{R}_V{V}"] = {"us_per_call": round(statistics.median(times), 2), "kept_per_row": round(kept, 1)}
        print(json.dumps({"R": R, "V": V, **res[f"R{R}_V{V}"]}), flush=True)
    torch.cuda.synchronize()
    return res


def analyze(path, calls):
    with open(path) as f:
        ks = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in csv.DictReader(f)
                    if "probs_truncate" in r["Kernel_Name"])
    n = WARMUP + calls
    assert len(ks) == n * len(SHAPES), (len(ks), n * len(SHAPES))
    return {f"R{R}_V{V}": {"kernel_us_median": round(statistics.median((e - s) / 1e3 for s, e in ks[i * n + WARMUP:(i + 1) * n]), 2)}
            for i, (R, V) in enumerate(SHAPES)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["run", "analyze"])
    ap.add_argument("path", nargs="?")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.what == "analyze":
        res = analyze(a.path, a.calls)
    else:
        assert torch.cuda.is_available(), "this benchmark measures the GPU"
        res = run(a.calls)
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
