"""One training step of tools/generate_bench.py's decoder (8 layers, hidden 1024, 16 heads / 4 kv heads, FFN 2816, bf16)
three ways, interleaved on one box:

    unfused     fuse_attention only: the decoder glue on the framework's ops (the path before the backward kernels)
    fused       + fuse_decoder_blocks(backward=True): bf_add_rmsnorm / bf_rope_qk / bf_swiglu and their backward
    graphed     the fused model under GraphedTrainingStep

    python tools/decoder_train_bench.py step [--rounds 5] [--iters 10]     ms per step, min / median / max over the rounds
    python tools/decoder_train_bench.py kernels                            the three backward kernels alone: us, bytes/s
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/decoder_train_bench.py trace --mode fused --steps 3
                                                                           launches per step and per-kernel time (a run of its own)

profiles/decoder_blocks_train.md holds the numbers."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from generate_bench import HBM, _decoder, _time  # noqa: E402

S, B, T, NB = 4, 4, 512, 100


def _setup(mode):
    import bayeformers_amd as bf
    from bayeformers_amd.training import GraphedTrainingStep, training_step

    bmodel = _decoder()
    if mode != "unfused":
        assert bf.fuse_decoder_blocks(bmodel, backward=True) == 8
    gen = torch.Generator().manual_seed(1)
    ids = torch.randint(0, 32000, (B, T), generator=gen).cuda()
    inputs = {"input_ids": ids, "use_cache": False}

    def nll(mean):
        logits = mean[0].float()
        return torch.nn.functional.cross_entropy(logits[:, :-1].reshape(-1, logits.shape[-1]), ids[:, 1:].reshape(-1))

    opt = torch.optim.AdamW([p for p in bmodel.parameters() if p.requires_grad], lr=torch.tensor(1e-5, device="cuda"),
                            weight_decay=0.0, fused=True, capturable=True)
    bf.manual_seed(0x5EED)
    if mode == "graphed":
        step = GraphedTrainingStep(bmodel, inputs, S, nll, opt, NB, max_grad_norm=None, eager_steps=1)
        return step, step.close
    return (lambda: training_step(bmodel, inputs, S, nll, opt, NB, max_grad_norm=None)), (lambda: None)


def steps(rounds, iters):
    modes = ("unfused", "fused", "graphed")
    fns = {m: _setup(m) for m in modes}
    times = {m: [] for m in modes}
    try:
        for m in modes:  # warm-up (and the capture)
            for _ in range(3):
                fns[m][0]()
        torch.cuda.synchronize()
        for _ in range(rounds):  # interleaved: every round times every mode
            for m in modes:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(iters):
                    fns[m][0]()
                b.record()
                b.synchronize()
                times[m].append(a.elapsed_time(b) / iters)
    finally:
        for m in modes:
            fns[m][1]()
    for m in modes:
        print(json.dumps({"mode": m, "ms_min": round(min(times[m]), 3), "ms_median": round(statistics.median(times[m]), 3),
                          "ms_max": round(max(times[m]), 3), "rounds": rounds, "iters": iters}), flush=True)


def kernels():
    """The three backward kernels at the step's size (S B T = 8192 rows), bf16: us per call and achieved bytes/s against
    the algorithmic bytes (the dgamma partials, 1024 x N fp32 written and read once, are counted for the norm)."""
    from bayeformers_amd import ops

    N, F, H, Hkv, D, rows = 1024, 2816, 16, 4, 64, S * B * T
    dt = torch.bfloat16

    def row(name, nbytes, fn):
        t = _time(fn)
        print(json.dumps({"kernel": name, "rows": rows, "MB": round(nbytes / 1e6, 3), "us": round(t, 2),
                          "TB_per_s": round(nbytes / (t * 1e-6) / 1e12, 3), "hbm_frac": round(nbytes / (t * 1e-6) / HBM, 3)}), flush=True)

    z, dy, h = (torch.randn(rows, N, device="cuda", dtype=dt) for _ in range(3))
    g = torch.ones(N, device="cuda", dtype=dt)
    part = 2 * 1024 * N * 4
    row("add_rmsnorm_bwd (dy, dz_in -> dz, dgamma)", 4 * rows * N * 2 + part, lambda: ops.add_rmsnorm_backward(z, g, dy, 1e-5, grad_sum=h))
    row("add_rmsnorm_bwd (dy -> dz, dgamma)", 3 * rows * N * 2 + part, lambda: ops.add_rmsnorm_backward(z, g, dy, 1e-5))
    Bq = rows // T
    q = torch.randn(Bq, T, H * D, device="cuda", dtype=dt).view(Bq, T, H, D).transpose(1, 2)
    k = torch.randn(Bq, T, Hkv * D, device="cuda", dtype=dt).view(Bq, T, Hkv, D).transpose(1, 2)
    cos, sin = (torch.randn(1, T, D, device="cuda", dtype=dt) for _ in range(2))
    row("rope_qk_bwd (out of place)", 2 * rows * (H + Hkv) * D * 2 + 2 * T * D * 2, lambda: ops.rope_qk_backward(q, k, cos, sin))
    gate, up, d = (torch.randn(rows, F, device="cuda", dtype=dt) for _ in range(3))
    row("swiglu_bwd", 5 * rows * F * 2, lambda: ops.swiglu_backward(gate, up, d))


def trace(mode, n):
    fn, close = _setup(mode)
    try:
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
    finally:
        close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["step", "kernels", "trace"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--mode", choices=["unfused", "fused", "graphed"], default="fused")
    ap.add_argument("--steps", type=int, default=3)
    a = ap.parse_args()
    if a.what == "step":
        steps(a.rounds, a.iters)
    elif a.what == "kernels":
        kernels()
    else:
        trace(a.mode, a.steps)


if __name__ == "__main__":
    main()
