"""Packed-sequence attention timings: the band kernels (bf_attention_fwd_gqa_band / bf_attention_bwd_gqa_band) against the
framework's sdpa_attention_forward over the dense [B, 1, T, T] mask (what a packed row ran before them), forward alone
and forward + backward, interleaved in one process.

    python tools/packed_attention_bench.py [--iters N] [--rounds R] [--out R.json] [--quick]

Shapes: bf16, B 4, H / Hkv 32 / 8 at D 128 and 8 / 4 at D 256, T 2048 and 8192; documents of 512 tokens, of mixed
lengths (boundaries off the tiles) and one single document; without a window and with W 1024.  Times: device events
around each call, the median of `iters` per round; `rounds` interleaved rounds, of which the best is the figure and
(max - min) / min the spread.  Every kernel result is checked against SDPA on the same inputs before it is timed.
x = SDPA time / kernel time.  Flops of a forward: 4 * D * (visible (query, key) pairs) per (sequence, head); the backward
2.5x."""
import argparse
import json
import os
import statistics
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, iters):
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    return statistics.median(ts)


def rounds_of(fns, rounds, iters):
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for key, fn in fns.items():
            out[key].append(timed(fn, iters))
    return out


def layouts(T):
    mixed = [T // 16 + 37, T // 8 - 37, T // 2 + 5]
    return {"docs512": [512] * (T // 512), "mixed": mixed + [T - sum(mixed)], "single": [T]}


def rel(a, b):
    return ((a.float() - b.float()).abs().max() / b.float().abs().max()).item()


def run(iters, rounds, quick):
    from transformers.integrations.sdpa_attention import sdpa_attention_forward

    from bayeformers_amd import ops

    rows = []
    B = 4
    for H, Hkv, D in ((32, 8, 128), (8, 4, 256)):
        for T in ((2048,) if quick else (2048, 8192)):
            g = torch.Generator(device="cuda").manual_seed(0)
            q = torch.randn(B, T, H * D, device="cuda", generator=g, dtype=torch.bfloat16).view(B, T, H, D).transpose(1, 2)
            k, v = (torch.randn(B, T, Hkv * D, device="cuda", generator=g, dtype=torch.bfloat16).view(B, T, Hkv, D)
                    .transpose(1, 2) for _ in range(2))
            go = torch.randn(B, T, H, D, device="cuda", generator=g, dtype=torch.bfloat16)
            scale = D ** -0.5
            mod = types.SimpleNamespace(is_causal=True, num_key_value_groups=H // Hkv, training=False)
            pos = torch.arange(T, device="cuda")
            for name, docs in layouts(T).items():
                ids = torch.cat([torch.full((n,), i, device="cuda") for i, n in enumerate(docs)])[None].expand(B, T)
                for W in (None, 1024):
                    lo, hi = ops.band_bounds(ids, W)
                    mask = ((pos[None, :] <= pos[:, None]) & (pos[None, :] >= lo[:, :, None]))[:, None]
                    pairs = int((pos[None, :] - lo + 1).sum().item())  # visible (query, key) pairs over the batch
                    qs, ks, vs = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
                    with torch.no_grad():
                        out = ops.attention_forward_gqa_band(q, k, v, lo, scale)
                        ref = sdpa_attention_forward(mod, q, k, v, mask, dropout=0.0, scaling=scale)[0]
                    err = rel(out, ref)
                    assert err < 2e-2, err

                    def kernel_fwd():
                        with torch.no_grad():
                            ops.attention_forward_gqa_band(q, k, v, lo, scale)

                    def sdpa_fwd():
                        with torch.no_grad():
                            sdpa_attention_forward(mod, q, k, v, mask, dropout=0.0, scaling=scale)

                    def kernel_train():
                        o = ops.AttentionGqaBandFn.apply(qs, ks, vs, lo, hi, scale)
                        torch.autograd.grad(o, (qs, ks, vs), go)

                    def sdpa_train():
                        o = sdpa_attention_forward(mod, qs, ks, vs, mask, dropout=0.0, scaling=scale)[0]
                        torch.autograd.grad(o, (qs, ks, vs), go)

                    g_k = torch.autograd.grad(ops.AttentionGqaBandFn.apply(qs, ks, vs, lo, hi, scale), (qs, ks, vs), go)
                    g_s = torch.autograd.grad(sdpa_attention_forward(mod, qs, ks, vs, mask, dropout=0.0, scaling=scale)[0],
                                              (qs, ks, vs), go)
                    gerr = max(rel(a, b) for a, b in zip(g_k, g_s))
                    assert gerr < 5e-2, gerr
                    del g_k, g_s
                    fns = {"kernel_fwd": kernel_fwd, "sdpa_fwd": sdpa_fwd, "kernel_train": kernel_train,
                           "sdpa_train": sdpa_train}
                    rounds_of(fns, 1, 2)  # warm-up of every shape the timed window uses
                    t = rounds_of(fns, rounds, iters)
                    row = {"B": B, "H": H, "Hkv": Hkv, "D": D, "T": T, "docs": name, "W": W,
                           "visible_frac_of_causal": round(pairs / (B * T * (T + 1) / 2), 3),
                           "max_rel_err_vs_sdpa": round(err, 5), "max_rel_grad_err_vs_sdpa": round(gerr, 5)}
                    for key, ts in t.items():
                        flops = 4 * D * pairs * H * (3.5 if key.endswith("train") else 1.0)
                        row[key] = {"ms": round(min(ts) * 1e3, 4), "spread": round((max(ts) - min(ts)) / min(ts), 3),
                                    "tflops": round(flops / min(ts) / 1e12, 1)}
                    row["x_fwd"] = round(min(t["sdpa_fwd"]) / min(t["kernel_fwd"]), 2)
                    row["x_train"] = round(min(t["sdpa_train"]) / min(t["kernel_train"]), 2)
                    rows.append(row)
                    print(json.dumps(row), flush=True)
                    del mask, qs, ks, vs, ref, out
            del q, k, v, go
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="T 2048 only")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU"
    rows = run(a.iters, a.rounds, a.quick)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
