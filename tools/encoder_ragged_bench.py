"""Encoder attention at lengths that are no multiple of 128: the any-length entries (bf_attention_fwd_any /
bf_attention_bwd_any and their dropout siblings, what `bayeformers_amd.encoder_ragged_attention()` routes to) against
  (a) sdpa — the framework's sdpa_attention_forward over the additive padding mask, the route such a call takes with the
      switch off (with p > 0: the framework's dropout);
  (b) gqa  — the generic non-causal kernels, ops.attention_forward_gqa / attention_backward_gqa (no dropout form exists);
  (c) next — the existing encoder kernels at the next multiple of 128, Tp, on padded operands: the cost of the tail;
forward alone and forward + backward, without dropout and with p = 0.1, interleaved in one process.

    python tools/encoder_ragged_bench.py [--iters N] [--rounds R] [--inner K] [--out R.json] [--quick]

Shapes: bf16, S*B = 320 sequences, H = 12, head size 64, T in {64, 100, 197, 200, 300}; a key-padding mask with lengths
drawn from [T/2, T].  Times: device events around `inner` back-to-back calls, the median of `iters` such windows per
round; `rounds` interleaved rounds, of which the median is the figure.  `any` is timed twice per round (any, any_again):
their ratio over the rounds is the null run's spread, the yardstick for every other ratio.  Every route's forward result
is compared with a float64 softmax on every sequence before anything is timed (the entries' must be within 2e-2 of it).  x_<name> = <name> time / any time (> 1: the new entries win)."""
import argparse
import json
import os
import statistics
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, iters, inner):
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3 / inner)
    return statistics.median(ts)


def rounds_of(fns, rounds, iters, inner):
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for key, fn in fns.items():
            out[key].append(timed(fn, iters, inner))
    return out


def rel(a, b):
    return ((a.float() - b.float()).abs().max() / b.float().abs().max()).item()


def operands(B, T, H, D, seed, lens=None):
    g = torch.Generator(device="cuda").manual_seed(seed)
    q, k, v = (torch.randn(B, T, H * D, device="cuda", generator=g, dtype=torch.bfloat16).view(B, T, H, D).transpose(1, 2)
               for _ in range(3))
    go = torch.randn(B, T, H, D, device="cuda", generator=g, dtype=torch.bfloat16)
    if lens is None:
        lens = torch.randint(T // 2, T + 1, (B,), device="cuda", generator=g)
    mask = torch.where(torch.arange(T, device="cuda")[None, :] < lens[:, None], 0.0, float("-inf")).to(torch.float32)
    return q, k, v, go, mask, lens


def run(iters, rounds, inner, quick):
    from transformers.integrations.sdpa_attention import sdpa_attention_forward

    from bayeformers_amd import ops

    B, H, D = 320, 12, 64
    scale = D ** -0.5
    off = torch.zeros(1, dtype=torch.uint8, device="cuda")
    rows = []
    for T in ((100,) if quick else (64, 100, 197, 200, 300)):
        Tp = 128 * ((T + 127) // 128)
        q, k, v, go, mask, lens = operands(B, T, H, D, T)
        qn, kn, vn, gon, maskn, _ = operands(B, Tp, H, D, T + 1, lens)  # the same sequences, padded to Tp
        mask4 = mask[:, None, None, :].to(torch.bfloat16)
        leaves = [t.detach().clone().requires_grad_(True) for t in (q, k, v)]
        leaves_n = [t.detach().clone().requires_grad_(True) for t in (qn, kn, vn)]
        with torch.no_grad():  # every route against float64 on every sequence, before anything is timed
            eval_mod = types.SimpleNamespace(training=False, is_causal=False)
            outs = {"any": ops.attention_forward_any(q, k, v, mask, scale, off),
                    "sdpa": sdpa_attention_forward(eval_mod, q, k, v, mask4, dropout=0.0, scaling=scale, is_causal=False)[0],
                    "gqa": ops.attention_forward_gqa(q, k, v, mask, scale, False, off)}
            errs = {name: 0.0 for name in outs}
            for b0 in range(0, B, 16):
                sl = slice(b0, b0 + 16)
                s = torch.einsum("bhqd,bhkd->bhqk", q[sl].double(), k[sl].double()) * scale + mask[sl, None, None, :].double()
                ref = torch.einsum("bhqk,bhkd->bqhd", torch.softmax(s, -1), v[sl].double())
                for name, o in outs.items():
                    errs[name] = max(errs[name], rel(o[sl], ref))
            del s, ref, outs
        err = errs["any"]
        print(json.dumps({"T": T, "max_rel_err_vs_float64": {k_: round(e, 5) for k_, e in errs.items()}}), flush=True)
        assert err < 2e-2, errs
        for p in (0.0, 0.1):
            mod = types.SimpleNamespace(training=p > 0, is_causal=False)
            drop = ops.Dropout(p, 0x5EED, 1, 1) if p else None

            def any_fwd():
                with torch.no_grad():
                    ops.attention_forward_any(q, k, v, mask, scale, off, drop=drop)

            def sdpa_fwd():
                with torch.no_grad():
                    sdpa_attention_forward(mod, q, k, v, mask4, dropout=p, scaling=scale, is_causal=False)

            def gqa_fwd():
                with torch.no_grad():
                    ops.attention_forward_gqa(q, k, v, mask, scale, False, off)

            def next_fwd():
                with torch.no_grad():
                    ops.attention_forward(qn, kn, vn, maskn, scale, off, drop=drop)

            def any_train():
                o = ops.AttentionAnyFn.apply(*leaves, mask, off, scale, drop)
                torch.autograd.grad(o, leaves, go)

            def sdpa_train():
                o = sdpa_attention_forward(mod, *leaves, mask4, dropout=p, scaling=scale, is_causal=False)[0]
                torch.autograd.grad(o, leaves, go)

            def gqa_train():
                o = ops.AttentionGqaFn.apply(*leaves, mask, off, scale, False)
                torch.autograd.grad(o, leaves, go)

            def next_train():
                o = ops.AttentionFn.apply(*leaves_n, maskn, off, scale, drop)
                torch.autograd.grad(o, leaves_n, gon)

            fns = {"any_fwd": any_fwd, "sdpa_fwd": sdpa_fwd, "next_fwd": next_fwd, "any_again_fwd": any_fwd,
                   "any_train": any_train, "sdpa_train": sdpa_train, "next_train": next_train, "any_again_train": any_train}
            if not p:
                fns.update({"gqa_fwd": gqa_fwd, "gqa_train": gqa_train})
            rounds_of(fns, 1, 2, 1)  # warm-up of every shape the timed window uses
            t = rounds_of(fns, rounds, iters, inner)
            row = {"B": B, "H": H, "T": T, "Tp": Tp, "p": p,
                   "max_rel_err_vs_float64": {k_: round(e, 5) for k_, e in errs.items()}}
            for key, ts in t.items():
                row[key] = {"us": round(statistics.median(ts) * 1e6, 1), "spread": round((max(ts) - min(ts)) / min(ts), 3)}
            for mode in ("fwd", "train"):
                base = statistics.median(t[f"any_{mode}"])
                ratios = [a / b for a, b in zip(t[f"any_again_{mode}"], t[f"any_{mode}"])]
                row[f"null_{mode}"] = [round(min(ratios), 3), round(max(ratios), 3)]
                for name in ("sdpa", "gqa", "next"):
                    if f"{name}_{mode}" in t:
                        row[f"x_{name}_{mode}"] = round(statistics.median(t[f"{name}_{mode}"]) / base, 2)
            rows.append(row)
            print(json.dumps(row), flush=True)
        del q, k, v, go, qn, kn, vn, gon, leaves, leaves_n
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10, help="calls between one pair of device events")
    ap.add_argument("--quick", action="store_true", help="T 100 only")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU"
    rows = run(a.iters, a.rounds, a.inner, a.quick)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
