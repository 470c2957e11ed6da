"""Logit soft-capping (Gemma 2): what the cap costs the causal grouped-query kernels and the KV-cache decode kernel, and what
they give against the only framework path that computes the function, the model's eager chain; interleaved in one process.

    python tools/softcap_attention_bench.py [--prefill] [--decode] [--iters N] [--rounds R] [--out R.json]

Gemma 2 shapes, bf16, softcap 50: H / Hkv 8 / 4 (2B) and 16 / 8 (9B) at D 256, 32 / 16 (27B) at D 128.
Prefill (B 2): T 512, 2048, 8192 without a window and T 8192 with the sliding layers' W 4096; forward, and forward +
backward (the forward that keeps lse, then the backward entry).  Three candidates: the soft-cap entry, the SAME entry without
the cap (the kernels as they were: the difference is the price of the tanh), and the eager chain of transformers' gemma2
eager_attention_forward with the cap (repeat_kv, matmul, / softcap, tanh, * softcap, + the additive mask, fp32 softmax,
matmul; autograd for the backward) on the mask a decoder hands it.
Decode (N 8, Tq 1): Tk 512, 4096, 32768 and Tk 32768 behind W 4096, the same three candidates plus the fixed-capacity form.
Times: device events around each call, the median of `iters` calls per round, `rounds` rounds that alternate the candidates;
reported: the median over the rounds and their spread (max - min) / median.  Every soft-cap result is checked against the
eager chain on the same inputs before it is timed.
"""
import argparse
import json
import os
import statistics
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CAP = 50.0
LAYOUTS = ((8, 4, 256), (16, 8, 256), (32, 16, 128))
HBM = 6.3e12


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
    """{name: (median over the rounds, (max - min) / median)}; one warm-up call each, then the candidates alternate"""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(rounds):
        for key, fn in fns.items():
            ts[key].append(timed(fn, iters))
    return {k: (statistics.median(v), (max(v) - min(v)) / statistics.median(v)) for k, v in ts.items()}


def rel(a, b):
    return ((a.float() - b.float()).abs().max() / b.float().abs().max()).item()


def visible(Tq, Tk, W):
    i = (Tk - Tq + torch.arange(Tq, device="cuda"))[:, None]
    j = torch.arange(Tk, device="cuda")[None, :]
    return (j <= i) if W is None else (j <= i) & (i - j < W)


def prefill(iters, rounds):
    import bayeformers_amd as bf
    from bayeformers_amd import ops

    rows = []
    B = 2
    for H, Hkv, D in LAYOUTS:
        scale = D ** -0.5
        mod = types.SimpleNamespace(is_causal=True, num_key_value_groups=H // Hkv, training=False)
        for T, W in ((512, None), (2048, None), (8192, None), (8192, 4096)):
            g = torch.Generator(device="cuda").manual_seed(0)
            q = torch.randn(B, T, H * D, device="cuda", generator=g, dtype=torch.bfloat16).view(B, T, H, D).transpose(1, 2)
            k, v = (torch.randn(B, T, Hkv * D, device="cuda", generator=g, dtype=torch.bfloat16).view(B, T, Hkv, D)
                    .transpose(1, 2) for _ in range(2))
            go = torch.randn(B, T, H, D, device="cuda", generator=g, dtype=torch.bfloat16)
            mask = visible(T, T, W)[None, None].expand(B, 1, T, T)  # the SDPA-format bool mask of a decoder's mask function
            qs, ks, vs = (t.detach().clone().requires_grad_(True) for t in (q, k, v))

            def eager(a, b, c):
                return bf._softcap_eager(mod, a, b, c, mask, 0.0, scale, CAP)

            def fwd(cap):
                return ops.attention_forward_gqa(q, k, v, None, scale, True, None, window=W, softcap=cap)

            def fwd_bwd(cap):
                out, lse = ops.attention_forward_gqa(q, k, v, None, scale, True, None, want_lse=True, window=W, softcap=cap)
                return ops.attention_backward_gqa(q, k, v, None, None, out, go, lse, scale, True, window=W, softcap=cap)

            def eager_fwd_bwd():
                return torch.autograd.grad(eager(qs, ks, vs), (qs, ks, vs), go)

            with torch.no_grad():
                err = rel(fwd(CAP), eager(q, k, v))
            grads, ref_grads = fwd_bwd(CAP), eager_fwd_bwd()
            gerr = max(rel(a, b.transpose(1, 2)) for a, b in zip(grads, ref_grads))
            del grads, ref_grads
            with torch.no_grad():
                t = rounds_of({"softcap_fwd": lambda: fwd(CAP), "plain_fwd": lambda: fwd(None),
                               "eager_fwd": lambda: eager(q, k, v)}, rounds, iters)
            t.update(rounds_of({"softcap_fwd_bwd": lambda: fwd_bwd(CAP), "plain_fwd_bwd": lambda: fwd_bwd(None),
                                "eager_fwd_bwd": eager_fwd_bwd}, rounds, iters))
            row = {"B": B, "H": H, "Hkv": Hkv, "D": D, "T": T, "W": W, "max_rel_err_vs_eager": round(err, 5),
                   "max_rel_grad_err_vs_eager": round(gerr, 5)}
            for key, (s, spread) in t.items():
                row[key] = {"ms": round(s * 1e3, 4), "spread": round(spread, 3)}
            for what in ("fwd", "fwd_bwd"):
                row[f"{what}_cost_of_cap"] = round(t[f"softcap_{what}"][0] / t[f"plain_{what}"][0], 3)
                row[f"{what}_speedup_vs_eager"] = round(t[f"eager_{what}"][0] / t[f"softcap_{what}"][0], 3)
            rows.append(row)
            print(json.dumps(row), flush=True)
            del q, k, v, go, qs, ks, vs, mask
            torch.cuda.empty_cache()
    return rows


def decode(iters, rounds):
    import bayeformers_amd as bf
    from bayeformers_amd import ops

    rows = []
    N, Tq = 8, 1
    for H, Hkv, D in LAYOUTS:
        scale = D ** -0.5
        mod = types.SimpleNamespace(is_causal=True, num_key_value_groups=H // Hkv, training=False)
        for Tk, W in ((512, None), (4096, None), (32768, None), (32768, 4096)):
            k = torch.randn(N, Hkv, Tk, D, device="cuda", dtype=torch.bfloat16)
            v = torch.randn(N, Hkv, Tk, D, device="cuda", dtype=torch.bfloat16)
            q = torch.randn(N, Tq, H, D, device="cuda", dtype=torch.bfloat16).transpose(1, 2)
            L = torch.tensor([Tk], device="cuda")
            mask = None if W is None else visible(Tq, Tk, W)[None, None].expand(N, 1, Tq, Tk)
            ws = torch.empty(max(ops.attention_decode_workspace_bytes(q, k, v), 16), dtype=torch.uint8, device="cuda")

            def eager():
                return bf._softcap_eager(mod, q, k, v, mask, 0.0, scale, CAP)

            with torch.no_grad():
                err = rel(ops.attention_forward_decode(q, k, v, None, scale, workspace=ws, window=W, softcap=CAP), eager())
                t = rounds_of({
                    "softcap": lambda: ops.attention_forward_decode(q, k, v, None, scale, workspace=ws, window=W, softcap=CAP),
                    "plain": lambda: ops.attention_forward_decode(q, k, v, None, scale, workspace=ws, window=W),
                    "softcap_len": lambda: ops.attention_forward_decode_len(q, k, v, L, None, scale, workspace=ws, window=W,
                                                                            softcap=CAP),
                    "eager": eager,
                }, rounds, iters)
            read = Tk if W is None else min(Tk, W + Tq - 1)
            kv_bytes = 2 * N * Hkv * read * D * 2
            row = {"N": N, "H": H, "Hkv": Hkv, "D": D, "Tq": Tq, "Tk": Tk, "W": W, "max_rel_err_vs_eager": round(err, 5)}
            for key, (s, spread) in t.items():
                row[key] = {"us": round(s * 1e6, 2), "spread": round(spread, 3), "hbm_frac": round(kv_bytes / s / HBM, 3)}
            row["cost_of_cap"] = round(t["softcap"][0] / t["plain"][0], 3)
            row["speedup_vs_eager"] = round(t["eager"][0] / t["softcap"][0], 3)
            rows.append(row)
            print(json.dumps(row), flush=True)
            del k, v, q
            torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prefill", action="store_true")
    ap.add_argument("--decode", action="store_true")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU"
    if not (a.prefill or a.decode):
        a.prefill = a.decode = True
    res = {}
    if a.prefill:
        res["prefill"] = prefill(a.iters, a.rounds)
    if a.decode:
        res["decode"] = decode(a.iters * 5, a.rounds)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
