"""FP8 kept weights (keep_weights="fp8") against the bf16 kept weights (keep_weights=True): the skinny decode GEMMs per shape,
sample_generate tokens/s and kept bytes, and the shift of the predictive statistics.

    python tools/kept_fp8_bench.py kernels [--out K.json] [--only N,K,S,M]
    python tools/kept_fp8_bench.py e2e [--out E.json] [--runs 3] [--new-tokens 256] [--samples 4]
    python tools/kept_fp8_bench.py fidelity [--out F.json]

kernels: per layer shape of the DESIGN 4.5 decoder (N x K), S 4 and 10, M 1, 4 and 16 rows per sample: bf_gemm_nt_skinny on
bf16 draws and bf_gemm_nt_skinny_fp8 on their centred FP8 rows, alternated in one process.  Time per call as
tools/generate_bench.py: device events around 200 back-to-back calls after 20 warm-up calls, median of 5 windows (launch gaps
included).  Bytes: S*N*K*2 for bf16; S*N*K + S*N*4 + N*K*2 for fp8 (the centre counted once: it is re-read per sample, from
cache when it fits).  Also the one-off costs: bf_fp8_rows_quantize and bf_fp8_rows_dequantize of the shape.
e2e: sample_generate on the DESIGN 4.5 decoder (tools/generate_bench.py's), B 4, prompt 512, bf16; keep_weights=True and "fp8"
alternated in one process on the dynamic and the graph=True decode paths, `runs` each; tokens/s and kept bytes.
fidelity: teacher-forced logits of one fixed sequence inside a keep_weights=True block and a "fp8" block under one seed: the
largest shifts of mc_predictive's entropies and mutual information, and of the logits.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from generate_bench import HBM, SHAPES, _decoder, _time  # noqa: E402


def kernels(only=None):
    from bayeformers_amd import ops

    rows = []
    configs = [(N, K, S, M) for N, K in SHAPES for S in (4, 10) for M in (1, 4, 16)]
    if only is not None:
        configs = [only]
    for N, K, S, M in configs:
        g = torch.Generator(device="cuda").manual_seed(N + K + S)
        mu = torch.randn(N, K, device="cuda", generator=g) * 0.02
        w = (mu[None] + 0.05 * mu.abs()[None] * torch.randn(S, N, K, device="cuda", generator=g)).to(torch.bfloat16)
        c = mu.to(torch.bfloat16)
        x = torch.randn(S * M, K, device="cuda", generator=g).to(torch.bfloat16)
        q, scale = ops.quantize_rows_fp8(w, c)
        out16 = torch.empty_like(w)
        b16, b8 = S * N * K * 2, S * N * K + S * N * 4 + N * K * 2
        # alternated: bf16, fp8, bf16, fp8; the speed-up is taken on the means of the two
        t16, t8 = [], []
        for _ in range(2):
            t16.append(_time(lambda: ops.skinny_linear_forward(x, w, None, S, N, K)))
            t8.append(_time(lambda: ops.skinny_linear_forward_fp8(x, q, scale, c, None, S, N, K)))
        t16m, t8m = statistics.mean(t16), statistics.mean(t8)
        t_q = _time(lambda: ops.quantize_rows_fp8(w, c, q, scale), iters=20, warm=3)
        t_d = _time(lambda: ops.dequantize_rows_fp8(q, scale, c, out16), iters=20, warm=3)
        rows.append({"N": N, "K": K, "S": S, "M": M, "bf16_MB": round(b16 / 1e6, 2), "fp8_MB": round(b8 / 1e6, 2),
                     "skinny_bf16_us": [round(t, 2) for t in t16], "skinny_fp8_us": [round(t, 2) for t in t8],
                     "speedup": round(t16m / t8m, 3), "bf16_hbm_frac": round(b16 / (t16m * 1e-6) / HBM, 3),
                     "fp8_hbm_frac": round(b8 / (t8m * 1e-6) / HBM, 3), "quantize_us": round(t_q, 2),
                     "dequantize_us": round(t_d, 2)})
        print(json.dumps(rows[-1]), flush=True)
        del w, q, x, out16
    return rows


def e2e(runs, new_tokens, S):
    import bayeformers_amd as bf
    from bayeformers_amd.sampling import sample_generate

    bmodel = _decoder()
    ids = torch.randint(0, 32000, (4, 512), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    modes = {"bf16_keep": True, "fp8_keep": "fp8"}
    paths = {"dynamic": {}, "graph": {"graph": True}}
    res = {f"{m}_{p}": [] for m in modes for p in paths}
    res["samples"] = S
    res["kept_bytes"] = {"bf16_keep": bf.kept_weight_bytes(bmodel, S, torch.bfloat16),
                         "fp8_keep": bf.kept_weight_bytes(bmodel, S, torch.bfloat16, fp8=True)}
    seqs = {}
    with torch.no_grad():
        for keep in modes.values():  # warm-up
            for kw in paths.values():
                sample_generate(bmodel, ids, samples=S, max_new_tokens=8, keep_weights=keep, **kw)
        for _ in range(runs):
            for m, keep in modes.items():
                for p, kw in paths.items():
                    bf.manual_seed(0x5EED)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    gen = sample_generate(bmodel, ids, samples=S, max_new_tokens=new_tokens, keep_weights=keep, **kw)
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                    res[f"{m}_{p}"].append(round(4 * new_tokens / dt, 1))
                    seqs[m, p] = gen.sequences
                    print(json.dumps({"keep_weights": keep, "path": p, "seconds": round(dt, 3),
                                      "tokens_per_s": round(4 * new_tokens / dt, 1)}), flush=True)
    res["tokens_equal_to_bf16_keep"] = {p: round(float((seqs["fp8_keep", p] == seqs["bf16_keep", p]).float().mean()), 4)
                                        for p in paths}
    for k in [k for k in res if isinstance(res[k], list)]:
        v = res[k]
        res[k + "_summary"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
    return res


def fidelity(S=4):
    import bayeformers_amd as bf
    from bayeformers_amd.sampling import mc_predictive

    bmodel = _decoder()
    ids = torch.randint(0, 32000, (2, 256), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    preds, logits = {}, {}
    for keep in (True, "fp8"):
        bf.manual_seed(0x5EED)
        with torch.no_grad(), bmodel.monte_carlo(S), bmodel.pinned_samples(keep_weights=keep):
            out = bmodel(input_ids=ids.repeat(S, 1), use_cache=False).logits
            logits[keep] = out.float()
            preds[keep] = mc_predictive(out.view(S, ids.shape[0], *out.shape[1:]))
    res = {"samples": S, "tokens": ids.numel(),
           "max_logit_shift": round((logits[True] - logits["fp8"]).abs().max().item(), 5),
           "max_abs_logit": round(logits[True].abs().max().item(), 3),
           "same_prediction": round(float((preds[True].prediction == preds["fp8"].prediction).float().mean()), 4)}
    for name in ("predictive_entropy", "expected_entropy", "mutual_information"):
        a, b = getattr(preds[True], name), getattr(preds["fp8"], name)
        res[name] = {"max_shift": round((a - b).abs().max().item(), 6), "mean_shift": round((a - b).abs().mean().item(), 6),
                     "mean_bf16_keep": round(a.mean().item(), 5)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernels", "e2e", "fidelity"])
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--new-tokens", type=int, default=256)
    ap.add_argument("--samples", type=int, default=4)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU"
    if a.what == "kernels":
        res = kernels(tuple(int(v) for v in a.only.split(",")) if a.only else None)
    elif a.what == "e2e":
        res = e2e(a.runs, a.new_tokens, a.samples)
    else:
        res = fidelity(a.samples)
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
