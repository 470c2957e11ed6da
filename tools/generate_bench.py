"""Kept sampled weights for generation: the skinny decode GEMM against what decode runs today, and sample_generate tokens/s.

    python tools/generate_bench.py kernels [--out K.json] [--only N,K,S,M]
    python tools/generate_bench.py e2e [--out E.json] [--runs 3] [--new-tokens 256] [--mode dynamic|static|graph ...]
                                       [--top-k K] [--top-p P] [--min-p M]
                                       [--repetition-penalty R] [--no-repeat-ngram N] [--min-new-tokens M --eos-token-id E]
    python tools/generate_bench.py trace --mode keep|draw [--mode dynamic|static|graph] [--steps 32] [the processors]
                                                                                         (under rocprofv3 --kernel-trace)
    python tools/generate_bench.py analyze <kernel_trace.csv> [--steps 32]
    --fuse-blocks (e2e, trace, kernels): with fuse_decoder_blocks — e2e alternates the fused and the unfused model in one
    process (`..._blocks` rows), trace runs the fused model, kernels measures bf_add_rmsnorm / bf_rope_qk / bf_swiglu instead

kernels: per layer shape of the DESIGN 4.5 decoder (N x K), S and M rows per sample, bf16: bf_gemm_nt_skinny on kept weights,
fused_small (bf_linear_fwd: sampling + GEMM + log-probs, what a decode step runs without keep_weights) and bf_gemm_nt_act on the
same kept weights.  Time per call = device events around 200 back-to-back calls after 20 warm-up calls, median of 5 windows
(launch gaps included).  Weight bandwidth = S*N*K*2 bytes / time, against 6.29 TB/s.
e2e: sample_generate on the DESIGN 4.5 decoder (8 layers, hidden 1024, 16 / 4 heads, FFN 2816, vocab 32000), S 4, B 4, prompt
512, bf16, fuse_attention; keep_weights off and on alternated in one process, `runs` each, and for each of them the decode
paths named by --mode (default all three, alternated): dynamic (the default DynamicCache loop), static
(static_cache=True) and graph (graph=True).  With --top-k / --top-p / --min-p every decode path runs do_sample=True twice,
alternated: without the truncation (`..._sample`) and with it (`..._truncated`).  With --repetition-penalty /
--no-repeat-ngram / --min-new-tokens every decode path runs twice, alternated: without the logits processors (`..._plain`)
and with them (`..._processed`), both with the truncation when one is given.
e2e --kv-cache fp8: the FP8 KV cache instead — graph=True with the bf16 static cache and with kv_cache="fp8", alternated, each
without and with keep_weights=True (`runs` each), tokens/s; then the bytes the caching allocator holds for each static cache
of that generation (torch.cuda.memory_allocated before and after the hand-over's updates) beside plan.kv_cache_bytes.
--prompt / --batch / --samples size it (default 512 / 4 / 4, as above).
trace: a prefill-only generation, a 2 s pause, then a generation of `new-tokens`; analyze splits a kernel trace of it at the
pause and attributes (second - first) to the decode steps: GPU time per kernel class and the host gaps between kernels.
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM = 6.29e12
SHAPES = [(1024, 1024), (256, 1024), (2816, 1024), (1024, 2816), (32000, 1024)]


def _time(fn, iters=200, warm=20, reps=5):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / iters)
    return statistics.median(ts)


def kernels(only=None):
    import bayeformers_amd as bf
    import bayeformers_amd.nn as bnn
    from bayeformers_amd import ops

    bf.set_compute_dtype("bf16")
    rows = []
    configs = [(N, K, S, M) for N, K in SHAPES for S in (4, 10) for M in (1, 4, 16, 64)]
    if only is not None:
        configs = [only]
    for N, K, S, M in configs:
        torch.manual_seed(0)
        layer = bnn.Linear(K, N, bias=False).cuda()
        w = torch.randn(S, N, K, device="cuda", dtype=torch.bfloat16)
        x = torch.randn(S * M, K, device="cuda", dtype=torch.bfloat16)
        lp = torch.empty((S, 2), dtype=torch.float64, device="cuda")
        wbytes = S * N * K * 2
        t_skinny = _time(lambda: ops.skinny_linear_forward(x, w, None, S, N, K))
        t_gemm = _time(lambda: ops.gemm_nt(x, w, None, S, M, N, K, M * K, torch.bfloat16))
        assert M <= ops.fused_small_rows(N, K)
        t_fused = _time(lambda: ops.linear_forward(layer, x, S, 0x5EED, 0, lp))
        rows.append({"N": N, "K": K, "S": S, "M": M, "weight_MB": round(wbytes / 1e6, 2), "skinny_us": round(t_skinny, 2),
                     "fused_small_us": round(t_fused, 2), "gemm_nt_act_us": round(t_gemm, 2),
                     "skinny_hbm_frac": round(wbytes / (t_skinny * 1e-6) / HBM, 3),
                     "gemm_nt_act_hbm_frac": round(wbytes / (t_gemm * 1e-6) / HBM, 3)})
        print(json.dumps(rows[-1]), flush=True)
        del w, x, layer
    return rows


def block_kernels():
    """bf_add_rmsnorm, bf_rope_qk and bf_swiglu at the DESIGN 4.5 decoder's prefill size (S B T = 8192 rows) and decode size (16
    rows), bf16: time per call as in kernels(), achieved bytes/s from the algorithmic bytes; bf_add_layernorm at the same
    rows x N in the same process beside bf_add_rmsnorm (the same structure)."""
    from bayeformers_amd import ops

    N, F, H, Hkv, D, T = 1024, 2816, 16, 4, 64, 512
    dt = torch.bfloat16
    out = []

    def row(name, rows, nbytes, fn):
        t = _time(fn)
        out.append({"kernel": name, "rows": rows, "MB": round(nbytes / 1e6, 3), "us": round(t, 2),
                    "TB_per_s": round(nbytes / (t * 1e-6) / 1e12, 3), "hbm_frac": round(nbytes / (t * 1e-6) / HBM, 3)})
        print(json.dumps(out[-1]), flush=True)

    for rows in (8192, 16):
        x, r = (torch.randn(rows, N, device="cuda", dtype=dt) for _ in range(2))
        g, b = torch.ones(N, device="cuda", dtype=dt), torch.zeros(N, device="cuda", dtype=dt)
        row("add_rmsnorm (x + residual -> sum, norm)", rows, 4 * rows * N * 2, lambda: ops.add_rmsnorm(x, r, g, 1e-5))
        row("add_rmsnorm (x + residual -> norm)", rows, 3 * rows * N * 2, lambda: ops.add_rmsnorm(x, r, g, 1e-5, want_sum=False))
        row("add_layernorm (x + residual -> norm)", rows, 3 * rows * N * 2, lambda: ops.add_layernorm(x, r, g, b, 1e-5))
        row("add_rmsnorm (x -> norm)", rows, 2 * rows * N * 2, lambda: ops.add_rmsnorm(x, None, g, 1e-5, want_sum=False))
        row("add_layernorm (x -> norm)", rows, 2 * rows * N * 2, lambda: ops.add_layernorm(x, None, g, b, 1e-5))
        B, Tq = (rows // T, T) if rows >= T else (rows, 1)
        q = torch.randn(B, Tq, H * D, device="cuda", dtype=dt).view(B, Tq, H, D).transpose(1, 2)
        k = torch.randn(B, Tq, Hkv * D, device="cuda", dtype=dt).view(B, Tq, Hkv, D).transpose(1, 2)
        cos, sin = (torch.randn(1, Tq, D, device="cuda", dtype=dt) for _ in range(2))
        row("rope_qk (in place)", rows, 2 * rows * (H + Hkv) * D * 2 + 2 * Tq * D * 2,
            lambda: ops.rope_qk(q, k, cos, sin, inplace=True))
        gate, up = (torch.randn(rows, F, device="cuda", dtype=dt) for _ in range(2))
        row("swiglu", rows, 3 * rows * F * 2, lambda: ops.swiglu(gate, up))
    return out


def _decoder(fuse_blocks=False):
    from transformers import LlamaConfig, LlamaForCausalLM

    import bayeformers_amd as bf

    cfg = LlamaConfig(hidden_size=1024, num_attention_heads=16, num_key_value_heads=4, num_hidden_layers=8,
                      intermediate_size=2816, vocab_size=32000, max_position_embeddings=1024, tie_word_embeddings=False,
                      attention_dropout=0.0, attn_implementation="sdpa")
    torch.manual_seed(0)
    bmodel = bf.to_bayesian(LlamaForCausalLM(cfg).eval(), delta=0.05, freeze=True).eval().cuda()
    freqs = {n: b.detach().clone() for n, b in bmodel.named_buffers() if "inv_freq" in n}
    bmodel = bmodel.to(torch.bfloat16)
    for n, b in freqs.items():
        setattr(bmodel.get_submodule(n.rsplit(".", 1)[0]), n.rsplit(".", 1)[1], b)
    assert bf.fuse_attention(bmodel)
    if fuse_blocks:
        assert bf.fuse_decoder_blocks(bmodel) == 8
    bf.set_compute_dtype("bf16")
    return bmodel


PATHS = {"dynamic": {}, "static": {"static_cache": True}, "graph": {"graph": True}}


def e2e(runs, new_tokens, paths=("dynamic", "static", "graph"), truncation=None, processors=None, fuse_blocks=False):
    import bayeformers_amd as bf
    from bayeformers_amd.sampling import sample_generate

    # (the same seed: the same weights) unfused first, then with fuse_decoder_blocks, inside every configuration
    models = {"": _decoder()}
    if fuse_blocks:
        models["_blocks"] = _decoder(fuse_blocks=True)
    bmodel = models[""]
    ids = torch.randint(0, 32000, (4, 512), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    variants = {"": {}} if not truncation else {"_sample": dict(do_sample=True),
                                                "_truncated": dict(do_sample=True, **truncation)}
    if processors:
        base = variants["_truncated"] if truncation else {}
        variants = {"_plain": base, "_processed": dict(base, **processors)}
    name = lambda keep, path, v="": (("keep_weights" if keep else "draw_per_step") + ("" if path == "dynamic" else "_" + path)
                                     + v)
    variants = {v + m: (kw, model) for v, kw in variants.items() for m, model in models.items()}
    res = {name(k, p, v): [] for k in (False, True) for p in paths for v in variants}
    res["kept_bytes"] = bf.kept_weight_bytes(bmodel, 4, torch.bfloat16)
    seqs = {}
    with torch.no_grad():
        for keep in (False, True):  # warm-up
            for path in paths:
                for v, (kw, bmodel) in variants.items():
                    sample_generate(bmodel, ids, samples=4, max_new_tokens=8, keep_weights=keep, **PATHS[path], **kw)
        for _ in range(runs):
            for keep in (False, True):
                for path in paths:
                    for v, (kw, bmodel) in variants.items():
                        bf.manual_seed(0x5EED)
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        gen = sample_generate(bmodel, ids, samples=4, max_new_tokens=new_tokens, keep_weights=keep,
                                              generator=torch.Generator(device="cuda").manual_seed(3)
                                              if kw.get("do_sample") else None,
                                              **PATHS[path], **kw)
                        torch.cuda.synchronize()
                        dt = time.perf_counter() - t0
                        res[name(keep, path, v)].append(round(4 * new_tokens / dt, 1))
                        seqs[keep, path, v] = gen.sequences
                        print(json.dumps({"keep_weights": keep, "path": path + v, "seconds": round(dt, 3),
                                          "tokens_per_s": round(4 * new_tokens / dt, 1)}), flush=True)
    first = next(iter(seqs.values()))
    res["same_tokens"] = all(bool(torch.equal(first, v)) for v in seqs.values())
    if fuse_blocks:  # per configuration: does the fused model emit the unfused model's tokens?
        res["same_tokens_blocks"] = {name(*k): bool(torch.equal(v, seqs[k[0], k[1], k[2] + "_blocks"]))
                                     for k, v in seqs.items() if not k[2].endswith("_blocks")}
    for k in [k for k in res if isinstance(res[k], list)]:
        v = res[k]
        res[k + "_summary"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
    return res


def e2e_kv_cache(runs, new_tokens, prompt=512, batch=4, samples=4):
    import bayeformers_amd as bf
    from bayeformers_amd.sampling import _static_cache, sample_generate

    bmodel = _decoder()
    S, B = samples, batch
    ids = torch.randint(0, 32000, (B, prompt), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    configs = [(keep, kv) for keep in (False, True) for kv in (None, "fp8")]
    name = lambda keep, kv: ("keep_weights" if keep else "draw_per_step") + "_graph" + ("_kv_fp8" if kv else "_kv_bf16")
    res = {name(*c): [] for c in configs}
    res.update(samples=S, batch=B, prompt=prompt, new_tokens=new_tokens)
    seqs = {}
    with torch.no_grad():
        for keep, kv in configs:  # warm-up
            sample_generate(bmodel, ids, samples=S, max_new_tokens=8, keep_weights=keep, graph=True, kv_cache=kv)
        for _ in range(runs):
            for keep, kv in configs:
                bf.manual_seed(0x5EED)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                gen = sample_generate(bmodel, ids, samples=S, max_new_tokens=new_tokens, keep_weights=keep, graph=True,
                                      kv_cache=kv)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                res[name(keep, kv)].append(round(B * new_tokens / dt, 1))
                seqs[keep, kv] = gen.sequences
                print(json.dumps({"keep_weights": keep, "kv_cache": kv, "seconds": round(dt, 3),
                                  "tokens_per_s": round(B * new_tokens / dt, 1)}), flush=True)
        # tokens of the two caches: equal up to the first step at which e4m3's rounding flips an argmax
        diff = (seqs[True, None] != seqs[True, "fp8"]).any(0).nonzero()
        res["first_differing_position"] = int(diff[0]) - prompt if diff.numel() else None
        # the allocator's view of each static cache at this generation's capacity
        cap, cfg = prompt + new_tokens - 1, bmodel.model.config
        k = torch.randn(S * B, prompt, cfg.num_key_value_heads * cfg.head_dim, device="cuda", dtype=torch.bfloat16)
        k = k.view(S * B, prompt, cfg.num_key_value_heads, cfg.head_dim).transpose(1, 2)
        for kv in (None, "fp8"):
            torch.cuda.synchronize()
            before = torch.cuda.memory_allocated()
            cache = _static_cache(bmodel, cap, kv_cache=kv)
            for i in range(len(cache.layers)):
                cache.update(k, k, i)
            torch.cuda.synchronize()
            res["cache_bytes_allocated" + ("_fp8" if kv else "_bf16")] = torch.cuda.memory_allocated() - before
            res["kv_cache_bytes" + ("_fp8" if kv else "_bf16")] = bf.kv_cache_bytes(bmodel, S, B, cap, fp8=kv is not None)
            del cache
    for key in [key for key in res if isinstance(res[key], list)]:
        v = res[key]
        res[key + "_summary"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
    for keep in (False, True):
        res[("keep_weights" if keep else "draw_per_step") + "_fp8_over_bf16"] = round(
            res[name(keep, "fp8") + "_summary"]["median"] / res[name(keep, None) + "_summary"]["median"], 3)
    return res


def trace(mode, new_tokens, path="dynamic", processors=None, fuse_blocks=False):
    from bayeformers_amd.sampling import sample_generate

    bmodel = _decoder(fuse_blocks)
    ids = torch.randint(0, 32000, (4, 512), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    kw = dict(keep_weights=mode == "keep", **PATHS[path], **(processors or {}))
    with torch.no_grad():
        sample_generate(bmodel, ids, samples=4, max_new_tokens=4, **kw)  # warm-up
        torch.cuda.synchronize()
        time.sleep(2.0)
        sample_generate(bmodel, ids, samples=4, max_new_tokens=1, **kw)  # prefill only
        torch.cuda.synchronize()
        time.sleep(2.0)
        sample_generate(bmodel, ids, samples=4, max_new_tokens=new_tokens, **kw)
        torch.cuda.synchronize()


def _klass(name):
    for key, k in (("rmsnorm", "decoder blocks (rmsnorm / rope / swiglu)"), ("rope_qk", "decoder blocks (rmsnorm / rope / swiglu)"),
                   ("swiglu", "decoder blocks (rmsnorm / rope / swiglu)"), ("gemm_skinny", "skinny GEMM (Bayesian layers)"), ("fused_small", "fused_small (Bayesian layers)"),
                   ("sample", "sampling (Bayesian layers)"), ("reduce_logprob", "sampling (Bayesian layers)"),
                   ("gemm", "tiled GEMM (Bayesian layers)"), ("attention", "attention"), ("predictive", "predictive statistics")):
        if key in name:
            return k
    return "other kernels"


def analyze(path, steps):
    with open(path) as f:
        ks = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(f)))
    # the last two gaps of over 1.5 s between kernels are the pauses: warm-up | prefill | prefill + decode steps
    a, b = [i for i in range(1, len(ks)) if ks[i][0] - ks[i - 1][1] > 1.5e9][-2:]
    parts = [ks[a:b], ks[b:]]

    def summary(part):
        busy, by = 0, {}
        for s, e, n in part:
            busy += e - s
            by[_klass(n)] = by.get(_klass(n), 0) + e - s
        return part[-1][1] - part[0][0], busy, by

    (w1, b1, by1), (w2, b2, by2) = summary(parts[0]), summary(parts[1])
    out = {"decode_steps": steps, "step_wall_us": round((w2 - w1) / steps / 1e3, 1),
           "step_kernel_us": round((b2 - b1) / steps / 1e3, 1)}
    out["step_host_gap_us"] = round(out["step_wall_us"] - out["step_kernel_us"], 1)
    out["per_class_us"] = {k: round((by2.get(k, 0) - by1.get(k, 0)) / steps / 1e3, 1) for k in sorted(set(by1) | set(by2))}
    out["kernels_per_step"] = round((len(parts[1]) - len(parts[0])) / steps, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernels", "e2e", "trace", "analyze"])
    ap.add_argument("path", nargs="?")
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--new-tokens", type=int, default=256)
    # keep | draw: the weights (trace); dynamic | static | graph: the decode path (e2e: the ones to alternate; trace: one)
    ap.add_argument("--mode", choices=["keep", "draw", "dynamic", "static", "graph"], action="append", default=None)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--top-k", type=int, default=None)
    ap.add_argument("--top-p", type=float, default=None)
    ap.add_argument("--min-p", type=float, default=None)
    ap.add_argument("--repetition-penalty", type=float, default=None)
    ap.add_argument("--no-repeat-ngram", type=int, default=None)
    ap.add_argument("--min-new-tokens", type=int, default=None)
    ap.add_argument("--eos-token-id", type=int, default=None)
    ap.add_argument("--fuse-blocks", action="store_true")
    ap.add_argument("--kv-cache", choices=["fp8"], default=None)
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--samples", type=int, default=4)
    a = ap.parse_args()
    processors = {k: v for k, v in (("repetition_penalty", a.repetition_penalty), ("no_repeat_ngram_size", a.no_repeat_ngram),
                                    ("min_new_tokens", a.min_new_tokens), ("eos_token_id", a.eos_token_id))
                  if v is not None}
    if a.what == "analyze":
        res = analyze(a.path, a.steps)
    else:
        assert torch.cuda.is_available(), "this benchmark measures the GPU"
        modes = a.mode or []
        paths = [m for m in modes if m in PATHS] or None
        if a.what == "kernels":
            res = block_kernels() if a.fuse_blocks else kernels(tuple(int(v) for v in a.only.split(",")) if a.only else None)
        elif a.what == "e2e" and a.kv_cache:
            res = e2e_kv_cache(a.runs, a.new_tokens, a.prompt, a.batch, a.samples)
        elif a.what == "e2e":
            truncation = {k: v for k, v in (("top_k", a.top_k), ("top_p", a.top_p), ("min_p", a.min_p)) if v is not None}
            res = e2e(a.runs, a.new_tokens, paths or ("dynamic", "static", "graph"), truncation, processors, a.fuse_blocks)
        else:
            trace("draw" if "draw" in modes else "keep", a.steps + 1, (paths or ["dynamic"])[-1], processors, a.fuse_blocks)
            return
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
