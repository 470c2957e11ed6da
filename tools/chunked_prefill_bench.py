"""Chunked prefill: what sample_generate(prefill_chunk=C) costs and saves, and the chunk kernels against the routes they
replace, in one process.

    python tools/chunked_prefill_bench.py [--prefill] [--kernels] [--prompts 3840,16384] [--iters N] [--runs N] [--out R.json]

Prefill: the DESIGN 4.5 decoder (8 layers, hidden 1024, 16 / 4 heads of size 64, vocabulary 32000), S 4, B 2, one new
token (the call is its prefill), keep_weights=True; the whole prompt against chunks of 512 and 2048, on the default path
(DynamicCache), static_cache=True and kv_cache="fp8".  Per run: torch.cuda.max_memory_allocated over the call minus what
was allocated before it, and device-event time; one warm-up call per setting, then the median of `runs`, the settings
interleaved.  Step-0 statistics of each chunked run are compared with the whole-prompt run's.
Kernels: N 8, H / Hkv 16 / 4, Tq new queries against a cache filled to L (capacity L: the route it replaces reads the
whole capacity either way), with and without a window of 1024: bf_attention_chunk_gqa against the framework's SDPA over
the dense [N, 1, Tq, L] bool mask, and bf_attention_chunk_gqa_kv8 against kv8_dequantize of the whole cache + that SDPA.
Device events around each call, median of `iters`, best of 3 interleaved rounds; every result is checked against SDPA first.
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


def timed(fn, iters):
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    return statistics.median(ts), (max(ts) - min(ts)) / statistics.median(ts)


def best(res, rounds, iters):
    out = {k: [] for k in res}
    for _ in range(rounds):
        for key, fn in res.items():
            out[key].append(timed(fn, iters))
    return {k: min(v) for k, v in out.items()}


def rel(a, b):
    return ((a.float() - b.float()).abs().max() / b.float().abs().max()).item()


def _decoder(max_pos):
    from transformers import LlamaConfig, LlamaForCausalLM

    import bayeformers_amd as bf

    cfg = LlamaConfig(hidden_size=1024, num_attention_heads=16, num_key_value_heads=4, num_hidden_layers=8,
                      intermediate_size=2816, vocab_size=32000, max_position_embeddings=max_pos, tie_word_embeddings=False,
                      attention_dropout=0.0, attn_implementation="sdpa")
    torch.manual_seed(0)
    bmodel = bf.to_bayesian(LlamaForCausalLM(cfg).eval(), delta=0.05, freeze=True).eval().cuda()
    freqs = {n: b.detach().clone() for n, b in bmodel.named_buffers() if "inv_freq" in n}
    bmodel = bmodel.to(torch.bfloat16)
    for n, b in freqs.items():
        setattr(bmodel.get_submodule(n.rsplit(".", 1)[0]), n.rsplit(".", 1)[1], b)
    assert bf.fuse_attention(bmodel)
    bf.set_compute_dtype("bf16")
    return bmodel


STATS = ("predictive_entropy", "expected_entropy", "mutual_information", "token_prob")


def prefill(prompts, runs, S=4, B=2):
    import bayeformers_amd as bf
    from bayeformers_amd.sampling import sample_generate

    bmodel = _decoder(max(prompts) + 8)
    rows = []
    paths = {"dynamic": {}, "static": {"static_cache": True}, "fp8": {"kv_cache": "fp8"}}
    for T0 in prompts:
        ids = torch.randint(0, 32000, (B, T0), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
        mask = torch.ones_like(ids)
        mask[B - 1, :T0 // 16] = 0  # one left-padded row
        settings = [(p, c) for p in paths for c in (None, 512, 2048) if c is None or c < T0]

        def run(path, chunk):
            bf.manual_seed(0x5EED)
            with torch.no_grad():
                return sample_generate(bmodel, ids, attention_mask=mask, samples=S, max_new_tokens=1, keep_weights=True,
                                       prefill_chunk=chunk, **paths[path])

        res = {s: {"peak": [], "s": []} for s in settings}
        gens = {}
        for s in settings:  # warm-up: plans, workspaces
            run(*s)
        for _ in range(runs):
            for s in settings:
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                gens[s] = run(*s)
                b.record()
                b.synchronize()
                res[s]["peak"].append(torch.cuda.max_memory_allocated() - base)
                res[s]["s"].append(a.elapsed_time(b) * 1e-3)
        for (path, chunk), r in res.items():
            whole = gens[(path, None)]
            row = {"S": S, "B": B, "T0": T0, "path": path, "prefill_chunk": chunk,
                   "peak_MiB": round(statistics.median(r["peak"]) / 2 ** 20, 1),
                   "ms": round(statistics.median(r["s"]) * 1e3, 2), "ms_min": round(min(r["s"]) * 1e3, 2),
                   "ms_max": round(max(r["s"]) * 1e3, 2),
                   "step0_max_abs_diff_vs_whole": max((getattr(whole, n)[:, 0] - getattr(gens[(path, chunk)], n)[:, 0])
                                                      .abs().max().item() for n in STATS),
                   "same_first_token": bool(torch.equal(whole.sequences, gens[(path, chunk)].sequences))}
            rows.append(row)
            print(json.dumps(row), flush=True)
        del gens
    return rows


def kernels(iters, N=8, H=16, Hkv=4):
    from transformers.integrations.sdpa_attention import sdpa_attention_forward

    from bayeformers_amd import ops

    rows = []
    mod = types.SimpleNamespace(is_causal=True, num_key_value_groups=H // Hkv, training=False)
    for D in (64, 128, 256):
        scale = D ** -0.5
        for L in (4096, 16384):
            g = torch.Generator(device="cuda").manual_seed(D + L)
            k = torch.randn(N, Hkv, L, D, device="cuda", generator=g, dtype=torch.bfloat16)
            v = torch.randn(N, Hkv, L, D, device="cuda", generator=g, dtype=torch.bfloat16)
            kq, vq = (torch.zeros(N, Hkv, L, D, dtype=torch.uint8, device="cuda") for _ in range(2))
            ks, vs = (torch.zeros(N, Hkv, L, device="cuda") for _ in range(2))
            ops.kv8_append(k, v, kq, vq, ks, vs, torch.zeros(1, dtype=torch.long, device="cuda"))
            kv_len = torch.tensor([L], device="cuda")
            for Tq in (512, 2048):
                q = torch.randn(N, Tq, H, D, device="cuda", generator=g, dtype=torch.bfloat16).transpose(1, 2)
                for W in (None, 1024):
                    i = (L - Tq + torch.arange(Tq, device="cuda"))[:, None]
                    j = torch.arange(L, device="cuda")[None, :]
                    seen = j <= i
                    if W is not None:
                        seen = seen & (i - j < W)
                    mask = seen[None, None].expand(N, 1, Tq, L)

                    def sdpa(kk=k, vv=v):
                        return sdpa_attention_forward(mod, q, kk, vv, mask, dropout=0.0, scaling=scale)[0]

                    def sdpa8():
                        return sdpa(ops.kv8_dequantize(kq, ks), ops.kv8_dequantize(vq, vs))

                    err = rel(ops.attention_forward_chunk(q, k, v, kv_len, None, scale, window=W), sdpa())
                    err8 = rel(ops.attention_forward_chunk_kv8(q, kq, vq, ks, vs, kv_len, None, scale, window=W), sdpa8())
                    t = best({
                        "chunk": lambda: ops.attention_forward_chunk(q, k, v, kv_len, None, scale, window=W),
                        "sdpa_dense_mask": sdpa,
                        "chunk_kv8": lambda: ops.attention_forward_chunk_kv8(q, kq, vq, ks, vs, kv_len, None, scale, window=W),
                        "dequantize_sdpa": sdpa8,
                    }, 3, iters)
                    keys = L - Tq if W is None else min(W, L - Tq)  # visible pairs: a trapezoid
                    pairs = Tq * keys + Tq * (Tq + 1) // 2 if W is None else sum(min(W, L - Tq + a + 1) for a in range(Tq))
                    row = {"N": N, "H": H, "Hkv": Hkv, "D": D, "L": L, "Tq": Tq, "W": W,
                           "max_rel_err_vs_sdpa": round(err, 5), "kv8_max_rel_err_vs_sdpa": round(err8, 5)}
                    for key, (s, spread) in t.items():
                        row[key] = {"ms": round(s * 1e3, 4), "spread": round(spread, 3),
                                    "tflops": round(4 * D * pairs * N * H / s / 1e12, 1)}
                    row["sdpa_over_chunk"] = round(t["sdpa_dense_mask"][0] / t["chunk"][0], 2)
                    row["dequantize_sdpa_over_chunk_kv8"] = round(t["dequantize_sdpa"][0] / t["chunk_kv8"][0], 2)
                    rows.append(row)
                    print(json.dumps(row), flush=True)
                    del mask
            del k, v, kq, vq
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prefill", action="store_true")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--prompts", default="3840,16384")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU"
    if not (a.prefill or a.kernels):
        a.prefill = a.kernels = True
    res = {}
    if a.kernels:
        res["kernels"] = kernels(a.iters)
    if a.prefill:
        res["prefill"] = prefill([int(t) for t in a.prompts.split(",")], a.runs)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
