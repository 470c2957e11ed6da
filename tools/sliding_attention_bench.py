"""Sliding-window attention timings: the window kernels against the framework's SDPA with the dense sliding mask (what a
sliding layer ran before them) and against our full causal kernel, interleaved in one process; and sample_generate on a
Mistral-shaped Bayesian decoder whose window is shorter than prompt + new tokens (dynamic, static and graph paths).

    python tools/sliding_attention_bench.py [--kernels] [--decode] [--generate] [--iters N] [--out R.json]

Prefill (S*B, H, Hkv, D, T, W): S*B 8, H 32, Hkv 8, T 8192, D 128 and D 64, W in {4096, 1024, 256}; forward and backward.
Decode: S*B 8, H 32 / Hkv 8, D 128, Tk 32768, W 4096, Tq in {1, 8}: bf_attention_decode_gqa_window and its fixed-capacity
form (_len, L = Tk) against the plain entries over all Tk keys and SDPA with the dense mask.  Times: device events around
each call, median of `iters`, best of 3 interleaved rounds.  Every window result is checked against SDPA on the same inputs
before it is timed.  Flops of a window forward: 4 * D * (visible (query, key) pairs) per (sequence, head), the backward 2.5x.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 2.5e15
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


def visible_pairs(T, W):
    """query / key pairs with 0 <= i - j < W over T queries"""
    W = min(W, T)
    return W * (W + 1) // 2 + (T - W) * W


def dense_mask(Tq, Tk, W):
    i = (Tk - Tq + torch.arange(Tq, device="cuda"))[:, None]
    j = torch.arange(Tk, device="cuda")[None, :]
    return ((j <= i) & (i - j < W))[None, None]


def rel(a, b):
    return ((a.float() - b.float()).abs().max() / b.float().abs().max()).item()


def best(res, rounds, iters):
    out = {k: [] for k in res}
    for _ in range(rounds):
        for key, fn in res.items():
            out[key].append(timed(fn, iters))
    return {k: min(v) for k, v in out.items()}


def kernels(iters):
    from bayeformers_amd import ops

    rows = []
    for D in (128, 64):
        B, H, Hkv, T = 8, 32, 8, 8192
        g = torch.Generator(device="cuda").manual_seed(0)
        q = torch.randn(B, T, H * D, device="cuda", generator=g, dtype=torch.bfloat16).view(B, T, H, D).transpose(1, 2)
        k, v = (torch.randn(B, T, Hkv * D, device="cuda", generator=g, dtype=torch.bfloat16).view(B, T, Hkv, D).transpose(1, 2)
                for _ in range(2))
        go = torch.randn(B, T, H, D, device="cuda", generator=g, dtype=torch.bfloat16)
        scale = D ** -0.5
        full_out, full_lse = ops.attention_forward_gqa(q, k, v, None, scale, True, want_lse=True)
        for W in (4096, 1024, 256):
            out, lse = ops.attention_forward_gqa(q, k, v, None, scale, True, want_lse=True, window=W)
            mask = dense_mask(T, T, W)
            qs, ks, vs = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
            ref = torch.nn.functional.scaled_dot_product_attention(qs, ks, vs, attn_mask=mask, enable_gqa=True, scale=scale)
            err = rel(out, ref.transpose(1, 2))
            t = best({
                "window_fwd": lambda: ops.attention_forward_gqa(q, k, v, None, scale, True, want_lse=True, window=W),
                "sdpa_fwd": lambda: torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=mask, enable_gqa=True,
                                                                                     scale=scale),
                "causal_fwd": lambda: ops.attention_forward_gqa(q, k, v, None, scale, True, want_lse=True),
                "window_bwd": lambda: ops.attention_backward_gqa(q, k, v, None, None, out, go, lse, scale, True, window=W),
                "sdpa_bwd": lambda: torch.autograd.grad(ref, (qs, ks, vs), go.transpose(1, 2), retain_graph=True),
                "causal_bwd": lambda: ops.attention_backward_gqa(q, k, v, None, None, full_out, go, full_lse, scale, True),
            }, 3, iters)
            flops = 4 * D * visible_pairs(T, W) * B * H
            row = {"B": B, "H": H, "Hkv": Hkv, "D": D, "T": T, "W": W, "max_rel_err_vs_sdpa": round(err, 5)}
            for key, s in t.items():
                f = flops * (2.5 if key.endswith("bwd") else 1.0)
                row[key] = {"ms": round(s * 1e3, 4), "window_tflops": round(f / s / 1e12, 1),
                            "window_peak_frac": round(f / s / PEAK, 3)}
            rows.append(row)
            print(json.dumps(row), flush=True)
            del ref, qs, ks, vs, mask
        del q, k, v, go
    return rows


def decode(iters):
    from transformers.integrations.sdpa_attention import sdpa_attention_forward
    import types

    from bayeformers_amd import ops

    rows = []
    N, H, Hkv, D, Tk, W = 8, 32, 8, 128, 32768, 4096
    k = torch.randn(N, Hkv, Tk, D, device="cuda", dtype=torch.bfloat16)
    v = torch.randn(N, Hkv, Tk, D, device="cuda", dtype=torch.bfloat16)
    L = torch.tensor([Tk], device="cuda")
    for Tq in (1, 8):
        q = torch.randn(N, Tq, H, D, device="cuda", dtype=torch.bfloat16).transpose(1, 2)
        scale = D ** -0.5
        mod = types.SimpleNamespace(is_causal=True, num_key_value_groups=H // Hkv, training=False)
        mask = dense_mask(Tq, Tk, W).expand(N, 1, Tq, Tk)
        ws = torch.empty(max(ops.attention_decode_workspace_bytes(q, k, v), 16), dtype=torch.uint8, device="cuda")
        out = ops.attention_forward_decode(q, k, v, None, scale, workspace=ws, window=W)
        ref = sdpa_attention_forward(mod, q, k, v, mask, dropout=0.0, scaling=scale)[0]
        err = rel(out, ref)
        err_len = rel(ops.attention_forward_decode_len(q, k, v, L, None, scale, workspace=ws, window=W), ref)
        t = best({
            "window": lambda: ops.attention_forward_decode(q, k, v, None, scale, workspace=ws, window=W),
            "window_len": lambda: ops.attention_forward_decode_len(q, k, v, L, None, scale, workspace=ws, window=W),
            "full": lambda: ops.attention_forward_decode(q, k, v, None, scale, workspace=ws),
            "full_len": lambda: ops.attention_forward_decode_len(q, k, v, L, None, scale, workspace=ws),
            "sdpa_dense_mask": lambda: sdpa_attention_forward(mod, q, k, v, mask, dropout=0.0, scaling=scale),
        }, 3, iters)
        kv_bytes = 2 * N * Hkv * (W + Tq - 1) * D * 2
        row = {"SB": N, "H": H, "Hkv": Hkv, "D": D, "Tk": Tk, "W": W, "Tq": Tq, "max_rel_err_vs_sdpa": round(err, 5),
               "max_rel_err_len_vs_sdpa": round(err_len, 5)}
        for key, s in t.items():
            row[key] = {"us": round(s * 1e6, 2), "window_bytes_hbm_frac": round(kv_bytes / s / HBM, 3)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def generate(runs, new_tokens):
    from transformers import MistralConfig, MistralForCausalLM

    import bayeformers_amd as bf
    from bayeformers_amd.sampling import sample_generate

    cfg = MistralConfig(hidden_size=1024, num_attention_heads=16, num_key_value_heads=4, num_hidden_layers=8,
                        intermediate_size=2816, vocab_size=32000, max_position_embeddings=4096, sliding_window=256,
                        tie_word_embeddings=False, attention_dropout=0.0, attn_implementation="sdpa")
    torch.manual_seed(0)
    bmodel = bf.to_bayesian(MistralForCausalLM(cfg).eval(), delta=0.05, freeze=True).eval().cuda()
    freqs = {n: b.detach().clone() for n, b in bmodel.named_buffers() if "inv_freq" in n}
    bmodel = bmodel.to(torch.bfloat16)
    for n, b in freqs.items():
        setattr(bmodel.get_submodule(n.rsplit(".", 1)[0]), n.rsplit(".", 1)[1], b)
    assert bf.fuse_attention(bmodel)
    bf.set_compute_dtype("bf16")
    ids = torch.randint(0, 32000, (4, 512), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    modes = {"dynamic": {}, "static": {"static_cache": True}, "graph": {"graph": True}}
    res = {m: [] for m in modes}
    seqs = {}
    with torch.no_grad():
        for m, kw in modes.items():  # warm-up
            sample_generate(bmodel, ids, samples=4, max_new_tokens=8, keep_weights=True, **kw)
        for _ in range(runs):
            for m, kw in modes.items():
                bf.manual_seed(0x5EED)  # the same posterior draws on every path: the texts are comparable
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                gen = sample_generate(bmodel, ids, samples=4, max_new_tokens=new_tokens, keep_weights=True, **kw)
                torch.cuda.synchronize()
                res[m].append(4 * new_tokens / (time.perf_counter() - t0))
                seqs[m] = gen.sequences
    out = {m: {"tokens_per_s_median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}
           for m, v in res.items()}
    out["config"] = {"layers": 8, "hidden": 1024, "heads": "16/4", "W": 256, "S": 4, "B": 4, "prompt": 512,
                     "new_tokens": new_tokens, "keep_weights": True}
    out["static_equals_graph"] = bool(torch.equal(seqs["static"], seqs["graph"]))
    out["static_equals_dynamic"] = bool(torch.equal(seqs["static"], seqs["dynamic"]))
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--decode", action="store_true")
    ap.add_argument("--generate", action="store_true")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--new-tokens", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU"
    if not (a.kernels or a.decode or a.generate):
        a.kernels = a.decode = a.generate = True
    res = {}
    if a.kernels:
        res["prefill"] = kernels(a.iters)
    if a.decode:
        res["decode"] = decode(a.iters * 5)
    if a.generate:
        res["generate"] = generate(a.runs, a.new_tokens)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
