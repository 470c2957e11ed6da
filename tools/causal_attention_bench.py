"""Causal / grouped-query attention timings: the kernels against torch's scaled_dot_product_attention
(is_causal=True, enable_gqa=True), interleaved in one process, and a Bayesian decoder's Monte-Carlo forward with and
without fuse_attention.

    python tools/causal_attention_bench.py [--kernels] [--model] [--iters N]

Kernel shapes (S*B, H, Hkv, D, T): (a) 16, 16, 4, 64, 1024; (b) 8, 32, 8, 128, 2048; (c) the non-causal kernel at (a).
Causal forward flops = 2 * 2 * D * T * (T + 1) / 2 per (sequence, head) (QK^T and PV over the visible half), the
backward 2.5x that; the non-causal forward 4 * D * T^2.  Peak: 2.5 PFLOP/s dense bf16.  Times here are host-timed events
around each launch sequence (median); kernel-only times come from a rocprofv3 --kernel-trace --stats run of the same
script.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 2.5e15
SHAPES = {"a": (16, 16, 4, 64, 1024, True), "b": (8, 32, 8, 128, 2048, True), "c": (16, 16, 4, 64, 1024, False)}


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


def kernels(iters):
    from bayeformers_amd import ops

    rows = []
    for name, (B, H, Hkv, D, T, causal) in SHAPES.items():
        g = torch.Generator(device="cuda").manual_seed(0)
        q = torch.randn(B, T, H * D, device="cuda", generator=g, dtype=torch.bfloat16).view(B, T, H, D).transpose(1, 2)
        k, v = (torch.randn(B, T, Hkv * D, device="cuda", generator=g, dtype=torch.bfloat16).view(B, T, Hkv, D).transpose(1, 2)
                for _ in range(2))
        go = torch.randn(B, T, H, D, device="cuda", generator=g, dtype=torch.bfloat16)
        scale = D ** -0.5
        out, lse = ops.attention_forward_gqa(q, k, v, None, scale, causal, want_lse=True)
        qs, ks, vs = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
        ref = torch.nn.functional.scaled_dot_product_attention(qs, ks, vs, is_causal=causal, enable_gqa=True, scale=scale)
        fwd_flops = B * H * (2 * D * T * (T + 1) if causal else 4 * D * T * T)
        res = {"ours_fwd": [], "sdpa_fwd": [], "ours_bwd": [], "sdpa_bwd": []}
        for _ in range(3):  # interleaved rounds
            res["ours_fwd"].append(timed(lambda: ops.attention_forward_gqa(q, k, v, None, scale, causal, want_lse=True), iters))
            res["sdpa_fwd"].append(timed(lambda: torch.nn.functional.scaled_dot_product_attention(
                q, k, v, is_causal=causal, enable_gqa=True, scale=scale), iters))
            res["ours_bwd"].append(timed(lambda: ops.attention_backward_gqa(q, k, v, None, None, out, go, lse, scale, causal), iters))
            res["sdpa_bwd"].append(timed(lambda: torch.autograd.grad(ref, (qs, ks, vs), go.transpose(1, 2), retain_graph=True), iters))
        row = {"shape": name, "B": B, "H": H, "Hkv": Hkv, "D": D, "T": T, "causal": causal}
        for key, vals in res.items():
            t = min(vals)
            flops = fwd_flops * (2.5 if key.endswith("bwd") else 1.0)
            row[key] = {"ms": round(t * 1e3, 4), "tflops": round(flops / t / 1e12, 1), "peak_frac": round(flops / t / PEAK, 3)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def model(iters):
    from transformers import LlamaConfig, LlamaForCausalLM

    import bayeformers_amd as bf
    from bayeformers_amd.sampling import elbo, sample_bayesian

    cfg = LlamaConfig(hidden_size=1024, num_attention_heads=16, num_key_value_heads=4, num_hidden_layers=8,
                      intermediate_size=2816, vocab_size=32000, max_position_embeddings=1024, tie_word_embeddings=False,
                      use_cache=False, attn_implementation="sdpa")
    S, B, T = 4, 4, 1024
    torch.manual_seed(0)
    bmodel = bf.to_bayesian(LlamaForCausalLM(cfg).eval(), delta=0.05, freeze=True).eval().cuda()
    freqs = {n: b.detach().clone() for n, b in bmodel.named_buffers() if "inv_freq" in n}
    bmodel = bmodel.to(torch.bfloat16)
    for n, b in freqs.items():
        setattr(bmodel.get_submodule(n.rsplit(".", 1)[0]), n.rsplit(".", 1)[1], b)
    ids = torch.randint(0, cfg.vocab_size, (B, T), device="cuda")
    mask = torch.ones(B, T, dtype=torch.long, device="cuda")
    labels = ids[:, 1:].reshape(-1)
    inputs = {"input_ids": ids, "attention_mask": mask, "use_cache": False}

    def step():
        with torch.no_grad():
            raw, mean, lp, lq = sample_bayesian(bmodel, inputs, S)
            nll = torch.nn.functional.cross_entropy(mean[0][:, :-1].reshape(-1, cfg.vocab_size).float(), labels)
            return elbo(lp, lq, nll.double(), 1000)

    bf.manual_seed(0x5EED)
    out = {}
    for label in ("sdpa", "fused"):
        if label == "fused":
            assert bf.fuse_attention(bmodel)
        for _ in range(2):
            step()
        t = timed(step, iters)
        out[label] = {"step_ms": round(t * 1e3, 2), "mc_samples_per_s": round(S / t, 2)}
        print(json.dumps({"model": label, **out[label]}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--model", action="store_true")
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    if not (a.kernels or a.model):
        a.kernels = a.model = True
    if a.kernels:
        kernels(a.iters)
    if a.model:
        model(max(3, a.iters // 4))


if __name__ == "__main__":
    main()
