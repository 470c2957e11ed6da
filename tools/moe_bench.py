#!/usr/bin/env python
"""Measure the Bayesian mixture-of-experts kernels (bnn.Experts, include/bayeformers_amd_moe.h) against the framework's expert
loop on one MI355X.

    python tools/moe_bench.py [--out profiles/bayesian_moe.json] [--quick] [--skip-generate]

What is timed (device events around `iters` calls, after a warm-up of every shape; the two sides of a comparison alternate
round by round in one process, and the median with the min .. max spread over the rounds is reported):
  layers    the forward of ONE layer on the SAME sampled weights, kernel route (ops.moe_forward: bf_moe_route, _gate_up, _down,
            _combine) against the framework loop (ops.moe_composite: per sample and hit expert a gather, two F.linear calls,
            the activation, the scaling and an index_add; it reads the hit experts back to the host).  A Mixtral-shaped layer
            (E 8, k 2, H 4096, I 14336) and a Qwen3-MoE-shaped one (E 128, k 8, H 2048, I 768), S 4, decode-like (2 rows per
            sample) and prefill-like (1024 rows per sample).  The kernel route is also timed as a replayed HIP graph, where
            the host's launches do not count; the loop cannot be captured.  Launches per layer are counted by the profiler.
  stages    every entry of the kernel route alone, with the bytes it must move and the bytes/s it reaches
  generate  tokens/s of sample_generate on the decoder of DESIGN 4.5 (8 layers, hidden 1024, 16 / 4 heads, vocab 32000) given
            experts (E 8, k 2, I 2048), converted with experts=True: default, keep_weights=True, static cache and graph=True
Nothing is compared with a number from another run.  Needs a ROCm device; there is no CPU path."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bayeformers_amd as bf  # noqa: E402
from bayeformers_amd import ops  # noqa: E402

BF = torch.bfloat16
SILU = torch.nn.functional.silu


def time_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def alternate(fns, iters, rounds, warm=2):
    """{name: (median ms, min ms, max ms)} of each callable, the callables taking turns round by round."""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    got = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            got[k].append(time_ms(fn, iters))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in got.items()}


def fmt(t):
    return f"{t[0] * 1e3:10.1f} us ({t[1] * 1e3:.1f} .. {t[2] * 1e3:.1f})"


def launches(fn):
    """Device kernels one call of `fn` launches, as the profiler counts them."""
    from torch.profiler import ProfilerActivity, profile

    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
               and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())


def launches_or_none(fn):
    try:
        return launches(fn)
    except Exception as err:  # (a profiler that cannot trace here: the timings stand without the count)
        print(f"    (launch count not taken: {type(err).__name__}: {err})", flush=True)
        return None


def host_waits(fn):
    """Synchronising framework calls (read-backs to the host) one call of `fn` makes (torch's sync debug mode)."""
    import warnings

    fn()
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    return sum("synchroniz" in str(w.message).lower() for w in seen)


def problem(S, M, E, k, H, I, seed=1):
    g = torch.Generator(device="cuda").manual_seed(seed)
    R = S * M
    x = torch.randn(R, H, generator=g, device="cuda").to(BF)
    w_gu = (torch.randn(S, E, 2 * I, H, generator=g, device="cuda", dtype=BF) / H ** 0.5)
    w_d = (torch.randn(S, E, H, I, generator=g, device="cuda", dtype=BF) / I ** 0.5)
    wts, idx = torch.topk(torch.softmax(torch.randn(R, E, generator=g, device="cuda"), -1), k, dim=-1)
    wts = wts / wts.sum(-1, keepdim=True)
    return x, idx.contiguous(), wts.contiguous(), w_gu, w_d


def graphed(fn):
    """`fn` captured once on a side stream's warm-up, returned as a replay."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g.replay


def bench_layers(shapes, rounds, out):
    rows = []
    for name, S, M, E, k, H, I, iters in shapes:
        x, idx, wts, w_gu, w_d = problem(S, M, E, k, H, I)
        kern = lambda: ops.moe_forward(x, idx, wts, w_gu, w_d, S, SILU)
        loop = lambda: ops.moe_composite(x, idx, wts, w_gu, w_d, S, SILU)
        assert ops.moe_supported(BF, H, I, E, k, SILU, x, w_gu, w_d, S=S)
        a, b = kern().float(), loop().float()
        diff = (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)  # two 16-bit routes of one function
        t = alternate({"kernels": kern, "loop": loop, "kernels_graph": graphed(kern)}, iters, rounds)
        n_kern, n_loop = launches_or_none(kern), launches_or_none(loop)
        waits = {"kernels": host_waits(kern), "loop": host_waits(loop)}
        hit = int((torch.bincount((torch.arange(S * M, device="cuda")[:, None] // M * E + idx).reshape(-1),
                                  minlength=S * E) > 0).sum())
        weight_bytes = hit * 3 * I * H * 2  # the weights of the (sample, expert) pairs that were hit, read once
        row = {"layer": name, "S": S, "rows_per_sample": M, "E": E, "k": k, "H": H, "I": I, "groups_hit": hit,
               "forward_ms": t, "launches": {"kernels": n_kern, "loop": n_loop}, "host_waits": waits, "kernels_over_loop": t["kernels"][0] / t["loop"][0],
               "graph_over_loop": t["kernels_graph"][0] / t["loop"][0], "max_rel_difference": diff,
               "weight_bytes_hit": weight_bytes, "graph_weight_bytes_per_s": weight_bytes / (t["kernels_graph"][0] * 1e-3)}
        rows.append(row)
        print(f"{name} S={S} M={M}: kernels {fmt(t['kernels'])} [{n_kern} launches] | graph replay {fmt(t['kernels_graph'])} | "
              f"loop {fmt(t['loop'])} [{n_loop} launches, {waits['loop']} host waits against {waits['kernels']}] | kernels/loop {row['kernels_over_loop']:.2f}x, graph/loop "
              f"{row['graph_over_loop']:.2f}x | {hit} groups hit, {weight_bytes / 1e9:.2f} GB of weights, "
              f"{row['graph_weight_bytes_per_s'] / 1e12:.2f} TB/s in the replay | rel diff {diff:.1e}", flush=True)
        # the stages alone
        route = ops.moe_route(idx, S, E)
        h = ops.moe_gate_up(x, w_gu, route, k)
        y = ops.moe_down(h, w_d, route, k)
        st = alternate({"route": lambda: ops.moe_route(idx, S, E), "gate_up": lambda: ops.moe_gate_up(x, w_gu, route, k),
                        "down": lambda: ops.moe_down(h, w_d, route, k), "combine": lambda: ops.moe_combine(y, idx, wts, E, BF)},
                       iters, rounds)
        R = S * M
        moved = {"route": R * k * 8 * 2 + R * k * 4, "gate_up": hit * 2 * I * H * 2 + R * k * (H + I) * 2,
                 "down": hit * I * H * 2 + R * k * (I * 2 + H * 4), "combine": R * k * H * 4 + R * H * 2}
        row["stages_ms"] = st
        row["stages_bytes"] = moved
        print("    " + " | ".join(f"{n} {fmt(st[n])} {moved[n] / (st[n][0] * 1e-3) / 1e9:.0f} GB/s" for n in st), flush=True)
        del x, idx, wts, w_gu, w_d, h, y
        torch.cuda.empty_cache()
    out["layers"] = rows


def bench_generate(out, prompt, new, rounds):
    from transformers import MixtralConfig, MixtralForCausalLM

    from bayeformers_amd.sampling import sample_generate

    cfg = MixtralConfig(hidden_size=1024, intermediate_size=2048, num_local_experts=8, num_experts_per_tok=2,
                        num_attention_heads=16, num_key_value_heads=4, num_hidden_layers=8, vocab_size=32000,
                        max_position_embeddings=2048, sliding_window=None, tie_word_embeddings=False, attention_dropout=0.0,
                        attn_implementation="sdpa")
    torch.manual_seed(0)
    src = MixtralForCausalLM(cfg).eval()
    model = bf.to_bayesian(src, delta=0.05, freeze=True, experts=True).eval().cuda()
    freqs = {n: b.detach().clone() for n, b in model.named_buffers() if "inv_freq" in n}
    model = model.to(BF)
    for n, b in freqs.items():
        setattr(model.get_submodule(n.rsplit(".", 1)[0]), n.rsplit(".", 1)[1], b)
    del src
    assert bf.fuse_attention(model)
    bf.set_compute_dtype("bf16")
    S, B = 4, 4
    ids = torch.randint(0, 32000, (B, prompt), generator=torch.Generator().manual_seed(3)).cuda()
    modes = {"default": {}, "keep_weights": {"keep_weights": True}, "static_keep": {"static_cache": True, "keep_weights": True},
             "graph_keep": {"graph": True, "keep_weights": True}, "graph_draw": {"graph": True}}

    def run(kw):
        bf.manual_seed(7)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            gen = sample_generate(model, ids, samples=S, max_new_tokens=new, **kw)
        torch.cuda.synchronize()
        return B * new / (time.perf_counter() - t0), gen

    res, texts = {k: [] for k in modes}, {}
    for k, kw in modes.items():
        run(kw)  # warm-up of the mode
    for _ in range(rounds):
        for k, kw in modes.items():
            tps, gen = run(kw)
            res[k].append(tps)
            texts[k] = gen.sequences
    rows = {k: (statistics.median(v), min(v), max(v)) for k, v in res.items()}
    same = {k: bool(torch.equal(texts[k], texts["default"])) for k in modes}
    out["generate"] = {"S": S, "B": B, "prompt": prompt, "new_tokens": new, "kept_weight_bytes": bf.kept_weight_bytes(model, S, BF),
                       "tokens_per_s": rows, "same_text_as_default": same}
    for k, v in rows.items():
        print(f"generate {k:13s}: {v[0]:8.1f} tokens/s ({v[1]:.1f} .. {v[2]:.1f}); same text as default: {same[k]}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="small shapes, few rounds: a rehearsal of the script, not a measurement")
    ap.add_argument("--skip-generate", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "moe_bench needs a ROCm device"
    out = {"device": torch.cuda.get_device_name(0), "dtype": "bf16"}
    if args.quick:
        shapes = [("mixtral-like", 2, 2, 4, 2, 256, 512, 5), ("qwen3moe-like", 2, 64, 16, 4, 128, 64, 5)]
        rounds = 2
    else:
        shapes = [("mixtral", 4, 2, 8, 2, 4096, 14336, 20), ("mixtral", 4, 1024, 8, 2, 4096, 14336, 3),
                  ("qwen3moe", 4, 2, 128, 8, 2048, 768, 20), ("qwen3moe", 4, 1024, 128, 8, 2048, 768, 3)]
        rounds = 5
    bench_layers(shapes, rounds, out)
    if not args.skip_generate:
        bench_generate(out, 32 if args.quick else 128, 8 if args.quick else 64, 1 if args.quick else 3)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
        print("wrote", args.out)


if __name__ == "__main__":
    main()
