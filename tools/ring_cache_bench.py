"""The ring-buffer KV cache of sample_generate(sliding_cache="ring"): its decode entry against the window entry it stands in
for, its append against StaticLayer.update's index_copy_ pair, and sample_generate with and without it.

    python tools/ring_cache_bench.py [--out profiles/ring_kv_cache.json] [--md profiles/ring_kv_cache.md] [--new-tokens 1536]

Decode: bf_attention_decode_gqa_ring on a ring of W + 15 slots against bf_attention_decode_gqa_len_window on a linear cache
of L slots filled to L, the same L and W in one process (bf16, N 8, one query; H / Hkv 32 / 8 at D 128 and 8 / 4 at D 256).
Both are captured in a graph of 20 calls (the host is out) and alternated: 5 rounds of 3 windows of 10 replays each; the time
is the median of the rounds' medians and the spread (max - min) / median over the rounds.  The verdict of a class is "tie"
while the two times differ by no more than the larger spread.
Append: one bf_kv_ring_append launch against the arange + add + two index_copy_ launches of transformers'
StaticLayer.update (without its fill-pointer bump, which the ring layer pays too), per layer at T = 1, the same way.
End to end: the DESIGN §4.5 decoder as a Mistral (8 layers, hidden 1024, 16 / 4 heads of 64) with sliding_window 256, S 4, B 2,
prompt 512, graph=True, keep_weights=True, with and without sliding_cache="ring", in bf16 and with kv_cache="fp8": tokens/s
of one run after a warm-up run, the allocator's peak, and the cache's bytes (plan.kv_cache_bytes).
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _graph_of(fn, calls=20):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(calls):
            fn()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    return g


def _window(g, calls=20, replays=10):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(replays):
        g.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / (replays * calls)


def _alternate(fns, rounds=5, windows=3):
    """{name: (median us, spread)} of graph-replayed calls, the candidates alternated round by round"""
    graphs = {name: _graph_of(fn) for name, fn in fns.items()}
    per = {name: [] for name in fns}
    for _ in range(rounds):
        for name, g in graphs.items():
            per[name].append(statistics.median(_window(g) for _ in range(windows)))
    out = {}
    for name, ts in per.items():
        med = statistics.median(ts)
        out[name] = (med, (max(ts) - min(ts)) / med)
    del graphs
    return out


def _verdict(t_new, s_new, t_old, s_old):
    ratio = t_new / t_old
    if abs(ratio - 1.0) <= max(s_new, s_old):
        return "tie"
    return "LOSS" if ratio > 1.0 else "win"


def decode_classes():
    from bayeformers_amd import ops

    rows = []
    N = 8
    for H, Hkv, D in ((32, 8, 128), (8, 4, 256)):
        for W in (1024, 4096):
            for L in (4096, 16384, 32768):
                C = ops.ring_slots(W, L)
                if C is None:  # the ring would be the whole capacity: such a layer stays a plain one
                    continue
                g = torch.Generator().manual_seed(L + W + D)
                q = torch.randn(N, 1, H, D, generator=g).to("cuda", torch.bfloat16).transpose(1, 2)
                k, v = (torch.randn(N, Hkv, L, D, device="cuda", dtype=torch.bfloat16) for _ in range(2))
                slots = torch.arange(L - C, L, device="cuda") % C
                kr, vr = (torch.empty(N, Hkv, C, D, device="cuda", dtype=torch.bfloat16) for _ in range(2))
                kr[:, :, slots], vr[:, :, slots] = k[:, :, L - C:], v[:, :, L - C:]
                kv_len = torch.tensor([L], device="cuda")
                scale = D ** -0.5
                ws = torch.empty(max(ops.attention_decode_workspace_bytes(q, k, v), 16), dtype=torch.uint8, device="cuda")
                fns = {"window": lambda: ops.attention_forward_decode_len(q, k, v, kv_len, None, scale, workspace=ws, window=W),
                       "ring": lambda: ops.attention_forward_decode_ring(q, kr, vr, kv_len, None, scale, None, ws, W, C, L)}
                same = bool(torch.equal(fns["window"](), fns["ring"]()))
                t = _alternate(fns)
                row = {"N": N, "H": H, "Hkv": Hkv, "D": D, "W": W, "L": L, "ring_slots": C, "same_bits": same,
                       "window_us": round(t["window"][0], 2), "window_spread": round(t["window"][1], 3),
                       "ring_us": round(t["ring"][0], 2), "ring_spread": round(t["ring"][1], 3),
                       "ring_over_window": round(t["ring"][0] / t["window"][0], 3),
                       "verdict": _verdict(t["ring"][0], t["ring"][1], t["window"][0], t["window"][1]),
                       "cache_mib_linear": round(2 * N * Hkv * L * D * 2 / 2 ** 20, 1),
                       "cache_mib_ring": round(2 * N * Hkv * C * D * 2 / 2 ** 20, 1)}
                rows.append(row)
                print(json.dumps(row), flush=True)
                del q, k, v, kr, vr, ws
                torch.cuda.empty_cache()
    return rows


def append_classes():
    from bayeformers_amd import ops

    rows = []
    N, W, capacity = 8, 4096, 32768
    C = ops.ring_slots(W, capacity)
    for Hkv, D in ((8, 128), (4, 256)):
        k_new, v_new = (torch.randn(N, 1, Hkv * D, device="cuda", dtype=torch.bfloat16).view(N, 1, Hkv, D).transpose(1, 2)
                        for _ in range(2))
        k, v = (torch.zeros(N, Hkv, capacity, D, device="cuda", dtype=torch.bfloat16) for _ in range(2))
        kr, vr = (torch.zeros(N, Hkv, C, D, device="cuda", dtype=torch.bfloat16) for _ in range(2))
        pos = torch.tensor(20000, device="cuda")

        def index_copy():  # transformers' StaticLayer.update, less its fill-pointer bump
            at = torch.arange(1, device="cuda") + pos
            k.index_copy_(2, at, k_new)
            v.index_copy_(2, at, v_new)

        t = _alternate({"index_copy": index_copy, "ring": lambda: ops.kv_ring_append(k_new, v_new, kr, vr, pos)})
        row = {"N": N, "Hkv": Hkv, "D": D, "T": 1, "index_copy_us": round(t["index_copy"][0], 2),
               "index_copy_spread": round(t["index_copy"][1], 3), "ring_us": round(t["ring"][0], 2),
               "ring_spread": round(t["ring"][1], 3), "ring_over_index_copy": round(t["ring"][0] / t["index_copy"][0], 3),
               "verdict": _verdict(t["ring"][0], t["ring"][1], t["index_copy"][0], t["index_copy"][1])}
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def end_to_end(new_tokens, window=256):
    from transformers import MistralConfig, MistralForCausalLM

    import bayeformers_amd as bf
    from bayeformers_amd.plan import kv_cache_bytes
    from bayeformers_amd.sampling import sample_generate

    S, B, T0 = 4, 2, 512
    cfg = MistralConfig(hidden_size=1024, num_attention_heads=16, num_key_value_heads=4, head_dim=64, num_hidden_layers=8,
                        intermediate_size=2816, vocab_size=32000, max_position_embeddings=T0 + new_tokens,
                        tie_word_embeddings=False, attention_dropout=0.0, attn_implementation="sdpa", sliding_window=window)
    torch.manual_seed(0)
    bmodel = bf.to_bayesian(MistralForCausalLM(cfg).eval(), delta=0.05, freeze=True).eval().cuda()
    freqs = {n: b.detach().clone() for n, b in bmodel.named_buffers() if "inv_freq" in n}
    bmodel = bmodel.to(torch.bfloat16)
    for n, b in freqs.items():
        setattr(bmodel.get_submodule(n.rsplit(".", 1)[0]), n.rsplit(".", 1)[1], b)
    assert bf.fuse_attention(bmodel)
    bf.set_compute_dtype("bf16")
    ids = torch.randint(0, 32000, (B, T0), generator=torch.Generator().manual_seed(1)).cuda()
    capacity = T0 + new_tokens - 1
    rows, texts = [], {}
    for fp8 in (None, "fp8"):
        for ring in (None, "ring"):
            kw = dict(samples=S, graph=True, keep_weights=True, kv_cache=fp8, sliding_cache=ring)
            with torch.no_grad():
                bf.manual_seed(7)
                sample_generate(bmodel, ids, max_new_tokens=8, **kw)  # warm-up
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                before = torch.cuda.memory_allocated()
                bf.manual_seed(7)
                t0 = time.perf_counter()
                gen = sample_generate(bmodel, ids, max_new_tokens=new_tokens, **kw)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
            texts[(fp8, ring)] = gen.sequences
            row = {"kv_cache": fp8 or "bf16", "sliding_cache": ring or "none", "S": S, "B": B, "prompt": T0,
                   "new_tokens": new_tokens, "window": window, "seconds": round(dt, 3),
                   "tokens_per_s": round(B * new_tokens / dt, 1),
                   "peak_mib_above_model": round((torch.cuda.max_memory_allocated() - before) / 2 ** 20, 1),
                   "cache_mib": round(kv_cache_bytes(bmodel, S, B, capacity, fp8=bool(fp8), ring=bool(ring)) / 2 ** 20, 1),
                   "same_text_as_without_ring": bool(torch.equal(gen.sequences, texts[(fp8, None)]))}
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def _table(rows, cols):
    lines = ["| " + " | ".join(cols) + " |", "|" + "---|" * len(cols)]
    lines += ["| " + " | ".join(str(r[c]) for c in cols) + " |" for r in rows]
    return "\n".join(lines)


def markdown(res):
    parts = ["# Ring-buffer KV cache for sliding-window layers (`sliding_cache=\"ring\"`)", "",
             "Written by `tools/ring_cache_bench.py` on one MI355X; the method is in its docstring.  Times are graph-replayed "
             "(the host is out), medians over alternated rounds; a spread is (max - min) / median over the rounds; a class "
             "is a tie while the ratio is within the larger spread of 1.", ""]
    if "decode" in res:
        parts += ["## Decode: `bf_attention_decode_gqa_ring` against `bf_attention_decode_gqa_len_window`", "",
                  "bf16, N 8, one query, the same L and W; `same_bits`: the two results are bitwise equal.", "",
                  _table(res["decode"], ["H", "Hkv", "D", "W", "L", "ring_slots", "window_us", "window_spread", "ring_us",
                                         "ring_spread", "ring_over_window", "verdict", "same_bits", "cache_mib_linear",
                                         "cache_mib_ring"]), ""]
    if "append" in res:
        parts += ["## Append: one `bf_kv_ring_append` launch against `StaticLayer.update`'s `index_copy_` pair", "",
                  "bf16, N 8, T 1, per layer (the framework route: `arange`, an add and two `index_copy_` launches).", "",
                  _table(res["append"], ["Hkv", "D", "index_copy_us", "index_copy_spread", "ring_us", "ring_spread",
                                         "ring_over_index_copy", "verdict"]), ""]
    if "end_to_end" in res:
        parts += ["## End to end: `sample_generate(graph=True, keep_weights=True)`", "",
                  "The DESIGN §4.5 decoder as a Mistral with `sliding_window` 256 on every layer; one run after a warm-up "
                  "run, so the tokens/s carry no spread of their own.  `peak_mib_above_model`: the allocator's peak during "
                  "the call above what was allocated before it.  The rows without the ring are the path as it was.", "",
                  _table(res["end_to_end"], ["kv_cache", "sliding_cache", "S", "B", "prompt", "new_tokens", "window",
                                             "tokens_per_s", "peak_mib_above_model", "cache_mib",
                                             "same_text_as_without_ring"]), ""]
    parts += ["## Not measured", "",
              "- Other batch sizes, more than one query a step, fp16, the soft-cap form and the FP8 ring's decode and append "
              "kernels on their own.",
              "- Windows other than 1024 and 4096 in the kernel classes and 256 end to end; a 32 k generation end to end.",
              "- The spread of the end-to-end tokens/s (one run each).", ""]
    return "\n".join(parts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    ap.add_argument("--new-tokens", type=int, default=1536)
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--skip-kernels", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU"
    res = {}
    if not a.skip_kernels:
        res["decode"] = decode_classes()
        res["append"] = append_classes()
    if not a.skip_e2e:
        res["end_to_end"] = end_to_end(a.new_tokens)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    if a.md:
        with open(a.md, "w") as f:
            f.write(markdown(res))


if __name__ == "__main__":
    main()
