"""Decode attention against a KV cache: bf_attention_decode_gqa vs the framework's SDPA, and sample_generate tokens/s.

    python tools/decode_attention_bench.py [--out profiles/decode_attention_bench.json] [--new-tokens 256]

Per class (S*B sequences, H / Hkv heads, head size D, cache length Tk, new queries Tq; bf16): the call as the attention hook
makes it — the kernel through ops.attention_forward_decode, SDPA through transformers' sdpa_attention_forward with the cached
call's mask (none for Tq = 1, the [N, 1, Tq, Tk] bool mask otherwise).  Time per call = device events around 200 back-to-back
calls after 20 warm-up calls, the median of 5 such windows.  HBM fraction = (K + V bytes read) / time / 6.3 TB/s.
End to end: sample_generate on the DESIGN §4.5 decoder (8 layers, hidden 1024, 16 / 4 heads), S = 4, B = 4, prompt 512, with
and without fuse_attention.

    python tools/decode_attention_bench.py --kv8 [--baseline-lib OTHER/libbayeformers_amd.so] [--out K.json]

The FP8 KV cache (sample_generate(kv_cache="fp8")): per class of the same list, bf_attention_decode_gqa_kv8 on e4m3 rows
(ops.attention_forward_decode_kv8) beside the bf16 kernel on the same values, timed the same way and alternated.  With
--baseline-lib the bf16 column is bf_attention_decode_gqa of that build of the library (the parent commit's), called through
ctypes on the same tensors, and the tree's own bf16 kernel is a third column.  HBM fraction of the kv8 kernel =
(K + V bytes and scales read) / time / 6.3 TB/s.  Each time is taken twice: `_us` as above (eager calls: the short classes
are bound by the host's enqueue, where the wrappers' argument checks count) and `_graph_us` from replays of a captured graph
of 20 calls (the device's time alone: what a graph=True generation pays).
"""
import argparse
import json
import os
import statistics
import sys
import time
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM = 6.3e12


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


def _time_graph(fn, calls=20, replays=10, warm=3, reps=5):
    """Device time per call with the host taken out: `calls` back-to-back calls captured once in a graph, device events around
    `replays` replays, the median of `reps` such windows"""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(calls):
            fn()
    for _ in range(warm):
        g.replay()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(replays):
            g.replay()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / (replays * calls))
    del g
    return statistics.median(ts)


def kernel_vs_sdpa():
    from transformers.integrations.sdpa_attention import sdpa_attention_forward

    from bayeformers_amd import ops

    rows = []
    for N in (8, 32):
        for H, Hkv in ((16, 4), (32, 8), (16, 16)):
            for D in (64, 128):
                for Tk in (512, 4096, 16384):
                    for Tq in (1, 4):
                        q = torch.randn(N, Tq, H, D, device="cuda", dtype=torch.bfloat16).transpose(1, 2)
                        k = torch.randn(N, Hkv, Tk, D, device="cuda", dtype=torch.bfloat16)
                        v = torch.randn(N, Hkv, Tk, D, device="cuda", dtype=torch.bfloat16)
                        mod = types.SimpleNamespace(is_causal=True, num_key_value_groups=H // Hkv, training=False)
                        mask = None
                        if Tq > 1:
                            j = torch.arange(Tk, device="cuda")
                            mask = (j[None, :] <= torch.arange(Tk - Tq, Tk, device="cuda")[:, None])[None, None].expand(N, 1, Tq, Tk)
                        scale = D ** -0.5
                        ws = torch.empty(max(ops.attention_decode_workspace_bytes(q, k, v), 16), dtype=torch.uint8, device="cuda")
                        t_k = _time(lambda: ops.attention_forward_decode(q, k, v, None, scale, workspace=ws))
                        t_s = _time(lambda: sdpa_attention_forward(mod, q, k, v, mask, dropout=0.0, scaling=scale))
                        kv_bytes = 2 * N * Hkv * Tk * D * 2
                        rows.append({"SB": N, "H": H, "Hkv": Hkv, "D": D, "Tk": Tk, "Tq": Tq, "kernel_us": round(t_k, 2),
                                     "sdpa_us": round(t_s, 2), "speedup": round(t_s / t_k, 2),
                                     "kernel_hbm_frac": round(kv_bytes / (t_k * 1e-6) / HBM, 3)})
                        print(json.dumps(rows[-1]), flush=True)
                        del q, k, v, ws
    return rows


def _baseline_decode(path):
    """bf_attention_decode_gqa of another build of the library, as a callable (q, k, v, scale, workspace) -> out"""
    import ctypes

    from bayeformers_amd import _C, ops

    lib = ctypes.CDLL(path)
    res, args = _C.SYMBOLS["bf_attention_decode_gqa"]
    lib.bf_attention_decode_gqa.restype, lib.bf_attention_decode_gqa.argtypes = res, args

    def call(q, k, v, scale, ws):
        N, H, Tq, D = q.shape
        out = torch.empty((N, Tq, H, D), dtype=q.dtype, device=q.device)
        rc = lib.bf_attention_decode_gqa(q.data_ptr(), k.data_ptr(), v.data_ptr(), None, None, out.data_ptr(), ws.data_ptr(),
                                         _C.BF_DT_BF16, ctypes.byref(ops._decode_shape(q, k, v)), float(scale),
                                         torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
        return out

    return call


def kv8_vs_bf16(baseline_lib=None):
    from bayeformers_amd import ops

    base = _baseline_decode(baseline_lib) if baseline_lib else None
    rows = []
    for N in (8, 32):
        for H, Hkv in ((16, 4), (32, 8), (16, 16)):
            for D in (64, 128):
                for Tk in (512, 4096, 16384):
                    for Tq in (1, 4):
                        q = torch.randn(N, Tq, H, D, device="cuda", dtype=torch.bfloat16).transpose(1, 2)
                        kq, vq = (torch.empty(N, Hkv, Tk, D, dtype=torch.uint8, device="cuda") for _ in range(2))
                        ks, vs = (torch.empty(N, Hkv, Tk, dtype=torch.float32, device="cuda") for _ in range(2))
                        zero = torch.zeros(1, dtype=torch.int64, device="cuda")
                        k = torch.randn(N, Hkv, Tk, D, device="cuda", dtype=torch.bfloat16)
                        v = torch.randn(N, Hkv, Tk, D, device="cuda", dtype=torch.bfloat16)
                        ops.kv8_append(k, v, kq, vq, ks, vs, zero)
                        k, v = ops.kv8_dequantize(kq, ks, out=k), ops.kv8_dequantize(vq, vs, out=v)  # the same values
                        scale = D ** -0.5
                        ws = torch.empty(max(ops.attention_decode_workspace_bytes(q, k, v), 16), dtype=torch.uint8, device="cuda")
                        fns = {"bf16": lambda: ops.attention_forward_decode(q, k, v, None, scale, workspace=ws),
                               "kv8": lambda: ops.attention_forward_decode_kv8(q, kq, vq, ks, vs, None, None, scale, workspace=ws)}
                        if base is not None:
                            fns["baseline"] = lambda: base(q, k, v, scale, ws)
                        same = all(bool(torch.equal(fns["bf16"](), fn())) for fn in fns.values())
                        ts, tg = {name: [] for name in fns}, {name: [] for name in fns}
                        for _ in range(3):  # alternated
                            for name, fn in fns.items():
                                ts[name].append(_time(fn, reps=3))
                                tg[name].append(_time_graph(fn, reps=3))
                        t = {name: statistics.median(v_) for name, v_ in ts.items()}
                        g = {name: statistics.median(v_) for name, v_ in tg.items()}
                        ref, ref_g = t.get("baseline", t["bf16"]), g.get("baseline", g["bf16"])
                        kv_bytes = 2 * N * Hkv * Tk * (D + 4)
                        row = {"SB": N, "H": H, "Hkv": Hkv, "D": D, "Tk": Tk, "Tq": Tq, "same_bits": same,
                               "bf16_us": round(t["bf16"], 2), "kv8_us": round(t["kv8"], 2),
                               "kv8_over_bf16": round(t["kv8"] / ref, 3),
                               "bf16_graph_us": round(g["bf16"], 2), "kv8_graph_us": round(g["kv8"], 2),
                               "kv8_over_bf16_graph": round(g["kv8"] / ref_g, 3),
                               "bf16_hbm_frac": round(2 * N * Hkv * Tk * D * 2 / (ref_g * 1e-6) / HBM, 3),
                               "kv8_hbm_frac": round(kv_bytes / (g["kv8"] * 1e-6) / HBM, 3)}
                        if base is not None:
                            row["baseline_bf16_us"] = round(t["baseline"], 2)
                            row["baseline_bf16_graph_us"] = round(g["baseline"], 2)
                        rows.append(row)
                        print(json.dumps(row), flush=True)
                        del q, k, v, kq, vq, ks, vs, ws
    return rows


def end_to_end(new_tokens):
    from transformers import LlamaConfig, LlamaForCausalLM

    import bayeformers_amd as bf
    from bayeformers_amd.sampling import sample_generate

    out = {}
    for fused in (False, True):
        cfg = LlamaConfig(hidden_size=1024, num_attention_heads=16, num_key_value_heads=4, num_hidden_layers=8,
                          intermediate_size=2816, vocab_size=32000, max_position_embeddings=1024, tie_word_embeddings=False,
                          attention_dropout=0.0, attn_implementation="sdpa")
        torch.manual_seed(0)
        bmodel = bf.to_bayesian(LlamaForCausalLM(cfg).eval(), delta=0.05, freeze=True).eval().cuda()
        freqs = {n: b.detach().clone() for n, b in bmodel.named_buffers() if "inv_freq" in n}
        bmodel = bmodel.to(torch.bfloat16)
        for n, b in freqs.items():
            setattr(bmodel.get_submodule(n.rsplit(".", 1)[0]), n.rsplit(".", 1)[1], b)
        if fused:
            assert bf.fuse_attention(bmodel)
        bf.set_compute_dtype("bf16")
        ids = torch.randint(0, 32000, (4, 512), device="cuda")
        with torch.no_grad():
            sample_generate(bmodel, ids, samples=4, max_new_tokens=8)  # warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sample_generate(bmodel, ids, samples=4, max_new_tokens=new_tokens)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        out["fuse_attention" if fused else "sdpa"] = {"seconds": round(dt, 3), "tokens_per_s": round(4 * new_tokens / dt, 1)}
        print(json.dumps(out), flush=True)
        del bmodel
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--new-tokens", type=int, default=256)
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--kv8", action="store_true")
    ap.add_argument("--baseline-lib", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU"
    res = {"kv8_classes": kv8_vs_bf16(a.baseline_lib)} if a.kv8 else {"classes": kernel_vs_sdpa()}
    if not a.skip_e2e and not a.kv8:
        res["end_to_end"] = end_to_end(a.new_tokens)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
