"""Causal / grouped-query attention timings: the kernels against torch's scaled_dot_product_attention
(is_causal=True, enable_gqa=True), interleaved in one process, and a Bayesian decoder's Monte-Carlo forward with and
without fuse_attention.

    python tools/causal_attention_bench.py [--kernels] [--model] [--iters N] [--lengths T [T ...]] [--against LIB [--out J]]

Kernel shapes (S*B, H, Hkv, D, T): (a) 16, 16, 4, 64, 1024; (b) 8, 32, 8, 128, 2048; (c) the non-causal kernel at (a).
Causal forward flops = 2 * 2 * D * T * (T + 1) / 2 per (sequence, head) (QK^T and PV over the visible half), the
backward 2.5x that; the non-causal forward 4 * D * T^2.  Peak: 2.5 PFLOP/s dense bf16.  Times here are host-timed events
around each launch sequence (median); kernel-only times come from a rocprofv3 --kernel-trace --stats run of the same
script.  --lengths: shapes (a) and (b) at each of the given sequence lengths instead of their own (any T >= 1: a length
that is no multiple of 128 runs the kernels' tail forms), the same interleaved rounds; prints one line per (shape, T).
--against LIB [--out J.json]: every entry of the AGAINST table — the plain, ragged, non-causal, head-256, window, soft-cap and
band forward and backward, the chunk and the decode entries with their kv8 and kv_len forms — on this tree's library and on
another build of it (e.g. one built from another commit), both loaded into this process and timed in alternating pairs; says
per entry whether the two give the same bits (same_bits).
"""
import argparse
import ctypes
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


def kernels(iters, lengths=None):
    from bayeformers_amd import ops

    shapes = SHAPES
    if lengths:
        shapes = {f"{n}@{T}": SHAPES[n][:4] + (T, True) for n in ("a", "b") for T in lengths}
    rows = []
    for name, (B, H, Hkv, D, T, causal) in shapes.items():
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
            row[key + "_rounds_ms"] = [round(x * 1e3, 4) for x in vals]
            flops = fwd_flops * (2.5 if key.endswith("bwd") else 1.0)
            row[key] = {"ms": round(t * 1e3, 4), "tflops": round(flops / t / 1e12, 1), "peak_frac": round(flops / t / PEAK, 3)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


# --against: (entry, family, (S*B, H, Hkv, D, T), options), bf16.  gqa: forward and backward at sequence length T (window,
# softcap; docs: packed documents of that many tokens, the band entries; causal False: the non-causal kernels); chunk and
# decode: Tq new queries against T cached keys (kv8: the FP8 cache entries, which with the chunk entries take a window and
# a softcap; len: the filled keys of bf_attention_decode_gqa_len).  (a) and (b) are this tool's shapes, "ragged" is (a)
# at a T that is no multiple of 128, the others are shapes of sliding_attention_bench.py, softcap_attention_bench.py, packed_attention_bench.py, head256_attention_bench.py,
# chunked_prefill_bench.py and decode_attention_bench.py.
AGAINST = [
    ("a", "gqa", (16, 16, 4, 64, 1024), {}),
    ("b", "gqa", (8, 32, 8, 128, 2048), {}),
    ("ragged", "gqa", (16, 16, 4, 64, 1000), {}),
    ("noncausal128", "gqa", (8, 32, 8, 128, 2048), {"causal": False}),
    ("head256", "gqa", (4, 8, 4, 256, 2048), {}),
    ("window", "gqa", (8, 32, 8, 128, 8192), {"window": 1024}),
    ("softcap", "gqa", (2, 32, 16, 128, 2048), {"softcap": 50.0}),
    ("softcap_window", "gqa", (2, 8, 4, 256, 8192), {"softcap": 50.0, "window": 4096}),
    ("band", "gqa", (4, 32, 8, 128, 2048), {"docs": 512}),
    ("chunk", "chunk", (8, 16, 4, 128, 4096), {"Tq": 512}),
    ("chunk_window", "chunk", (8, 16, 4, 64, 4096), {"Tq": 512, "window": 1024}),
    ("chunk_kv8", "chunk", (8, 16, 4, 128, 4096), {"Tq": 512, "kv8": True}),
    ("chunk_kv8_256", "chunk", (8, 16, 4, 256, 4096), {"Tq": 512, "kv8": True}),
    ("decode", "decode", (8, 16, 4, 128, 4096), {"Tq": 1}),
    ("decode_len", "decode", (8, 16, 4, 64, 16384), {"Tq": 4, "len": 12001}),
    ("decode_kv8", "decode", (8, 16, 4, 128, 4096), {"Tq": 1, "kv8": True}),
    ("decode_kv8_softcap_window", "decode", (8, 16, 4, 64, 16384), {"Tq": 1, "kv8": True, "softcap": 50.0, "window": 4096}),
    ("decode256", "decode", (8, 8, 4, 256, 4096), {"Tq": 4}),
]


def _ptr(t):
    return None if t is None else t.data_ptr()


def _against_gqa(libs, dims, opt):
    from bayeformers_amd import _C, ops

    B, H, Hkv, D, T = dims
    W, cap, docs = opt.get("window"), opt.get("softcap"), opt.get("docs")
    g = torch.Generator(device="cuda").manual_seed(0)
    q = torch.randn(B, T, H * D, device="cuda", generator=g, dtype=torch.bfloat16).view(B, T, H, D).transpose(1, 2)
    k, v = (torch.randn(B, T, Hkv * D, device="cuda", generator=g, dtype=torch.bfloat16).view(B, T, Hkv, D).transpose(1, 2)
            for _ in range(2))
    go = torch.randn(B, T, H, D, device="cuda", generator=g, dtype=torch.bfloat16)
    shape, scale = ops._gqa_shape(q, k, v, opt.get("causal", True)), D ** -0.5
    new = lambda *s, dt=torch.bfloat16: torch.empty(*s, device="cuda", dtype=dt)
    res = {l: dict(out=new(B, T, H, D), lse=new(B, H, T, dt=torch.float32), delta=new(B, H, T, dt=torch.float32),
                   dq=new(B, T, H, D), dk=new(B, T, Hkv, D), dv=new(B, T, Hkv, D)) for l in libs}
    if docs:  # the band entries: (lo) / (lo, hi) in place of (mask, mask_off)
        lo, hi = ops.band_bounds((torch.arange(T, device="cuda") // docs)[None].expand(B, T))
        suffix, tail, fwd_keys, bwd_keys = "_band", (), (lo,), (lo, hi)
    else:
        suffix, tail = ("_softcap", (int(W or 0), cap)) if cap else ("_window", (W,)) if W else ("", ())
        fwd_keys = bwd_keys = (None, None)

    def fwd(l):
        r = res[l]
        assert getattr(libs[l], "bf_attention_fwd_gqa" + suffix)(
            *map(_ptr, (q, k, v, *fwd_keys, r["out"], r["lse"])), _C.BF_DT_BF16, ctypes.byref(shape), *tail, scale,
            ops._stream_ptr()) == 0

    def bwd(l):
        r = res[l]
        assert getattr(libs[l], "bf_attention_bwd_gqa" + suffix)(
            *map(_ptr, (q, k, v, *bwd_keys, r["out"], go, r["lse"], r["delta"], r["dq"], r["dk"], r["dv"])), _C.BF_DT_BF16,
            ctypes.byref(shape), *tail, scale, ops._stream_ptr()) == 0

    return {"fwd": fwd, "bwd": bwd}, res


def _against_cache(libs, dims, opt, chunk):
    """the chunk (chunk=True) and the decode entries: Tq new queries against a cache of T keys"""
    from bayeformers_amd import _C, ops

    N, H, Hkv, D, L = dims
    Tq, W, kv8, fill = opt["Tq"], opt.get("window"), opt.get("kv8", False), opt.get("len")
    cap = opt.get("softcap", 0.0)  # the chunk and the kv8 entries take (window, softcap): 0 = none
    g = torch.Generator(device="cuda").manual_seed(D + L)
    k, v = (torch.randn(N, Hkv, L, D, device="cuda", generator=g, dtype=torch.bfloat16) for _ in range(2))
    q = torch.randn(N, Tq, H, D, device="cuda", generator=g, dtype=torch.bfloat16).transpose(1, 2)
    scale, kv_len = D ** -0.5, None
    if chunk or fill:
        kv_len = torch.tensor([fill or L], device="cuda")
    scales = ()
    if kv8:
        kq, vq = (torch.zeros(N, Hkv, L, D, dtype=torch.uint8, device="cuda") for _ in range(2))
        scales = tuple(torch.zeros(N, Hkv, L, device="cuda") for _ in range(2))
        ops.kv8_append(k, v, kq, vq, *scales, torch.zeros(1, dtype=torch.long, device="cuda"))
        k, v = kq, vq
    shape = ops._decode_shape(q, k, v)
    res = {l: {"out": torch.empty(N, Tq, H, D, device="cuda", dtype=torch.bfloat16)} for l in libs}
    if chunk:
        entry = "bf_attention_chunk_gqa" + ("_kv8" if kv8 else "")
        tail = (int(W or 0), 0, cap)  # window, key_origin, softcap
        ws = {l: () for l in libs}
    else:
        entry = "bf_attention_decode_gqa" + ("_kv8" if kv8 else "_len" if fill else "")
        tail = (int(W or 0), cap) if kv8 else ()
        nbytes = max(int(libs["this"].bf_attention_decode_workspace_bytes(ctypes.byref(shape))), 16)
        ws = {l: (torch.empty(nbytes, dtype=torch.uint8, device="cuda"),) for l in libs}
    lens = (kv_len,) if chunk or kv8 or fill else ()  # the entries with a kv_len argument (nullable in the kv8 one)

    def run(l):
        assert getattr(libs[l], entry)(*map(_ptr, (q, k, v, *scales, None, None, *lens, res[l]["out"], *ws[l])),
                                       _C.BF_DT_BF16, ctypes.byref(shape), *tail, scale, ops._stream_ptr()) == 0

    return {"fwd": run}, res


def against(path, iters, out=None, pairs=15):
    """every AGAINST entry on this tree's library and on the one at `path`, in alternating pairs"""
    from bayeformers_amd import _C

    def load(p):
        l = ctypes.CDLL(p)
        for table in (_C.SYMBOLS, _C.SOFTCAP_SYMBOLS, _C.PACKED_SYMBOLS, _C.KV8_SYMBOLS, _C.CHUNK_SYMBOLS):
            for name, (restype, argtypes) in table.items():
                if name.startswith("bf_attention_") or name == "bf_version":
                    fn = getattr(l, name)
                    fn.restype, fn.argtypes = restype, argtypes
        assert l.bf_version() == _C.ABI_VERSION, p
        return l

    libs = {"this": load(_C.LIB_PATH), "other": load(path)}
    rows = []
    for name, family, dims, opt in AGAINST:
        calls, res = _against_gqa(libs, dims, opt) if family == "gqa" else _against_cache(libs, dims, opt, family == "chunk")
        for l in libs:
            for _ in range(3):
                for fn in calls.values():
                    fn(l)
        torch.cuda.synchronize()
        row = {"entry": name, "family": family, **dict(zip(("SB", "H", "Hkv", "D", "T"), dims)), **opt,
               "same_bits": all(torch.equal(res["this"][n], res["other"][n]) for n in res["this"])}
        for what, fn in calls.items():
            t = {"this": [], "other": []}
            for i in range(pairs):
                for l in (("this", "other") if i % 2 == 0 else ("other", "this")):
                    t[l].append(timed(lambda: fn(l), iters) * 1e3)
            ratios = [a / b for a, b in zip(t["this"], t["other"])]
            row[what] = {l + "_ms": {"median": round(statistics.median(x), 4), "min": round(min(x), 4), "max": round(max(x), 4)}
                         for l, x in t.items()}
            row[what]["pair_ratio_this_over_other"] = {"median": round(statistics.median(ratios), 4),
                                                       "min": round(min(ratios), 4), "max": round(max(ratios), 4)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if out:
        with open(out, "w") as f:
            json.dump({"this": _C.LIB_PATH, "other": path, "iters": iters, "pairs": pairs, "entries": rows}, f, indent=1)


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
    ap.add_argument("--lengths", type=int, nargs="+", default=None, help="time shapes (a) and (b) at these sequence lengths")
    ap.add_argument("--against", default=None, help="another build of the library: alternating pairs over the AGAINST table")
    ap.add_argument("--out", default=None, help="with --against: write the rows to this JSON file")
    a = ap.parse_args()
    if a.against:
        against(a.against, a.iters, a.out)
        return
    if a.lengths:
        a.kernels = True
    if not (a.kernels or a.model):
        a.kernels = a.model = True
    if a.kernels:
        kernels(a.iters, a.lengths)
    if a.model:
        model(max(3, a.iters // 4))


if __name__ == "__main__":
    main()
