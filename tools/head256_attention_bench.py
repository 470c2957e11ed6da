"""Head size 256 (Gemma 1/2/3, Qwen3-Next): the causal grouped-query kernels and the KV-cache decode kernel against the
framework's scaled-dot-product attention, interleaved in one process.

    python tools/head256_attention_bench.py [--prefill] [--decode] [--iters N] [--rounds R] [--out R.json]

Prefill (bf16, B 4, D 256): H / Hkv 8 / 4 (Gemma 3 4B), 16 / 16 (Gemma 7B) and 8 / 1 (Gemma 2B) at T 512, 2048, 8192
(8 / 4 also at 256); forward, and forward + backward (the forward that keeps lse, then bf_attention_bwd_gqa; the framework:
the forward under autograd, then autograd.grad).  The framework's side is sdpa_attention_forward with the mask a fuse_attention
decoder hands it: None ("unmasked": no 2-D attention_mask, SDPA runs is_causal) or _padding_mask_interface's dense
[B, 1, T, T] bool mask ("masked": a batch with a right-padded row; SDPA runs attn_mask).  Gemma 3's sliding layers: W 256
.. 4096 at T 512 .. 8192 against SDPA with the sliding mask.
Decode (bf16, N 8, D 256): the same three head layouts, Tq 1 and 4, Tk 512, 4096, 32768, against sdpa_attention_forward
as a fuse_attention decoder calls it (is_causal for Tq 1, the dense bottom-right mask otherwise).
Times: device events around each call, the median of `iters` calls per round, `rounds` rounds that alternate the candidates;
reported: the median over the rounds and their spread (max - min) / median.  Every kernel result is checked against SDPA on the
same inputs before it is timed.  Flops of a causal forward: 4 D (visible pairs) per (sequence, head); forward + backward 3.5x.
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

D = 256
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


def visible_pairs(T, W=None):
    W = T if W is None else min(W, T)
    return W * (W + 1) // 2 + (T - W) * W


def rel(a, b):
    return ((a.float() - b.float()).abs().max() / b.float().abs().max()).item()


def prefill(iters, rounds):
    from transformers.integrations.sdpa_attention import sdpa_attention_forward
    from transformers.masking_utils import causal_mask_function, sliding_window_causal_mask_function

    import bayeformers_amd as bf
    from bayeformers_amd import ops

    rows = []
    B, scale = 4, D ** -0.5
    cases = [(H, Hkv, T, None, masked) for H, Hkv, Ts in ((8, 4, (256, 512, 2048, 8192)), (16, 16, (512, 2048, 8192)),
                                                          (8, 1, (512, 2048, 8192)))
             for T in Ts for masked in (False, True)]
    cases += [(8, 4, 512, 256, False), (8, 4, 2048, 512, False), (8, 4, 2048, 1024, False), (8, 4, 8192, 1024, False),
              (8, 4, 8192, 4096, False), (8, 4, 8192, 1024, True)]
    for H, Hkv, T, W, masked in cases:
        g = torch.Generator(device="cuda").manual_seed(0)
        q = torch.randn(B, T, H * D, device="cuda", generator=g, dtype=torch.bfloat16).view(B, T, H, D).transpose(1, 2)
        k, v = (torch.randn(B, T, Hkv * D, device="cuda", generator=g, dtype=torch.bfloat16).view(B, T, Hkv, D).transpose(1, 2)
                for _ in range(2))
        go = torch.randn(B, T, H, D, device="cuda", generator=g, dtype=torch.bfloat16)
        # the mask a fuse_attention decoder hands both paths: None without a 2-D attention_mask and without a window (the
        # framework's attention then runs is_causal), else _padding_mask_interface's dense [B, 1, T, T] bool mask
        pad = None
        if masked:  # a right-padded last row, as a tokenizer's batch has
            pad = torch.ones(B, T, dtype=torch.long, device="cuda")
            pad[B - 1, T - 37:] = 0
        fn = causal_mask_function if W is None else sliding_window_causal_mask_function(W)
        extra = {} if W is None else {"local_size": W}
        mask = bf._padding_mask_interface(B, q_length=T, kv_length=T, mask_function=fn, attention_mask=pad, device="cuda",
                                          **extra)
        assert (mask is None) == (not masked and W is None)
        key_mask = getattr(mask, "_bf_key_mask", None)
        mask_off = getattr(mask, "_bf_mask_off", None) if key_mask is not None else None
        mod = types.SimpleNamespace(is_causal=True, num_key_value_groups=H // Hkv, training=False)
        qs, ks, vs = (t.detach().clone().requires_grad_(True) for t in (q, k, v))

        def sdpa(a, b, c):
            return sdpa_attention_forward(mod, a, b, c, mask, dropout=0.0, scaling=scale)[0]

        def ours_fwd_bwd():
            out, lse = ops.attention_forward_gqa(q, k, v, key_mask, scale, True, mask_off, want_lse=True, window=W)
            return ops.attention_backward_gqa(q, k, v, key_mask, mask_off, out, go, lse, scale, True, window=W)

        def sdpa_fwd_bwd():
            return torch.autograd.grad(sdpa(qs, ks, vs), (qs, ks, vs), go)

        out = ops.attention_forward_gqa(q, k, v, key_mask, scale, True, mask_off, window=W)
        with torch.no_grad():
            err = rel(out, sdpa(q, k, v))
        grads, ref_grads = ours_fwd_bwd(), sdpa_fwd_bwd()
        gerr = max(rel(a, b.transpose(1, 2)) for a, b in zip(grads, ref_grads))
        del grads, ref_grads
        with torch.no_grad():
            t = rounds_of({"kernel_fwd": lambda: ops.attention_forward_gqa(q, k, v, key_mask, scale, True, mask_off, window=W),
                           "sdpa_fwd": lambda: sdpa(q, k, v)}, rounds, iters)
        t.update(rounds_of({"kernel_fwd_bwd": ours_fwd_bwd, "sdpa_fwd_bwd": sdpa_fwd_bwd}, rounds, iters))
        flops = 4 * D * visible_pairs(T, W) * B * H
        row = {"B": B, "H": H, "Hkv": Hkv, "D": D, "T": T, "W": W, "masked": masked, "max_rel_err_vs_sdpa": round(err, 5),
               "max_rel_grad_err_vs_sdpa": round(gerr, 5)}
        for key, (s, spread) in t.items():
            f = flops * (3.5 if key.endswith("bwd") else 1.0)
            row[key] = {"ms": round(s * 1e3, 4), "spread": round(spread, 3), "tflops": round(f / s / 1e12, 1),
                        "peak_frac": round(f / s / PEAK, 3)}
        row["fwd_speedup"] = round(t["sdpa_fwd"][0] / t["kernel_fwd"][0], 3)
        row["fwd_bwd_speedup"] = round(t["sdpa_fwd_bwd"][0] / t["kernel_fwd_bwd"][0], 3)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del q, k, v, go, qs, ks, vs, mask, out
        torch.cuda.empty_cache()
    return rows


def decode(iters, rounds):
    from transformers.integrations.sdpa_attention import sdpa_attention_forward

    from bayeformers_amd import ops

    rows = []
    N, scale = 8, D ** -0.5
    for H, Hkv in ((8, 4), (16, 16), (8, 1)):
        for Tk in (512, 4096, 32768):
            k = torch.randn(N, Hkv, Tk, D, device="cuda", dtype=torch.bfloat16)
            v = torch.randn(N, Hkv, Tk, D, device="cuda", dtype=torch.bfloat16)
            L = torch.tensor([Tk], device="cuda")
            for Tq in (1, 4):
                q = torch.randn(N, Tq, H, D, device="cuda", dtype=torch.bfloat16).transpose(1, 2)
                mod = types.SimpleNamespace(is_causal=True, num_key_value_groups=H // Hkv, training=False)
                mask = None
                if Tq > 1:  # the bottom-right aligned causal mask a cached chunk gets
                    i = (Tk - Tq + torch.arange(Tq, device="cuda"))[:, None]
                    mask = (torch.arange(Tk, device="cuda")[None, :] <= i)[None, None].expand(N, 1, Tq, Tk)
                ws = torch.empty(max(ops.attention_decode_workspace_bytes(q, k, v), 16), dtype=torch.uint8, device="cuda")
                with torch.no_grad():
                    ref = sdpa_attention_forward(mod, q, k, v, mask, dropout=0.0, scaling=scale)[0]
                    err = rel(ops.attention_forward_decode(q, k, v, None, scale, workspace=ws), ref)
                    t = rounds_of({
                        "kernel": lambda: ops.attention_forward_decode(q, k, v, None, scale, workspace=ws),
                        "kernel_len": lambda: ops.attention_forward_decode_len(q, k, v, L, None, scale, workspace=ws),
                        "sdpa": lambda: sdpa_attention_forward(mod, q, k, v, mask, dropout=0.0, scaling=scale),
                    }, rounds, iters)
                kv_bytes = 2 * N * Hkv * Tk * D * 2
                row = {"N": N, "H": H, "Hkv": Hkv, "D": D, "Tq": Tq, "Tk": Tk, "max_rel_err_vs_sdpa": round(err, 5)}
                for key, (s, spread) in t.items():
                    row[key] = {"us": round(s * 1e6, 2), "spread": round(spread, 3), "hbm_frac": round(kv_bytes / s / HBM, 3)}
                row["speedup"] = round(t["sdpa"][0] / t["kernel"][0], 3)
                row["speedup_len"] = round(t["sdpa"][0] / t["kernel_len"][0], 3)
                rows.append(row)
                print(json.dumps(row), flush=True)
            del k, v
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
