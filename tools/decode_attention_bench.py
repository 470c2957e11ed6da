"""Decode attention against a KV cache: bf_attention_decode_gqa vs the framework's SDPA, and sample_generate tokens/s.

    python tools/decode_attention_bench.py [--out profiles/decode_attention_bench.json] [--new-tokens 256]

Per class (S*B sequences, H / Hkv heads, head size D, cache length Tk, new queries Tq; bf16): the call as the attention hook
makes it — the kernel through ops.attention_forward_decode, SDPA through transformers' sdpa_attention_forward with the cached
call's mask (none for Tq = 1, the [N, 1, Tq, Tk] bool mask otherwise).  Time per call = device events around 200 back-to-back
calls after 20 warm-up calls, the median of 5 such windows.  HBM fraction = (K + V bytes read) / time / 6.3 TB/s.
End to end: sample_generate on the DESIGN §4.5 decoder (8 layers, hidden 1024, 16 / 4 heads), S = 4, B = 4, prompt 512, with
and without fuse_attention.
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
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU"
    res = {"classes": kernel_vs_sdpa()}
    if not a.skip_e2e:
        res["end_to_end"] = end_to_end(a.new_tokens)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
