"""Measure the Bayesian LoRA kernels (bf_lora_fwd / bf_lora_bwd) on one MI355X and write profiles/bayesian_lora.{json,md}.

    python tools/lora_bench.py [--out profiles] [--iters 30] [--quick]

Per shape (N, K, r, rows = S * M, S = 4, bf16), each timed with device events after a warm-up, the alternatives interleaved in
one loop so that they see the same clocks:
  base       the base projection the adapter rides on (ops.lora_base_forward: one GEMM over all samples' rows)
  fwd        bf_lora_fwd alone: h = x A_s^T, y += scale * h B^T in place
  fwd_ref    the framework composite of the same two steps on the same A_s (torch.bmm + torch.baddbmm)
  bwd        bf_lora_bwd alone (g, dx += scale * g A_s in place, dA, dB)
  bwd_ref    the framework composite of the same four products
`y_pass` is the achieved bytes/s of fwd counted as ONE read and one write of y (2 * rows * N * 2 bytes): the traffic a form
fused into the base GEMM's epilogue would remove; the HBM roof it is compared with is 8 TB/s (MI355X data sheet).
A measurement path that finds no GPU fails: nothing here falls back.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bayeformers_amd import ops  # noqa: E402

HBM_ROOF = 8.0e12


def _time(fns, iters):
    """Mean milliseconds of each callable, interleaved, after 3 warm-up rounds."""
    for _ in range(3):
        for f in fns:
            f()
    torch.cuda.synchronize()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)] for _ in fns]
    for i in range(iters):
        for j, f in enumerate(fns):
            ev[j][i][0].record()
            f()
            ev[j][i][1].record()
    torch.cuda.synchronize()
    return [sorted(a.elapsed_time(b) for a, b in e)[len(e) // 2] for e in ev]  # medians


def bench_shape(N, K, r, rows, S, iters, dt=torch.bfloat16):
    M = rows // S
    g = torch.Generator().manual_seed(0)
    x = torch.randn(rows, K, generator=g).to(dt).cuda()
    a_s = (0.1 * torch.randn(S, r, K, generator=g)).to(dt).cuda()
    b = (0.1 * torch.randn(N, r, generator=g)).cuda()
    w0 = (0.02 * torch.randn(N, K, generator=g)).to(dt).cuda()
    dy = torch.randn(rows, N, generator=g).to(dt).cuda()
    y = torch.zeros(rows, N, dtype=dt, device="cuda")
    dx = torch.zeros(rows, K, dtype=dt, device="cuda")
    b16 = b.to(dt)
    scale = 2.0
    h = ops.lora_fwd(x, a_s, b, None, scale, S)

    def fwd_ref():
        hh = torch.bmm(x.view(S, M, K), a_s.transpose(1, 2))
        return torch.baddbmm(y.view(S, M, N), hh, b16.t().expand(S, r, N), alpha=scale)

    def bwd_ref():
        gg = torch.matmul(dy.view(S, M, N), b16)
        torch.baddbmm(dx.view(S, M, K), gg, a_s, alpha=scale)
        torch.bmm(gg.transpose(1, 2), x.view(S, M, K))
        return torch.matmul(dy.t(), h)

    t = _time([lambda: ops.lora_base_forward(x, w0, None), lambda: ops.lora_fwd(x, a_s, b, y, scale, S), fwd_ref,
               lambda: ops.lora_bwd(x, dy, a_s, b, h, dx, scale, S), bwd_ref], iters)
    y_bytes = 2.0 * rows * N * 2
    return {"N": N, "K": K, "r": r, "rows": rows, "S": S, "base_ms": t[0], "fwd_ms": t[1], "fwd_ref_ms": t[2], "bwd_ms": t[3],
            "bwd_ref_ms": t[4], "y_pass_TBps": y_bytes / (t[1] * 1e-3) / 1e12, "y_pass_of_roof": y_bytes / (t[1] * 1e-3) / HBM_ROOF}


def _decoder(lora: bool):
    """The DESIGN 4.5 decoder (tools/generate_bench.py's): full Bayesian (to_bayesian, MOPED, frozen means for generation) or
    Bayesian LoRA r = 16 on the seven projections of every layer; bf16, fused attention and decoder blocks (with backward)."""
    from transformers import LlamaConfig, LlamaForCausalLM

    import bayeformers_amd as bf

    cfg = LlamaConfig(hidden_size=1024, num_attention_heads=16, num_key_value_heads=4, num_hidden_layers=8,
                      intermediate_size=2816, vocab_size=32000, max_position_embeddings=1024, tie_word_embeddings=False,
                      attention_dropout=0.0, attn_implementation="sdpa")
    torch.manual_seed(0)
    src = LlamaForCausalLM(cfg).eval()
    bmodel = bf.to_bayesian_lora(src, r=16, alpha=32) if lora else bf.to_bayesian(src, delta=0.05)
    bmodel = bmodel.eval().cuda()
    freqs = {n: b.detach().clone() for n, b in bmodel.named_buffers() if "inv_freq" in n}
    bmodel = bmodel.to(torch.bfloat16)
    for n, b in freqs.items():
        setattr(bmodel.get_submodule(n.rsplit(".", 1)[0]), n.rsplit(".", 1)[1], b)
    assert bf.fuse_attention(bmodel) and bf.fuse_decoder_blocks(bmodel, backward=True) == 8
    bf.set_compute_dtype("bf16")
    return bmodel


def bench_model(which, new_tokens=64, S=4, B=2, T=512):
    """graph=True generation (tokens/s, bytes) and one training step (ms, peak bytes) of a conversion.  One conversion per
    process: the per-stream workspace of an earlier model's backward would stay in the later one's peak bytes."""
    import time

    import bayeformers_amd as bf
    from bayeformers_amd import training
    from bayeformers_amd.sampling import sample_generate

    ids = torch.randint(0, 32000, (B, T), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    out = {}
    for name, lora in which:
        bmodel = _decoder(lora)
        rec = {"kept_weight_bytes": bf.kept_weight_bytes(bmodel, S, torch.bfloat16),
               "trainable_parameters": sum(p.numel() for p in bmodel.parameters() if p.requires_grad)}
        torch.cuda.reset_peak_memory_stats()
        times = []
        with torch.no_grad():
            for i in range(4):  # the first call warms up (schedules, workspaces, the capture's eager steps)
                bf.manual_seed(1)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                sample_generate(bmodel, ids, samples=S, max_new_tokens=new_tokens, keep_weights=True, graph=True)
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t0)
        best = sorted(times[1:])[1]
        rec.update(generate_s=best, generate_tokens_per_s=B * new_tokens / best, generate_all_s=times,
                   generate_peak_bytes=torch.cuda.max_memory_allocated())
        bmodel.train()
        params = [p for p in bmodel.parameters() if p.requires_grad]
        opt = torch.optim.AdamW(params, lr=1e-4)

        def nll(mean):
            logits = mean[0][:, :-1].float()
            return torch.nn.functional.cross_entropy(logits.reshape(-1, logits.shape[-1]), ids[:, 1:].reshape(-1))

        torch.cuda.reset_peak_memory_stats()
        steps = []
        for i in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            training.training_step(bmodel, {"input_ids": ids, "use_cache": False}, S, nll, opt, n_batches=100)
            torch.cuda.synchronize()
            steps.append(time.perf_counter() - t0)
        rec.update(train_step_s=sorted(steps[1:])[1], train_all_s=steps, train_peak_bytes=torch.cuda.max_memory_allocated())
        out[name] = rec
        print(json.dumps({name: rec}), flush=True)
        del bmodel, opt, params
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--quick", action="store_true", help="one (N, K) only")
    ap.add_argument("--model", choices=("full", "lora"), help="the model-level measurement of one conversion instead of the kernels")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lora_bench: needs a GPU (nothing is measured without one)")
    if args.model:
        os.makedirs(args.out, exist_ok=True)
        which = [("full_bayesian", False)] if args.model == "full" else [("bayesian_lora_r16", True)]
        with open(os.path.join(args.out, f"bayesian_lora_model_{args.model}.json"), "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "command": " ".join(sys.argv), "model": bench_model(which)}, f,
                      indent=1)
        return
    shapes = [(4096, 4096)] if args.quick else [(4096, 4096), (11008, 4096), (4096, 11008)]
    rows_out = []
    for N, K in shapes:
        for r in (16, 64):
            for rows in (8, 64, 4096, 16384):
                rec = bench_shape(N, K, r, rows, 4, args.iters)
                rows_out.append(rec)
                print(json.dumps(rec), flush=True)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "bayesian_lora.json"), "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "dtype": "bf16", "command": " ".join(sys.argv), "kernels": rows_out},
                  f, indent=1)
    lines = ["| N | K | r | S*M | base GEMM ms | bf_lora_fwd ms | bmm+baddbmm ms | y pass TB/s (of 8) | bf_lora_bwd ms | framework bwd ms |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for q in rows_out:
        lines.append(f"| {q['N']} | {q['K']} | {q['r']} | {q['rows']} | {q['base_ms']:.4f} | {q['fwd_ms']:.4f} | {q['fwd_ref_ms']:.4f} | "
                     f"{q['y_pass_TBps']:.2f} ({100 * q['y_pass_of_roof']:.0f} %) | {q['bwd_ms']:.4f} | {q['bwd_ref_ms']:.4f} |")
    with open(os.path.join(args.out, "bayesian_lora_table.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
