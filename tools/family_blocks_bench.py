"""bf_norm_add_rmsnorm / bf_qknorm_rope / bf_geglu against the framework's op chains they replace, in bf16, one process:

    python tools/family_blocks_bench.py kernels [--rounds 7]      each kernel and its chain at Gemma-2-2B's shapes (hidden 2304,
                                                                  8 / 4 heads of 256, FFN 9216) and Qwen3-8B's (hidden 4096,
                                                                  32 / 8 heads of 128, FFN 12288), rows = 1, 16, 4096
    python tools/family_blocks_bench.py model [--rounds 7]        a two-layer Gemma 2 of the 2B's layer shape, one forward with
                                                                  and without fuse_decoder_blocks(families="all")

    python tools/family_blocks_bench.py backward [--rounds 7]     bf_norm_add_rmsnorm_bwd / bf_qknorm_rope_bwd / bf_geglu_bwd
                                                                  against the autograd chains they replace, at Gemma-2-2B's
                                                                  shapes (and the q / k norms at Qwen3-8B's), rows = 1, 16, 4096
    python tools/family_blocks_bench.py train [--rounds 5]        a two-layer Gemma 2 of the 2B's layer shape, one ELBO training
                                                                  step: unfused, fused (backward="all"), fused and graphed

    rocprofv3 --kernel-trace -d DIR -f csv -- python tools/family_blocks_bench.py trace
                                                                  the three kernels alone, 20 calls per (op, shape, rows) in
                                                                  the order of `kernels`: device time per dispatch from the
                                                                  trace (a run of its own; prints nothing to time)

Device events around `iters` back-to-back calls, every candidate warmed up first, the candidates interleaved inside each
round; the figures are the median (and the minimum) over the rounds.  Bytes are the algorithmic ones: what the op has to
read and write once (for the backward kernels: the figures in each kernel's comment in bf_decoder_blocks.hip).
Launches are device kernels as torch.profiler counts them in one call.  One JSON line per
measurement; profiles/family_blocks.md holds the numbers."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DT = torch.bfloat16
SHAPES = {"gemma2-2b": dict(hidden=2304, H=8, Hkv=4, D=256, ffn=9216, qk_norm=False, offset=1),
          "qwen3-8b": dict(hidden=4096, H=32, Hkv=8, D=128, ffn=12288, qk_norm=True, offset=0)}
ROWS = (1, 16, 4096)


def _launches(fn):
    from torch.profiler import ProfilerActivity, profile

    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "Memcpy" not in e.name
               and "Memset" not in e.name)


def _interleaved(cands, rounds, iters):
    """{name: fn} -> {name: [us per call, one per round]}"""
    for fn in cands.values():
        for _ in range(max(3, iters // 10)):
            fn()
    torch.cuda.synchronize()
    times = {n: [] for n in cands}
    for _ in range(rounds):
        for n, fn in cands.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            b.synchronize()
            times[n].append(a.elapsed_time(b) * 1e3 / iters)
    return times


def _report(what, shape, rows, times, nbytes, launches, rounds, iters):
    k, c = times["kernel"], times["chain"]
    mk, mc = statistics.median(k), statistics.median(c)
    print(json.dumps({"op": what, "shape": shape, "rows": rows, "kernel_us": round(mk, 2), "kernel_us_min": round(min(k), 2),
                      "chain_us": round(mc, 2), "chain_us_min": round(min(c), 2), "speedup": round(mc / mk, 2),
                      "bytes": nbytes, "kernel_GBps": round(nbytes / mk / 1e3, 1), "chain_launches": launches["chain"],
                      "kernel_launches": launches["kernel"], "rounds": rounds, "iters": iters}), flush=True)


def kernels(rounds):
    from transformers.models.gemma2.modeling_gemma2 import Gemma2RMSNorm
    from transformers.models.gemma2.modeling_gemma2 import apply_rotary_pos_emb as gemma_rope
    from transformers.models.qwen3.modeling_qwen3 import Qwen3RMSNorm
    from transformers.models.qwen3.modeling_qwen3 import apply_rotary_pos_emb as qwen_rope

    from bayeformers_amd import ops

    gen = torch.Generator().manual_seed(7)

    def randn(*shape, scale=1.0):
        return (torch.randn(*shape, generator=gen) * scale).to("cuda", DT)

    with torch.no_grad():
        for name, s in SHAPES.items():
            N, H, Hkv, D, F = s["hidden"], s["H"], s["Hkv"], s["D"], s["ffn"]
            post, pre = Gemma2RMSNorm(N).to("cuda", DT), Gemma2RMSNorm(N).to("cuda", DT)
            for m in (post, pre):
                m.weight.copy_(randn(N, scale=0.3))
            qn, kn = Qwen3RMSNorm(D).to("cuda", DT), Qwen3RMSNorm(D).to("cuda", DT)
            for rows in ROWS:
                iters = 50 if rows >= 1024 else 300
                # norm -> add -> norm (the Gemma 2 / 3 sandwich; at Qwen3's hidden size too, for the width)
                x, r = randn(rows, N), randn(rows, N, scale=3.0)
                cands = {"kernel": lambda: ops.norm_add_rmsnorm(x, post.weight, r, pre.weight, post.eps, pre.eps, 1),
                         "chain": lambda: pre(r + post(x))}
                launches = {n: _launches(f) for n, f in cands.items()}
                nbytes = rows * N * 2 * 4 + 2 * N * 2
                _report("norm_add_rmsnorm", name, rows, _interleaved(cands, rounds, iters), nbytes, launches, rounds, iters)
                # (q / k norm and) rotary embedding on the projections' [1, T, heads * D] outputs
                q = randn(1, rows, H * D).view(1, rows, H, D).transpose(1, 2)
                k = randn(1, rows, Hkv * D).view(1, rows, Hkv, D).transpose(1, 2)
                ang = torch.rand(1, rows, D // 2, generator=gen, dtype=torch.float64) * 200.0
                ang = torch.cat((ang, ang), -1)
                cos, sin = ang.cos().to("cuda", DT), ang.sin().to("cuda", DT)
                if s["qk_norm"]:
                    cands = {"kernel": lambda: ops.qknorm_rope(q, k, cos, sin, qn.weight, kn.weight, eps=qn.variance_epsilon),
                             "chain": lambda: qwen_rope(qn(q), kn(k), cos, sin)}
                else:
                    cands = {"kernel": lambda: ops.qknorm_rope(q, k, cos, sin), "chain": lambda: gemma_rope(q, k, cos, sin)}
                launches = {n: _launches(f) for n, f in cands.items()}
                nbytes = rows * (H + Hkv) * D * 2 * 2 + rows * D * 2 * 2
                _report("qknorm_rope" + ("" if s["qk_norm"] else " (no gammas)"), name, rows,
                        _interleaved(cands, rounds, iters), nbytes, launches, rounds, iters)
                # the gate
                gate, up = randn(rows, F, scale=4.0), randn(rows, F)
                cands = {"kernel": lambda: ops.geglu(gate, up),
                         "chain": lambda: torch.nn.functional.gelu(gate, approximate="tanh") * up}
                launches = {n: _launches(f) for n, f in cands.items()}
                _report("geglu", name, rows, _interleaved(cands, rounds, iters), rows * F * 2 * 3, launches, rounds, iters)


def backward(rounds):
    """Each backward kernel (its two launches where it has two) against torch.autograd.grad through the chain of
    transformers' modules it replaces; the chain's graph is built once, outside the timed region, and kept."""
    from transformers.models.gemma2.modeling_gemma2 import Gemma2RMSNorm
    from transformers.models.gemma2.modeling_gemma2 import apply_rotary_pos_emb as gemma_rope
    from transformers.models.qwen3.modeling_qwen3 import Qwen3RMSNorm
    from transformers.models.qwen3.modeling_qwen3 import apply_rotary_pos_emb as qwen_rope

    from bayeformers_amd import ops

    gen = torch.Generator().manual_seed(7)

    def randn(*shape, scale=1.0):
        return (torch.randn(*shape, generator=gen) * scale).to("cuda", DT)

    def chain_of(outs, inputs, cots):
        return lambda: torch.autograd.grad(outs, inputs, cots, retain_graph=True)

    for name, s in SHAPES.items():
        N, H, Hkv, D, F = s["hidden"], s["H"], s["Hkv"], s["D"], s["ffn"]
        post, pre = Gemma2RMSNorm(N).to("cuda", DT), Gemma2RMSNorm(N).to("cuda", DT)
        qn, kn = Qwen3RMSNorm(D).to("cuda", DT), Qwen3RMSNorm(D).to("cuda", DT)
        with torch.no_grad():
            for m in (post, pre):
                m.weight.copy_(randn(N, scale=0.3))
        for rows in ROWS:
            iters = 50 if rows >= 1024 else 300
            if name == "gemma2-2b":  # the sandwich: dy, dz_in -> dx, dz and the two dgammas
                x, r = randn(rows, N).requires_grad_(), randn(rows, N, scale=3.0).requires_grad_()
                dy, dz_in = randn(rows, N), randn(rows, N, scale=0.5)
                h = r + post(x)
                z, wp, wo, xd = h.detach(), post.weight.detach(), pre.weight.detach(), x.detach()
                cands = {"kernel": lambda: ops.norm_add_rmsnorm_backward(xd, z, wp, wo, dy, post.eps, pre.eps, 1, grad_sum=dz_in),
                         "chain": chain_of([pre(h), h], [x, r, post.weight, pre.weight], [dy, dz_in])}
                launches = {n: _launches(f) for n, f in cands.items()}
                nbytes = rows * N * 2 * 6 + 2 * N * 2 + 2 * N * 4
                _report("norm_add_rmsnorm_bwd", name, rows, _interleaved(cands, rounds, iters), nbytes, launches, rounds, iters)
            q = randn(1, rows, H * D).view(1, rows, H, D).transpose(1, 2).requires_grad_()
            k = randn(1, rows, Hkv * D).view(1, rows, Hkv, D).transpose(1, 2).requires_grad_()
            wq, wk = randn(1, H, rows, D), randn(1, Hkv, rows, D)  # where the attention backward leaves them
            ang = torch.rand(1, rows, D // 2, generator=gen, dtype=torch.float64) * 200.0
            ang = torch.cat((ang, ang), -1)
            cos, sin = ang.cos().to("cuda", DT), ang.sin().to("cuda", DT)
            qd, kd = q.detach(), k.detach()
            if s["qk_norm"]:
                gq, gk = qn.weight.detach(), kn.weight.detach()
                cands = {"kernel": lambda: ops.qknorm_rope_backward(wq, wk, cos, sin, qd, kd, gq, gk, qn.variance_epsilon, 0),
                         "chain": chain_of(list(qwen_rope(qn(q), kn(k), cos, sin)), [q, k, qn.weight, kn.weight], [wq, wk])}
            else:
                cands = {"kernel": lambda: ops.qknorm_rope_backward(wq, wk, cos, sin),
                         "chain": chain_of(list(gemma_rope(q, k, cos, sin)), [q, k], [wq, wk])}
            launches = {n: _launches(f) for n, f in cands.items()}
            nbytes = rows * (H + Hkv) * D * 2 * (3 if s["qk_norm"] else 2) + rows * D * 2 * 2
            _report("qknorm_rope_bwd" + ("" if s["qk_norm"] else " (no gammas)"), name, rows,
                    _interleaved(cands, rounds, iters), nbytes, launches, rounds, iters)
            if name == "gemma2-2b":
                gate, up, dy = randn(rows, F, scale=4.0).requires_grad_(), randn(rows, F).requires_grad_(), randn(rows, F)
                gd, ud = gate.detach(), up.detach()
                cands = {"kernel": lambda: ops.geglu_backward(gd, ud, dy),
                         "chain": chain_of(torch.nn.functional.gelu(gate, approximate="tanh") * up, [gate, up], dy)}
                launches = {n: _launches(f) for n, f in cands.items()}
                _report("geglu_bwd", name, rows, _interleaved(cands, rounds, iters), rows * F * 2 * 5, launches, rounds, iters)


def train(rounds):
    """Two layers of Gemma-2-2B's shape as in `model`, one ELBO training step (S = 2 samples of [2, 512] tokens, AdamW) with
    the attention kernels in every mode: the blocks unfused, fused with backward="all", and fused inside GraphedTrainingStep."""
    from transformers import AutoConfig, AutoModelForCausalLM

    import bayeformers_amd as bf
    from bayeformers_amd.training import GraphedTrainingStep, training_step

    bf.softcap_attention()
    s = SHAPES["gemma2-2b"]
    B, T, S = 2, 512, 2
    ids = torch.randint(0, 4096, (B, T), generator=torch.Generator().manual_seed(1)).cuda()
    inputs = {"input_ids": ids, "use_cache": False}

    def nll(mean):
        logits = mean[0].float()
        return torch.nn.functional.cross_entropy(logits[:, :-1].reshape(-1, logits.shape[-1]), ids[:, 1:].reshape(-1), reduction="sum")

    cands, closers = {}, []
    for mode in ("unfused", "fused", "fused graphed"):
        cfg = AutoConfig.for_model("gemma2", hidden_size=s["hidden"], num_attention_heads=s["H"], num_key_value_heads=s["Hkv"],
                                   head_dim=s["D"], num_hidden_layers=2, intermediate_size=s["ffn"], vocab_size=4096,
                                   max_position_embeddings=2048, tie_word_embeddings=False, attention_dropout=0.0,
                                   attn_implementation="eager", sliding_window=512,
                                   layer_types=["sliding_attention", "full_attention"])
        torch.manual_seed(0)
        bmodel = bf.to_bayesian(AutoModelForCausalLM.from_config(cfg).eval(), delta=0.05, freeze=True).eval().cuda().to(DT)
        for p in bmodel.parameters():
            p.requires_grad_(p.dtype.is_floating_point)
        assert bf.fuse_attention(bmodel)
        if mode != "unfused":
            assert bf.fuse_decoder_blocks(bmodel, backward="all", families="all") == 2
        opt = torch.optim.AdamW([p for p in bmodel.parameters() if p.requires_grad], lr=torch.tensor(1e-5, device="cuda"),
                                fused=True, capturable=True)
        if mode == "fused graphed":
            step = GraphedTrainingStep(bmodel, inputs, S, nll, opt, 4, max_grad_norm=None, eager_steps=1)
            closers.append(step)
            cands[mode] = step
        else:
            cands[mode] = lambda m=bmodel, o=opt: training_step(m, inputs, S, nll, o, 4, max_grad_norm=None)
    try:
        launches = {n: (_launches(f) if n != "fused graphed" else None) for n, f in cands.items()}
        iters = 5
        times = _interleaved(cands, rounds, iters)
        for mode in cands:
            t = times[mode]
            print(json.dumps({"model": "gemma2 2 layers", "step": "train", "tokens": [S, B, T], "mode": mode,
                              "ms": round(statistics.median(t) / 1e3, 3), "ms_min": round(min(t) / 1e3, 3),
                              "device_kernels": launches[mode], "rounds": rounds, "iters": iters}), flush=True)
    finally:
        for step in closers:
            step.close()


TRACE_CALLS = 20


def trace():
    """The kernels of `kernels` without the chains, TRACE_CALLS calls per (shape, rows, op) in that nesting: a kernel trace
    of this run holds, for each of the three kernel families, consecutive groups of TRACE_CALLS dispatches in that order."""
    from bayeformers_amd import ops

    gen = torch.Generator().manual_seed(7)

    def randn(*shape, scale=1.0):
        return (torch.randn(*shape, generator=gen) * scale).to("cuda", DT)

    for name, s in SHAPES.items():
        N, H, Hkv, D, F = s["hidden"], s["H"], s["Hkv"], s["D"], s["ffn"]
        gp, go, gq, gk = randn(N, scale=0.3), randn(N, scale=0.3), randn(D) + 1, randn(D) + 1
        for rows in ROWS:
            x, r = randn(rows, N), randn(rows, N, scale=3.0)
            q = randn(1, rows, H * D).view(1, rows, H, D).transpose(1, 2)
            k = randn(1, rows, Hkv * D).view(1, rows, Hkv, D).transpose(1, 2)
            cos, sin = randn(1, rows, D), randn(1, rows, D)
            gate, up = randn(rows, F, scale=4.0), randn(rows, F)
            for _ in range(TRACE_CALLS):
                ops.norm_add_rmsnorm(x, gp, r, go, 1e-6, 1e-6, 1)
            for _ in range(TRACE_CALLS):
                ops.qknorm_rope(q, k, cos, sin, *((gq, gk) if s["qk_norm"] else ()))
            for _ in range(TRACE_CALLS):
                ops.geglu(gate, up)
            torch.cuda.synchronize()


def model(rounds):
    """Two layers of Gemma-2-2B's shape (vocabulary cut to 4096) as a Bayesian decoder on the attention kernels, with and
    without the block rewrite: ms per forward of [1, 16] and [4, 1024] tokens, device kernels per forward."""
    from transformers import AutoConfig, AutoModelForCausalLM

    import bayeformers_amd as bf
    from bayeformers_amd.sampling import sample_bayesian

    bf.softcap_attention()
    s = SHAPES["gemma2-2b"]
    models = {}
    for mode in ("unfused", "fused"):
        cfg = AutoConfig.for_model("gemma2", hidden_size=s["hidden"], num_attention_heads=s["H"], num_key_value_heads=s["Hkv"],
                                   head_dim=s["D"], num_hidden_layers=2, intermediate_size=s["ffn"], vocab_size=4096,
                                   max_position_embeddings=2048, tie_word_embeddings=False, attention_dropout=0.0,
                                   attn_implementation="eager", sliding_window=512,
                                   layer_types=["sliding_attention", "full_attention"])
        torch.manual_seed(0)
        bmodel = bf.to_bayesian(AutoModelForCausalLM.from_config(cfg).eval(), delta=0.05, freeze=True).eval().cuda().to(DT)
        assert bf.fuse_attention(bmodel)
        if mode == "fused":
            assert bf.fuse_decoder_blocks(bmodel, families="all") == 2
        bmodel.graph_replay = False
        models[mode] = bmodel
    for B, T in ((1, 16), (4, 1024)):
        ids = torch.randint(0, 4096, (B, T), generator=torch.Generator().manual_seed(1)).cuda()

        def run(m):
            bf.manual_seed(0x5EED)
            with torch.no_grad():
                return sample_bayesian(m, {"input_ids": ids, "use_cache": False}, 1)[0][0]

        cands = {mode: (lambda m=m: run(m)) for mode, m in models.items()}
        launches = {n: _launches(f) for n, f in cands.items()}
        iters = 20 if T < 256 else 5
        times = _interleaved(cands, rounds, iters)
        for mode in cands:
            t = times[mode]
            print(json.dumps({"model": "gemma2 2 layers", "tokens": [B, T], "mode": mode,
                              "ms": round(statistics.median(t) / 1e3, 3), "ms_min": round(min(t) / 1e3, 3),
                              "device_kernels": launches[mode], "rounds": rounds, "iters": iters}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernels", "model", "backward", "train", "trace"])
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("family_blocks_bench: no ROCm device; a timing without one is not a measurement")
    if args.what == "trace":
        trace()
    else:
        {"kernels": kernels, "model": model, "backward": backward, "train": train}[args.what](args.rounds)
