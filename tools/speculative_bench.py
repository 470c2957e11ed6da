"""Speculative decoding in sample_generate (speculative=γ): tokens/s against the same call without it, the acceptance
rate, and where an iteration's time goes.

    python tools/speculative_bench.py [--out profiles/speculative_decoding.json] [--md profiles/speculative_bench_tables.md]
                                      [--new-tokens 256] [--rounds 3] [--head-gain 8] [--quick]

The DESIGN §4.5 decoder (Llama, 8 layers, hidden 1024, 16 / 4 heads of 64, vocabulary 32000, MOPED δ = 0.05, random
weights), bf16, graph=True, keep_weights=True, prompt 512, S in {4, 10}, B in {1, 2}, γ in {2, 4, 7} where B·(γ+1) <= 16.
A random head gives near-uniform rows on which an argmax is a coin toss, so the head's weight is multiplied by --head-gain
(8: logits of standard deviation ~4); the acceptance rate of a trained model is its own and is NOT what this measures.  Each
configuration is also run on the same model with every ρ at −30 (the draws collapse onto the mean): every draft is accepted,
the upper end of what the loop can give.
Timing: one warm-up call, then `rounds` rounds in which the call without speculation and the calls with each γ alternate;
wall time of the whole call (prefill included) around a device synchronisation; tokens/s = B · new tokens / median, spread
= (max − min) / median over the rounds.  The time split is from a further call with sampling._SECTION_TIMES set: the
iteration is then captured as three graphs (the γ draft steps, the verify forward with its mc_predictive, the accept
launch with the two caches' rewinds) and events around their replays give the medians.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _decoder(head_gain, new_tokens, T0, collapsed=False):
    from transformers import LlamaConfig, LlamaForCausalLM

    import bayeformers_amd as bf

    cfg = LlamaConfig(hidden_size=1024, num_attention_heads=16, num_key_value_heads=4, num_hidden_layers=8,
                      intermediate_size=2816, vocab_size=32000, max_position_embeddings=T0 + new_tokens + 16,
                      tie_word_embeddings=False, attention_dropout=0.0, attn_implementation="sdpa")
    torch.manual_seed(0)
    plain = LlamaForCausalLM(cfg).eval()
    with torch.no_grad():
        plain.lm_head.weight.mul_(head_gain)
    bmodel = bf.to_bayesian(plain, delta=0.05, freeze=True).eval().cuda()
    freqs = {n: b.detach().clone() for n, b in bmodel.named_buffers() if "inv_freq" in n}
    bmodel = bmodel.to(torch.bfloat16)
    for n, b in freqs.items():
        setattr(bmodel.get_submodule(n.rsplit(".", 1)[0]), n.rsplit(".", 1)[1], b)
    if collapsed:
        with torch.no_grad():
            for layer in bmodel.fused_children():
                layer.weight.rho.fill_(-30.0)
    assert bf.fuse_attention(bmodel)
    bf.set_compute_dtype("bf16")
    return bmodel


def _timed(bmodel, ids, S, n, gamma):
    import bayeformers_amd as bf
    from bayeformers_amd.sampling import sample_generate

    bf.manual_seed(7)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad():
        gen = sample_generate(bmodel, ids, samples=S, max_new_tokens=n, graph=True, keep_weights=True, max_bytes=64 << 30,
                              speculative=gamma)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, gen


def _split(bmodel, ids, S, n, gamma):
    from bayeformers_amd import sampling

    sampling._SECTION_TIMES = marks = []
    try:
        _timed(bmodel, ids, S, n, gamma)
    finally:
        sampling._SECTION_TIMES = None
    torch.cuda.synchronize()
    cols = list(zip(*[[m[i].elapsed_time(m[i + 1]) * 1e3 for i in range(3)] for m in marks]))
    return [round(statistics.median(c), 1) for c in cols] if cols else [None] * 3


def sweep(new_tokens, rounds, head_gain, quick):
    T0 = 512
    rows = []
    for collapsed in (False, True):
        bmodel = _decoder(head_gain, new_tokens, T0, collapsed)
        for S in ((4,) if quick else (4, 10)):
            for B in ((2,) if quick else (1, 2)):
                ids = torch.randint(0, 32000, (B, T0), generator=torch.Generator().manual_seed(1)).cuda()
                gammas = [g for g in ((4,) if quick else (2, 4, 7)) if B * (g + 1) <= 16]
                for g in [None] + gammas:
                    _timed(bmodel, ids, S, 8 + (g or 0), g)  # warm-up: plans, workspaces, the mean weights
                times = {g: [] for g in [None] + gammas}
                gens = {}
                for _ in range(rounds):
                    for g in times:
                        dt, gens[g] = _timed(bmodel, ids, S, new_tokens, g)
                        times[g].append(dt)
                base = statistics.median(times[None])
                for g, ts in times.items():
                    med = statistics.median(ts)
                    row = {"posterior": "collapsed" if collapsed else "moped_0.05", "S": S, "B": B, "prompt": T0,
                           "new_tokens": new_tokens, "gamma": g or 0, "seconds": round(med, 4),
                           "spread": round((max(ts) - min(ts)) / med, 3), "tokens_per_s": round(B * new_tokens / med, 1),
                           "speedup": round(base / med, 3)}
                    if g is not None:
                        verify, proposed, accepted = gens[g].speculation.tolist()
                        same = (gens[g].sequences == gens[None].sequences).all(0)[T0:]
                        row.update(verify_steps=verify, proposed=proposed, accepted=accepted,
                                   acceptance=round(accepted / max(proposed, 1), 3),
                                   tokens_per_verify=round((new_tokens - 1) / max(verify, 1), 2),
                                   first_differing_token=int((~same).nonzero()[0]) if not bool(same.all()) else None)
                        row["draft_us"], row["verify_us"], row["accept_us"] = _split(bmodel, ids, S, new_tokens, g)
                    rows.append(row)
                    print(json.dumps(row), flush=True)
        del bmodel
        torch.cuda.empty_cache()
    return rows


def markdown(rows):
    cols = ["posterior", "S", "B", "gamma", "tokens_per_s", "spread", "speedup", "acceptance", "tokens_per_verify",
            "draft_us", "verify_us", "accept_us", "first_differing_token"]
    lines = ["| " + " | ".join(cols) + " |", "|" + "---|" * len(cols)]
    lines += ["| " + " | ".join(str(r.get(c, "")) for c in cols) + " |" for r in rows]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    ap.add_argument("--new-tokens", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--head-gain", type=float, default=8.0)
    ap.add_argument("--quick", action="store_true", help="S 4, B 2, γ 4 only")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU"
    rows = sweep(a.new_tokens, a.rounds, a.head_gain, a.quick)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)
    if a.md:
        with open(a.md, "w") as f:
            f.write(markdown(rows))


if __name__ == "__main__":
    main()
