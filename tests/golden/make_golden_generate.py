"""Reference fixture for Monte-Carlo generation (sampling.sample_generate): a tiny padded GQA LlamaForCausalLM converted by the
reference's to_bayesian, with the same Philox epsilon the HIP path draws (make_golden.inject).

    python tests/golden/make_golden_generate.py           # generate_gqa64.npz, a few seconds of CPU

fp32 on the CPU, greedy generation from the Bayesian-model-average probabilities of S samples: the reference has no KV cache,
so every step recomputes the whole sequence, once per sample (sample s = Monte-Carlo index s, the same weights every step).
Left-padded rows take their positions from the mask (what the framework's generate passes).  Stored per step and row: the
token, the predictive and expected entropy, the mutual information and the BMA probability of the token.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import SEED, checksum, inject, ref_to_bayesian, t2n  # noqa: E402

# hidden, heads, kv heads, layers, ffn, vocab, prompt length, batch, samples, new tokens, left padding of row 0
CONFIG = (256, 4, 2, 2, 512, 256, 24, 2, 3, 12, 5)
TEMPERATURE = 0.8


def build():
    from transformers import LlamaConfig, LlamaForCausalLM

    hidden, heads, kv_heads, layers, ffn, vocab, T0, B, S, n, pad = CONFIG
    cfg = LlamaConfig(hidden_size=hidden, num_attention_heads=heads, num_key_value_heads=kv_heads, num_hidden_layers=layers,
                      intermediate_size=ffn, vocab_size=vocab, max_position_embeddings=64, tie_word_embeddings=False,
                      use_cache=False, attention_dropout=0.0, attn_implementation="sdpa")
    torch.manual_seed(0)
    return cfg, LlamaForCausalLM(cfg).eval()


def prompt():
    hidden, heads, kv_heads, layers, ffn, vocab, T0, B, S, n, pad = CONFIG
    torch.manual_seed(321)
    ids = torch.randint(0, vocab, (B, T0))
    mask = torch.ones(B, T0, dtype=torch.long)
    mask[0, :pad] = 0
    return ids, mask


def main():
    torch.set_num_threads(8)
    hidden, heads, kv_heads, layers, ffn, vocab, T0, B, S, n, pad = CONFIG
    cfg, model = build()
    bmodel = ref_to_bayesian(model, delta=0.05, freeze=True).eval()
    csum = checksum(bmodel)
    ids, mask = prompt()
    clock = {"seed": SEED, "sample": 0}
    inject(bmodel, clock)
    tokens = np.zeros((B, n), np.int64)
    stats = np.zeros((4, B, n), np.float64)
    lp, lq = np.zeros(S), np.zeros(S)
    seq, m = ids.clone(), mask.clone()
    with torch.no_grad():
        for t in range(n):
            pos = (m.cumsum(-1) - 1).clamp(min=0)
            probs = []
            for s in range(S):
                clock["sample"] = s
                logits = bmodel(input_ids=seq, attention_mask=m, position_ids=pos, use_cache=False).logits[:, -1]
                probs.append(torch.softmax(logits.double() / TEMPERATURE, -1))
                if t == 0:
                    lp[s], lq[s] = float(bmodel.log_prior()), float(bmodel.log_variational_posterior())
            p = torch.stack(probs)  # [S, B, V]
            bma = p.mean(0)
            ent = lambda q: -(q * torch.log(q.clamp_min(1e-300))).sum(-1)  # noqa: E731
            pe, ee = ent(bma), ent(p).mean(0)
            tok = bma.argmax(-1)
            tokens[:, t] = t2n(tok)
            stats[:, :, t] = np.stack([t2n(pe), t2n(ee), t2n((pe - ee).clamp_min(0)), t2n(bma.gather(1, tok[:, None])[:, 0])])
            seq = torch.cat([seq, tok[:, None]], 1)
            m = torch.cat([m, torch.ones(B, 1, dtype=m.dtype)], 1)
    np.savez_compressed(os.path.join(HERE, "generate_gqa64.npz"), config=np.array(CONFIG, np.int64), temperature=TEMPERATURE,
                        model_seed=0, input_seed=321, delta=0.05, checksum=csum, ids=t2n(ids), mask=t2n(mask), tokens=tokens,
                        predictive_entropy=stats[0], expected_entropy=stats[1], mutual_information=stats[2],
                        token_prob=stats[3], log_prior=lp, lvp=lq)
    print("generate_gqa64:", tokens.tolist())


if __name__ == "__main__":
    main()
