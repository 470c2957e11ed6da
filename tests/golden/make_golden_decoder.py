"""Reference fixtures for decoder-only models (HF LlamaForCausalLM converted by the reference's to_bayesian), with the
same Philox epsilon the HIP path draws (make_golden.inject).

    python tests/golden/make_golden_decoder.py            # all four fixtures, a few seconds of CPU each

Every model is built from a LlamaConfig under torch.manual_seed(0): nothing is downloaded.  Stored per fixture: the
per-sample log_prior / log_variational_posterior, the per-sample LM logits and last-layer hidden states at 16 (sequence,
token) positions of visible tokens, and the per-sample token NLL over the visible next-token pairs.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import SEED, checksum, inject, ref_to_bayesian, t2n  # noqa: E402

N_BATCHES = 2105  # the loss's KL weight 1 / n_batches, as in make_golden.bert_train_case

# name: (hidden, heads, kv heads, layers, ffn, vocab, T, B, S, padded)
CASES = {
    "decoder_mha64": (256, 4, 4, 1, 768, 1024, 128, 2, 2, False),
    "decoder_gqa64": (512, 8, 2, 2, 1536, 1024, 256, 4, 3, True),
    "decoder_mqa128": (512, 4, 1, 2, 1536, 1024, 384, 2, 2, True),
}
TRAIN = (256, 4, 2, 2, 768, 1024, 256, 2, 2, True)


def config(hidden, heads, kv_heads, layers, ffn, vocab, T):
    from transformers import LlamaConfig

    return LlamaConfig(hidden_size=hidden, num_attention_heads=heads, num_key_value_heads=kv_heads, num_hidden_layers=layers,
                       intermediate_size=ffn, vocab_size=vocab, max_position_embeddings=T, tie_word_embeddings=False,
                       use_cache=False, attention_dropout=0.0, attn_implementation="sdpa")


def attention_mask(B, T, padded):
    """[B, T] long: without padding all ones; with padding row 0 left-padded, row 1 right-padded, the others full (the
    left padding is longer than one 128-token tile's worth of the first rows: those query rows see no key)."""
    m = torch.ones(B, T, dtype=torch.long)
    if padded:
        m[0, : T // 3 + 5] = 0
        m[1, T - T // 4 - 3:] = 0
    return m


def positions(mask, n=16, seed=7):
    """n (sequence, token) positions of visible tokens, spread over the batch (fixed seed)."""
    g = torch.Generator().manual_seed(seed)
    vis = mask.nonzero()
    idx = torch.randperm(vis.shape[0], generator=g)[:n].sort().values
    return vis[idx]


def token_nll(logits, ids, mask):
    """mean next-token cross entropy over the pairs (t, t + 1) whose tokens are both visible; logits [B, T, V]."""
    valid = (mask[:, :-1] * mask[:, 1:]).bool()
    labels = ids[:, 1:].masked_fill(~valid, -100)
    return torch.nn.functional.cross_entropy(logits[:, :-1].reshape(-1, logits.shape[-1]).double(), labels.reshape(-1),
                                             ignore_index=-100)


def build(hidden, heads, kv_heads, layers, ffn, vocab, T):
    from transformers import LlamaForCausalLM

    cfg = config(hidden, heads, kv_heads, layers, ffn, vocab, T)
    torch.manual_seed(0)
    model = LlamaForCausalLM(cfg).eval()
    return cfg, model


def inputs(cfg, B, T, padded):
    torch.manual_seed(321)
    ids = torch.randint(0, cfg.vocab_size, (B, T))
    return ids, attention_mask(B, T, padded)


def inference_case(hidden, heads, kv_heads, layers, ffn, vocab, T, B, S, padded):
    cfg, model = build(hidden, heads, kv_heads, layers, ffn, vocab, T)
    bmodel = ref_to_bayesian(model, delta=0.05, freeze=True).eval()
    csum = checksum(bmodel)
    ids, mask = inputs(cfg, B, T, padded)
    pos = positions(mask)
    clock = {"seed": SEED, "sample": 0}
    layers_ = inject(bmodel, clock)
    lp, lq, nll = np.zeros(S), np.zeros(S), np.zeros(S)
    logits_at = np.zeros((S, len(pos), vocab), np.float32)
    hidden_at = np.zeros((S, len(pos), hidden), np.float32)
    with torch.no_grad():
        for s in range(S):
            clock["sample"] = s
            out = bmodel(input_ids=ids, attention_mask=mask, output_hidden_states=True, use_cache=False)
            logits, last = out.logits, out.hidden_states[-1]
            for i, (b, t) in enumerate(pos.tolist()):
                logits_at[s, i] = t2n(logits[b, t])
                hidden_at[s, i] = t2n(last[b, t])
            nll[s] = float(token_nll(logits, ids, mask))
            lp[s] = float(bmodel.log_prior())
            lq[s] = float(bmodel.log_variational_posterior())
    return {"config": np.array([hidden, heads, kv_heads, layers, ffn, vocab, T, B, S, int(padded)], np.int64),
            "model_seed": 0, "input_seed": 321, "delta": 0.05, "n_layers": len(layers_), "checksum": csum,
            "ids_sum": int(ids.sum()), "mask": t2n(mask), "positions": t2n(pos), "logits": logits_at, "hidden": hidden_at,
            "token_nll": nll, "log_prior": lp, "lvp": lq}


def train_case():
    """One training step as make_golden.bert_train_case: the sample loop with gradients, loss = (lvp - log_prior) / NB +
    token NLL of the mean logits, loss.backward().  Stored: (sum, sum |g|, max |g|) of every trainable tensor and, in full,
    the rho gradients of layer 0's k_proj and o_proj."""
    hidden, heads, kv_heads, layers, ffn, vocab, T, B, S, padded = TRAIN
    cfg, model = build(hidden, heads, kv_heads, layers, ffn, vocab, T)
    bmodel = ref_to_bayesian(model, delta=0.05, freeze=True).eval()
    csum = checksum(bmodel)
    ids, mask = inputs(cfg, B, T, False)
    if padded:
        mask[1, T - T // 4 - 3:] = 0  # one right-padded row
    clock = {"seed": SEED, "sample": 0}
    inject(bmodel, clock)
    logits = torch.zeros(S, B, T, vocab)
    lp, lq = torch.zeros(S, B), torch.zeros(S, B)
    for s in range(S):
        clock["sample"] = s
        logits[s] = bmodel(input_ids=ids, attention_mask=mask, use_cache=False).logits
        lp[s] = bmodel.log_prior()
        lq[s] = bmodel.log_variational_posterior()
    nll = token_nll(logits.mean(0), ids, mask)
    loss = (lq.mean() - lp.mean()) / N_BATCHES + nll
    loss.backward()
    out = {"config": np.array(list(TRAIN[:-1]) + [int(padded)], np.int64), "n_batches": N_BATCHES, "model_seed": 0,
           "input_seed": 321, "delta": 0.05, "checksum": csum, "ids_sum": int(ids.sum()), "mask": t2n(mask),
           "nll": float(nll.detach()), "loss": float(loss.detach()), "log_prior": t2n(lp[:, 0]), "lvp": t2n(lq[:, 0])}
    full = ("model.layers.0.self_attn.k_proj", "model.layers.0.self_attn.o_proj")
    names = []
    for name, p_ in bmodel.named_parameters():
        if p_.grad is None:
            continue
        g = p_.grad.detach().double()
        names.append(name)
        out[f"stat/{name}"] = np.array([float(g.sum()), float(g.abs().sum()), float(g.abs().max())], np.float64)
        if name.endswith(".rho") and "prior" not in name and any(name.startswith(f + ".") or f".{f}." in name for f in full):
            out[f"grad/{name}"] = t2n(p_.grad)
    out["names"] = np.array(names)
    print(f"  decoder train: {len(names)} tensors with a gradient, {sum(k.startswith('grad/') for k in out)} stored in full")
    return out


def main():
    torch.set_num_threads(8)
    for name, spec in CASES.items():
        print(name, flush=True)
        np.savez_compressed(os.path.join(HERE, f"{name}.npz"), **inference_case(*spec))
    print("decoder_train", flush=True)
    np.savez_compressed(os.path.join(HERE, "decoder_train.npz"), **train_case())


if __name__ == "__main__":
    main()
