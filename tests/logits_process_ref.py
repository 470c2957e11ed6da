"""A numpy restatement of bf_logits_process's contract (include/bayeformers_amd.h) and transformers' own processor chain,
which the restatement must equal bit for bit."""
import numpy as np
import torch


def process_ref(logits, sequences, T0, step, samples, repetition_penalty=1.0, no_repeat_ngram_size=0,
                min_new_tokens=0, eos_token_id=None, temperature=1.0):
    """The expected fp32 [S * B, V] output of bf_logits_process for logits [S * B, V] (any float dtype) and the
    histories sequences [B, >= T0 + step] (int)."""
    x = np.array(torch.as_tensor(logits).float().cpu().numpy(), dtype=np.float32)
    seq = np.asarray(torch.as_tensor(sequences).cpu().numpy(), dtype=np.int64)
    R, V = x.shape
    B = seq.shape[0]
    assert R == samples * B
    L = min(T0 + step, seq.shape[1])
    theta, T, n = np.float32(repetition_penalty), np.float32(temperature), int(no_repeat_ngram_size)
    for b in range(B):
        h = [int(i) for i in seq[b, :L]]
        seen = sorted({i for i in h if 0 <= i < V})
        banned = set()
        if n >= 1 and L >= n:
            prefix = h[L - n + 1:]
            for i in range(L - n + 1):
                if h[i:i + n - 1] == prefix and 0 <= h[i + n - 1] < V:
                    banned.add(h[i + n - 1])
        if step < min_new_tokens:
            banned.add(int(eos_token_id))
        for s in range(samples):
            row = x[s * B + b]
            if theta != np.float32(1.0) and seen:
                v = row[seen]
                row[seen] = np.where(v < 0, v * theta, v / theta)
            if banned:
                row[sorted(banned)] = -np.inf
            if T != np.float32(1.0):
                row /= T
    return x


def process_hf(logits, sequences, T0, step, samples, repetition_penalty=None, no_repeat_ngram_size=0,
               min_new_tokens=0, eos_token_id=None, temperature=1.0):
    """transformers' RepetitionPenalty, NoRepeatNGram and MinNewTokensLength processors, then its temperature warper, in
    generate()'s order on the fp32 upcast (on the CPU), the input_ids being the sample-major repeat of the histories."""
    from transformers import (MinNewTokensLengthLogitsProcessor, NoRepeatNGramLogitsProcessor,
                              RepetitionPenaltyLogitsProcessor, TemperatureLogitsWarper)

    scores = torch.as_tensor(logits).cpu().to(torch.float32).clone()
    seq = torch.as_tensor(sequences).cpu().to(torch.long)
    input_ids = seq[:, :T0 + step].repeat(samples, 1)
    chain = []
    if repetition_penalty is not None:
        chain.append(RepetitionPenaltyLogitsProcessor(float(repetition_penalty)))
    if no_repeat_ngram_size:
        chain.append(NoRepeatNGramLogitsProcessor(int(no_repeat_ngram_size)))
    if min_new_tokens:
        chain.append(MinNewTokensLengthLogitsProcessor(int(T0), int(min_new_tokens), int(eos_token_id)))
    if temperature != 1.0:
        chain.append(TemperatureLogitsWarper(float(temperature)))
    for proc in chain:
        scores = proc(input_ids, scores)
    return scores.numpy()
