"""Host-side parts of the logits processors: the numpy restatement of bf_logits_process's contract against transformers'
own processor chain (bitwise), sample_generate's refusals of repetition_penalty / no_repeat_ngram_size /
min_new_tokens, and the refusals of ops.process_logits and of the C entries without a device."""
import numpy as np
import pytest
import torch

import bayeformers_amd.nn as bnn
from bayeformers_amd import _C, ops
from bayeformers_amd.sampling import sample_generate
from logits_process_ref import process_hf, process_ref


def _case(seed, B, S, V, T0, step, dtype=torch.bfloat16, repeats=True):
    g = torch.Generator().manual_seed(seed)
    logits = (torch.randn(S * B, V, generator=g) * 4).to(dtype)
    hi = max(2, V // 8) if repeats else V  # few distinct ids: many duplicates and matching n-grams
    seq = torch.randint(0, hi, (B, T0 + step + 3), generator=g)
    return logits, seq


@pytest.mark.parametrize("seed", range(60))
def test_restatement_matches_transformers_bitwise(seed):
    rng = np.random.default_rng(seed)
    B, S = int(rng.integers(1, 4)), int(rng.integers(1, 4))
    V = int(rng.choice([5, 17, 64, 300]))
    T0, step = int(rng.integers(1, 9)), int(rng.integers(0, 9))
    logits, seq = _case(seed, B, S, V, T0, step, dtype=[torch.bfloat16, torch.float16, torch.float32][seed % 3])
    if seed % 4 == 0:
        seq[0, :2] = 0  # a left-padded prompt (pad id 0)
    theta = [None, 0.5, 1.3, 1.2, 2.0][seed % 5]
    n = seed % 5
    m = [0, step, step + 1, 2][seed % 4]
    eos = int(rng.integers(0, V))
    T = [1.0, 0.7][(seed // 2) % 2]
    ref = process_ref(logits, seq, T0, step, S, theta if theta is not None else 1.0, n, m, eos, T)
    hf = process_hf(logits, seq, T0, step, S, theta, n, m, eos, T)
    assert np.array_equal(ref.view(np.uint32), hf.view(np.uint32))


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_restatement_n_gram_edges(n):
    """L < n bans nothing, n = 1 bans every token seen, duplicates are penalised once."""
    V, T0 = 12, 3
    logits = torch.linspace(-3, 3, V).repeat(2, 1)
    seq = torch.tensor([[4, 4, 7, 4, 7, 4, 9, 9]])
    for step in range(0, 5):
        ref = process_ref(logits, seq, T0, step, 2, 1.5, n, 0, None, 0.7)
        hf = process_hf(logits, seq, T0, step, 2, 1.5, n, 0, None, 0.7)
        assert np.array_equal(ref.view(np.uint32), hf.view(np.uint32))
        L = T0 + step
        banned = np.isneginf(ref[0])
        if L < n:
            assert not banned.any()
        if n == 1:
            assert set(np.flatnonzero(banned)) == set(seq[0, :L].tolist())


def test_restatement_all_banned_row_and_min_new_tokens_sides():
    V, T0 = 3, 3
    logits = torch.tensor([[0.5, -1.0, 2.0]] * 2)
    seq = torch.tensor([[0, 1, 2, 0]])
    ref = process_ref(logits, seq, T0, 0, 2, 1.0, 1)
    assert np.isneginf(ref).all()
    assert np.array_equal(ref.view(np.uint32), process_hf(logits, seq, T0, 0, 2, None, 1).view(np.uint32))
    for step, m in ((0, 1), (1, 1), (1, 2)):
        ref = process_ref(logits, seq, T0, step, 2, 1.0, 0, m, 2)
        assert np.isneginf(ref[:, 2]).all() == (step < m)
        assert np.array_equal(ref.view(np.uint32), process_hf(logits, seq, T0, step, 2, None, 0, m, 2).view(np.uint32))


class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.lin = bnn.Linear(32, 8)

    def forward(self, x):
        return self.lin(x)


@pytest.mark.parametrize("kw", [dict(repetition_penalty=0.0), dict(repetition_penalty=-1.2),
                                dict(repetition_penalty=float("inf")), dict(repetition_penalty=float("nan")),
                                dict(repetition_penalty="1.2"), dict(repetition_penalty=True),
                                dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size=2.0),
                                dict(no_repeat_ngram_size=True), dict(no_repeat_ngram_size=65),
                                dict(min_new_tokens=-1, eos_token_id=2), dict(min_new_tokens=1.5, eos_token_id=2),
                                dict(min_new_tokens=3), dict(min_new_tokens=3, static_cache=True),
                                dict(min_new_tokens=3, graph=True)])
def test_sample_generate_refuses_processor_arguments(kw):
    args = dict(samples=2, max_new_tokens=3)
    args.update(kw)
    with torch.no_grad(), pytest.raises(ValueError):
        sample_generate(bnn.Model(_Tiny()).eval(), torch.zeros(1, 4, dtype=torch.long), **args)


def test_process_logits_refuses_a_cpu_tensor():
    with pytest.raises(_C.BayeFormersAMDError, match="ROCm device"):
        ops.process_logits(torch.rand(2, 10), torch.zeros(1, 4, dtype=torch.long), 4, 0, 2, repetition_penalty=1.2)


def _args(**kw):
    a = dict(logits=16, dtype=_C.BF_DT_BF16, R=4, V=64, row_stride=64, out=1 << 20, seq=4096, B=2, seq_stride=8, T0=4,
             d_step=None, step=0, theta=1.2, n=2, m=0, eos=-1, T=1.0)
    a.update(kw)
    return list(a.values()) + [None]


@pytest.mark.parametrize("kw,what", [(dict(dtype=7), b"dtype"), (dict(R=3), b"R="), (dict(B=0), b"R="),
                                     (dict(B=65536, R=65536), b"R="), (dict(V=0), b"V="), (dict(V=524289), b"V="),
                                     (dict(row_stride=63), b"row_stride"), (dict(step=5), b"T0="),
                                     (dict(step=-1), b"T0="), (dict(T0=-1), b"T0="), (dict(logits=None), b"NULL"),
                                     (dict(seq=None), b"NULL"), (dict(out=None), b"NULL"),
                                     (dict(theta=0.0), b"repetition_penalty"),
                                     (dict(theta=float("nan")), b"repetition_penalty"),
                                     (dict(theta=float("inf")), b"repetition_penalty"),
                                     (dict(n=-1), b"no_repeat_ngram_size"), (dict(n=65), b"no_repeat_ngram_size"),
                                     (dict(m=-1), b"min_new_tokens"), (dict(m=2), b"eos_token_id"),
                                     (dict(m=2, eos=64), b"eos_token_id"), (dict(T=0.0), b"temperature"),
                                     (dict(T=float("inf")), b"temperature"), (dict(logits=17), b"aligned"),
                                     (dict(out=1 << 20 | 2), b"aligned"), (dict(seq=4100), b"aligned"),
                                     (dict(d_step=4100), b"aligned"), (dict(out=16 + 64), b"overlaps")])
def test_c_entry_refuses(kw, what):
    lib = _C.lib()
    assert lib.bf_logits_process(*_args(**kw)) != 0 and what in lib.bf_last_error()


def test_generate_step_stat_probs_refuses_a_null_row():
    lib = _C.lib()
    args = [16, None, 16, 16, 16, 2, 64, 1, 16, 4, 16, 8, 4, 16, None, 16, 16, None, -1, 0, 0, None, None]
    assert lib.bf_generate_step_stat_probs(*args) != 0 and b"NULL" in lib.bf_last_error()
