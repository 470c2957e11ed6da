"""Host-side parts of truncated sampling: sample_generate's refusals of top_k / top_p / min_p, ops.truncate_probs and the
C entry's refusals without a device, and the numpy restatement of bf_probs_truncate's contract against transformers'
warpers (the semantics users know)."""
import numpy as np
import pytest
import torch

import bayeformers_amd.nn as bnn
from bayeformers_amd import _C, ops
from bayeformers_amd.sampling import sample_generate
from truncation_ref import softmax_rows, truncate_ref


class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.lin = bnn.Linear(32, 8)

    def forward(self, x):
        return self.lin(x)


@pytest.mark.parametrize("kw", [dict(top_k=0), dict(top_k=-3), dict(top_k=2.5), dict(top_k=True), dict(top_k="4"),
                                dict(top_p=0.0), dict(top_p=-0.1), dict(top_p=1.5), dict(top_p=float("nan")),
                                dict(min_p=-0.1), dict(min_p=1.01), dict(min_p=float("nan")),
                                dict(top_k=5, do_sample=False), dict(top_p=0.9, do_sample=False),
                                dict(min_p=0.1, do_sample=False), dict(top_p=1.0, do_sample=False),
                                dict(top_k=5, do_sample=False, static_cache=True),
                                dict(top_p=0.9, do_sample=False, graph=True)])
def test_sample_generate_refuses_truncation_arguments(kw):
    args = dict(samples=2, max_new_tokens=3, do_sample=True)
    args.update(kw)
    with torch.no_grad(), pytest.raises(ValueError):
        sample_generate(bnn.Model(_Tiny()).eval(), torch.zeros(1, 4, dtype=torch.long), **args)


def test_truncate_probs_refuses_a_cpu_tensor():
    with pytest.raises(_C.BayeFormersAMDError, match="ROCm device"):
        ops.truncate_probs(torch.rand(2, 10), top_k=3)


def _args(**kw):
    a = dict(probs=16, out=16, R=2, V=64, top_k=5, top_p=0.9, min_p=0.1)
    a.update(kw)
    return list(a.values()) + [None]


@pytest.mark.parametrize("kw,what", [(dict(R=0), b"R="), (dict(R=65536), b"R="), (dict(V=0), b"V="),
                                     (dict(V=524289), b"V="), (dict(probs=None), b"NULL"), (dict(top_p=0.0), b"top_p"),
                                     (dict(top_p=float("nan")), b"top_p"), (dict(min_p=1.5), b"min_p"),
                                     (dict(min_p=float("nan")), b"min_p"), (dict(out=16 + 4 * 64), b"overlaps"),
                                     (dict(probs=18, out=18), b"aligned")])
def test_c_entry_refuses(kw, what):
    lib = _C.lib()
    assert lib.bf_probs_truncate(*_args(**kw)) != 0 and what in lib.bf_last_error()


def _hf_kept(probs, top_k=None, top_p=None, min_p=None):
    """transformers' warpers in generate()'s order on log-probabilities: the entries left finite."""
    from transformers import MinPLogitsWarper, TopKLogitsWarper, TopPLogitsWarper

    scores = torch.from_numpy(np.log(probs.astype(np.float64))).float()
    ids = torch.zeros(scores.shape[0], 1, dtype=torch.long)
    for warper in ([TopKLogitsWarper(top_k)] if top_k else []) + ([TopPLogitsWarper(top_p)] if top_p else []) + \
            ([MinPLogitsWarper(min_p)] if min_p else []):
        scores = warper(ids, scores)
    return torch.isfinite(scores).numpy()


def _clear_of_boundaries(p, top_k, top_p, min_p, margin=1e-5):
    """No near-tie at a criterion's boundary, where float32 rounding inside the warpers could decide either way."""
    s = np.sort(p.astype(np.float64))[::-1]
    if top_k is not None and top_k < len(s) and s[top_k - 1] - s[top_k] < margin * s[top_k - 1]:
        return False
    kept = s[:top_k] if top_k else s
    if top_p is not None and np.abs(np.cumsum(kept) / kept.sum() - top_p).min() < margin:
        return False
    return min_p is None or np.abs(p - min_p * s[0]).min() >= margin * s[0]


@pytest.mark.parametrize("V", [50, 1000, 5000])
@pytest.mark.parametrize("kw", [dict(top_k=10), dict(top_p=0.9), dict(min_p=0.05), dict(top_p=0.5),
                                dict(top_k=20, top_p=0.8, min_p=0.02), dict(top_k=40, top_p=0.95)],
                         ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_restatement_agrees_with_transformers_warpers(V, kw):
    rng = np.random.default_rng(V)
    rows = []
    for _ in range(200):
        scale = (0.3, 1.0, 3.0, 8.0)[len(rows) % 4]
        p = softmax_rows(rng.standard_normal(V) * scale)
        if _clear_of_boundaries(p, kw.get("top_k"), kw.get("top_p"), kw.get("min_p")):
            rows.append(p)
    assert len(rows) >= 24
    probs = np.stack(rows[:24])
    ours = truncate_ref(probs, **kw)
    assert np.array_equal(ours > 0, _hf_kept(probs, **kw))
    kept = ours > 0
    assert np.array_equal(ours[kept].view(np.int32), probs[kept].view(np.int32)) and (ours[~kept] == 0).all()


def test_restatement_keeps_ties_and_the_argmax():
    p = np.array([[0.3, 0.2, 0.2, 0.2, 0.1]], dtype=np.float32)
    assert (truncate_ref(p, top_p=0.6) > 0).tolist() == [[True, True, True, True, False]]  # every token tied at t
    assert (truncate_ref(p, top_k=2) > 0).tolist() == [[True, True, True, True, False]]  # every token tied at p_(k)
    assert (truncate_ref(p, min_p=1.0) > 0).tolist() == [[True, False, False, False, False]]
    assert (truncate_ref(p, top_p=1e-9) > 0).tolist() == [[True, False, False, False, False]]
    special = np.array([[0.5, np.nan, 0.5], [0.0, 0.0, 0.0], [0.2, np.inf, 0.1]], dtype=np.float32)
    assert np.array_equal(truncate_ref(special, top_k=1).view(np.int32), special.view(np.int32))
