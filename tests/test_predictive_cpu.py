"""Host side of the Monte-Carlo predictive statistics (no kernel is launched here): the public names, the packed-partial
layout of bf_mc_predictive_bytes, and the argument checks that come before any device work."""
import pytest
import torch

from bayeformers_amd import _C, ops
from bayeformers_amd.sampling import GraphedSampler, Predictive, mc_predictive, sample_predictive


def test_public_names():
    assert callable(mc_predictive) and callable(sample_predictive)
    names = {f for f in Predictive.__dataclass_fields__}
    assert {"mean", "probs", "predictive_entropy", "expected_entropy", "mutual_information", "prediction",
            "correct_per_sample", "acc_std", "bma_correct", "log_likelihood", "nll", "invalid_labels", "log_prior",
            "log_variational_posterior"} <= names
    import inspect

    sig = inspect.signature(GraphedSampler.__init__).parameters
    assert sig["predictive"].default is False and sig["labels"].default is None
    assert list(inspect.signature(GraphedSampler.__call__).parameters) == ["self", "inputs", "labels"]


def test_cpu_input_raises():
    with pytest.raises(_C.BayeFormersAMDError, match="ROCm device"):
        mc_predictive(torch.randn(4, 3, 5))
    with pytest.raises(_C.BayeFormersAMDError, match="ROCm device"):
        mc_predictive(torch.randn(4, 3, 5), torch.tensor([0, 1, 2]))


def _documented(R, C, S, labels):
    """include/bayeformers_amd.h: fp32 sum_p [R][C] | fp32 sum_h [R] | pad to 8 | fp64 sum_py [R] | fp64 sum_logpy [R] |
    fp64 counts [S] (the last three with labels only)."""
    sum_h = 4 * R * C
    sum_py = (sum_h + 4 * R + 7) // 8 * 8
    nl = R if labels else 0
    sum_logpy = sum_py + 8 * nl
    counts = sum_logpy + 8 * nl
    end = counts + (8 * S if labels else 0)
    return end, (0, sum_h, sum_py, sum_logpy, counts, end)


@pytest.mark.parametrize("R,C,S,labels", [(32, 2, 10, True), (32, 2, 10, False), (1, 1, 1, True), (3, 1, 1, False),
                                          (4096, 30522, 10, True), (7, 1001, 64, True), (5, 3, 5, False)])
def test_packed_partial_layout(R, C, S, labels):
    assert ops.predictive_layout(R, C, S, labels) == _documented(R, C, S, labels)


def test_layout_rejects_empty_shapes():
    assert _C.lib().bf_mc_predictive_bytes(0, 3, 2, 1, None) == 0
    assert _C.lib().bf_mc_predictive_bytes(3, 0, 2, 1, None) == 0
    assert _C.lib().bf_mc_predictive_bytes(3, 3, 0, 1, None) == 0
    assert _C.lib().bf_mc_predictive_workspace_bytes(0) == 0
    assert _C.lib().bf_mc_predictive_workspace_bytes(10) >= 64


def test_label_shape_validation():
    raw = torch.randn(4, 3, 5)
    with pytest.raises(ValueError, match="row shape"):
        mc_predictive(raw, torch.tensor([0, 1]))
    with pytest.raises(ValueError, match="row shape"):
        mc_predictive(torch.randn(4, 2, 6, 5), torch.zeros(2, dtype=torch.long))  # token classification wants [2, 6]
    with pytest.raises(TypeError, match="integer"):
        mc_predictive(raw, torch.zeros(3))
    with pytest.raises(TypeError, match="fp32, bf16 or fp16"):
        mc_predictive(torch.zeros(4, 3, 5, dtype=torch.int32))
    with pytest.raises(ValueError):
        mc_predictive(torch.randn(5))


def test_labels_per_output():
    from bayeformers_amd.sampling import _labels_per_output

    a, b = torch.zeros(2, dtype=torch.long), torch.ones(2, dtype=torch.long)
    assert _labels_per_output(None, 2) == (None, None)
    assert _labels_per_output((a, b), 2) == (a, b)
    with pytest.raises(ValueError, match="start_positions"):
        _labels_per_output(a, 2)
