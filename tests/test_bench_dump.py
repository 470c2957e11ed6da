"""bench.py --dump-outputs on CPU tensors: what is written, in which dtype and shape, which elements a large array keeps
(the same ones in every run) and the 64 MB bound.  The GPU run of the flag: tests/test_gpu_models.py."""
import os

import numpy as np
import torch

import bench


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_forward_outputs_whole_and_sampled(tmp_path):
    g = torch.Generator().manual_seed(1)
    raw = (torch.randn(10, 4096, 768, generator=g).bfloat16(),)   # linear768's per-sample outputs: over DUMP_CAP
    mean = (raw[0].float().mean(0).bfloat16(),)
    lp, lq = torch.tensor(-1.5, dtype=torch.float64), torch.tensor(2.5, dtype=torch.float64)
    info = bench.dump_outputs(str(tmp_path / "a"), {"step": (raw, mean, lp, lq)}, 123.25, None)
    bench.dump_outputs(str(tmp_path / "b"), {"step": (raw, mean, lp, lq)}, 123.25, None)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert set(a) == {"samples_0", "mean_0", "log_prior", "log_variational_posterior", "elbo"}
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert info["samples_0"] == {"shape": [10, 4096, 768], "sampled": True}
    assert info["mean_0"] == {"shape": [4096, 768], "sampled": False}
    idx = bench._dump_sample(raw[0].numel())
    assert idx.shape == (bench.DUMP_CAP,) and bool((idx[1:] >= idx[:-1]).all())
    assert a["samples_0"].dtype == np.float32 and np.array_equal(a["samples_0"], raw[0].reshape(-1)[idx].float().numpy())
    assert a["mean_0"].dtype == np.float32 and np.array_equal(a["mean_0"], mean[0].float().numpy())
    for k, v in (("log_prior", -1.5), ("log_variational_posterior", 2.5), ("elbo", 123.25)):
        assert a[k].dtype == np.float64 and a[k].shape == () and float(a[k]) == v
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64 << 20


def test_serial_samples_are_stacked(tmp_path):
    logits = [torch.randn(32, 2) for _ in range(3)]
    lp = torch.tensor(0.0, dtype=torch.float64)
    info = bench.dump_outputs(str(tmp_path), {"step": ((logits,), (torch.stack(logits).mean(0),), lp, lp)}, 1.0, None)
    assert info["samples_0"] == {"shape": [3, 32, 2], "sampled": False}
    assert np.array_equal(np.load(tmp_path / "samples_0.npy"), torch.stack(logits).numpy())


def test_training_parameters_are_one_seeded_sample_of_their_concatenation(tmp_path):
    g = torch.Generator().manual_seed(2)
    params = [torch.randn(3000, 1000, generator=g).bfloat16(), torch.randn(5, generator=g), torch.randn(2000, 1000, generator=g)]
    info = bench.dump_outputs(str(tmp_path), {}, 7.0, params)
    assert set(info) == {"parameters", "elbo"} and info["parameters"] == {"shape": [5000005], "sampled": True}
    flat = torch.cat([p.float().reshape(-1) for p in params])
    assert np.array_equal(np.load(tmp_path / "parameters.npy"), flat[bench._dump_sample(flat.numel())].numpy())
    small = [torch.randn(30, 10, generator=g), torch.randn(5, generator=g)]
    assert bench.dump_outputs(str(tmp_path), {}, 7.0, small)["parameters"] == {"shape": [305], "sampled": False}
    assert np.array_equal(np.load(tmp_path / "parameters.npy"), torch.cat([p.reshape(-1) for p in small]).numpy())
