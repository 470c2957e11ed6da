"""Local reparameterisation without a GPU: the float64 reference of tests/lrt_ref.py against torch.autograd, the variance of
the estimator itself against the weight-space one, the closed-form KL terms against sampled log-probs, the switch
(local_reparameterization) and the C-ABI table (include/bayeformers_amd_lrt.h)."""
import ctypes
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lrt_ref  # noqa: E402

import bayeformers_amd as bf  # noqa: E402
import bayeformers_amd.nn as bnn  # noqa: E402
from bayeformers_amd import _C, ops  # noqa: E402
from oracle import bayes_oracle as bo  # noqa: E402

SEED = 0x5EED


@pytest.mark.parametrize("act", [False, True])
def test_reference_gradients_match_autograd(act):
    S, M, N, K, layer_id = 3, 5, 24, 16, 7
    g = torch.Generator().manual_seed(4)
    x = torch.randn(S * M, K, generator=g, dtype=torch.float64, requires_grad=True)
    mu = (0.3 * torch.randn(N, K, generator=g)).double().requires_grad_()
    rho = (-2.0 + 0.5 * torch.randn(N, K, generator=g)).double().requires_grad_()
    mu_b = torch.randn(N, generator=g, dtype=torch.float64, requires_grad=True)
    rho_b = (-1.0 + 0.5 * torch.randn(N, generator=g)).double().requires_grad_()
    dy = torch.randn(S * M, N, generator=g, dtype=torch.float64)
    zeta = lrt_ref.zeta_host(S, M, N, SEED, 12, layer_id)
    assert zeta.shape == (S * M, N) and not torch.equal(zeta[:M], zeta[M:2 * M])
    # element e = i * N + n of sample s on stream BF_LRT_STREAM | layer_id
    one = ops.philox_normal_host(1, SEED, 13, _C.BF_LRT_STREAM | layer_id, offset=2 * N + 5)
    assert zeta[M + 2, 5] == one.double()[0]
    y, pre, v = lrt_ref.forward(x, mu, rho, mu_b, rho_b, zeta, act)
    m, v2 = lrt_ref.moments(x, mu, rho, mu_b, rho_b)
    want = m + torch.sqrt(v2) * zeta  # the restatement is the formula
    assert torch.allclose(pre, want, rtol=1e-12, atol=1e-12)
    assert torch.allclose(y, lrt_ref.gelu(want) if act else want, rtol=1e-12, atol=1e-12)
    (y * dy).sum().backward()
    hand = lrt_ref.backward(x.detach(), dy, mu.detach(), rho.detach(), mu_b.detach(), rho_b.detach(), zeta, v.detach(),
                            pre.detach() if act else None)
    for name, grad in (("dx", x.grad), ("dmu", mu.grad), ("drho", rho.grad), ("dmu_b", mu_b.grad), ("drho_b", rho_b.grad)):
        assert torch.allclose(hand[name], grad, rtol=1e-9, atol=1e-12), name


def test_reference_zero_variance_row():
    """A zero input row without a bias: v == 0 there, dv = 0, nothing non-finite."""
    S, M, N, K = 2, 3, 8, 8
    g = torch.Generator().manual_seed(5)
    x = torch.randn(S * M, K, generator=g, dtype=torch.float64)
    x[1] = 0.0
    x.requires_grad_()
    mu = torch.randn(N, K, generator=g, dtype=torch.float64, requires_grad=True)
    rho = (-2.0 + torch.randn(N, K, generator=g)).double().requires_grad_()
    dy = torch.randn(S * M, N, generator=g, dtype=torch.float64)
    zeta = lrt_ref.zeta_host(S, M, N, SEED, 0, 1)
    y, pre, v = lrt_ref.forward(x, mu, rho, None, None, zeta)
    assert torch.equal(v[1], torch.zeros(N, dtype=torch.float64)) and torch.equal(y[1], torch.zeros(N, dtype=torch.float64))
    hand = lrt_ref.backward(x.detach(), dy, mu.detach(), rho.detach(), None, None, zeta, v.detach())
    assert torch.equal(hand["dv"][1], torch.zeros(N, dtype=torch.float64))
    assert all(torch.isfinite(t).all() for t in hand.values() if t is not None)
    assert hand["dmu_b"] is None and hand["drho_b"] is None
    # autograd agrees on every other row's contribution: the zero row adds dm mu to dx and nothing to the parameters
    keep = torch.ones(S * M, dtype=torch.bool)
    keep[1] = False
    xk = x.detach()[keep].clone().requires_grad_()
    yk, _, _ = lrt_ref.forward(xk, mu, rho, None, None, zeta[keep])
    (yk * dy[keep]).sum().backward()
    assert torch.allclose(hand["dx"][keep], xk.grad, rtol=1e-9, atol=1e-12)
    assert torch.allclose(hand["dx"][1], dy[1] @ mu.detach(), rtol=1e-12, atol=1e-12)
    assert torch.allclose(hand["drho"], rho.grad, rtol=1e-9, atol=1e-12)
    # dmu: the zero row multiplies dm by x = 0
    assert torch.allclose(hand["dmu"], mu.grad, rtol=1e-9, atol=1e-12)


def test_variance_reduction_of_the_estimator():
    """K 64, N 32, M 256, S 1, x ~ N(0.5, 1), sigma = 0.05 |mu| + 1e-4, loss 1/2 |y - t|^2, 64 seeds: the summed variances of
    dmu and drho under local reparameterisation are at most HALF of the weight-space estimator's (this restatement, with
    mu ~ N(0, 1/K) and t ~ N(0, 1), gives 1/14.7 and 1/107), and the two mean dmu differ by less than 1 % of its norm (0.66 %)."""
    K, N, M, seeds = 64, 32, 256, 64
    g = torch.Generator().manual_seed(6)
    x = (0.5 + torch.randn(M, K, generator=g)).double()
    mu = (torch.randn(N, K, generator=g) / K ** 0.5).double()
    sigma = 0.05 * mu.abs() + 1e-4
    rho = torch.log(torch.expm1(sigma))
    t = torch.randn(M, N, generator=g).double()
    ws, lr = [], []
    for seed in range(seeds):
        eps = ops.philox_normal_host(N * K, 1000 + seed, 0, 0).double().view(N, K)
        zeta = lrt_ref.zeta_host(1, M, N, 1000 + seed, 0, 0)
        ws.append(torch.stack(lrt_ref.weight_space_grads(x, t, mu, rho, eps)))
        lr.append(torch.stack(lrt_ref.local_grads(x, t, mu, rho, zeta)))
    ws, lr = torch.stack(ws), torch.stack(lr)  # [seeds, 2, N, K]
    var_w, var_l = ws.var(0).sum((1, 2)), lr.var(0).sum((1, 2))
    ratio = var_l / var_w
    print(f"variance ratio local / weight-space: dmu {float(ratio[0]):.4f} (1/{1 / float(ratio[0]):.1f}), "
          f"drho {float(ratio[1]):.4f} (1/{1 / float(ratio[1]):.1f})")
    assert float(ratio[0]) <= 0.5 and float(ratio[1]) <= 0.5
    mean_w, mean_l = ws.mean(0)[0], lr.mean(0)[0]
    rel = float((mean_w - mean_l).norm() / mean_w.norm())
    print(f"mean dmu, relative difference of the two estimators: {rel:.2e}")
    assert rel < 0.01


def test_analytic_kl_is_the_mean_of_the_sampled_logprobs():
    """bf_kl_gaussian's closed form (the ref) against the mean over 4096 host-eps draws of the oracle's per-sample log-probs,
    within 5 standard errors."""
    N, K, draws = 6, 8, 4096
    g = torch.Generator().manual_seed(7)
    mu_w, mu_b = 0.2 * torch.randn(N, K, generator=g), 0.2 * torch.randn(N, generator=g)
    rho_w, rho_b = -3.0 + 0.3 * torch.randn(N, K, generator=g), -3.0 + 0.3 * torch.randn(N, generator=g)
    pw = ("gaussian", mu_w + 0.05 * torch.randn(N, K, generator=g), torch.full((N, K), -2.0))
    pb = ("gaussian", mu_b + 0.05 * torch.randn(N, generator=g), torch.full((N,), -2.0))
    lp, lq = [], []
    for s in range(draws):
        eps_w = ops.philox_normal_host(N * K, SEED, s, 0).view(N, K)
        eps_b = ops.philox_normal_host(N, SEED, s, 1)
        a, b = bo.linear_logprobs_f64(mu_w, rho_w, mu_b, rho_b, eps_w, eps_b, pw, pb)
        lp.append(a)
        lq.append(b)
    lp, lq = torch.tensor(lp, dtype=torch.float64), torch.tensor(lq, dtype=torch.float64)
    wp, wq, _, _ = lrt_ref.kl_gaussian(mu_w, rho_w, pw[1], pw[2])
    bp, bq, _, _ = lrt_ref.kl_gaussian(mu_b, rho_b, pb[1], pb[2])
    for name, closed, drawn in (("log_prior", wp + bp, lp), ("log_q", wq + bq, lq)):
        se = float(drawn.std() / draws ** 0.5)
        print(f"{name}: closed form {closed:.6f}, sampled mean {float(drawn.mean()):.6f}, standard error {se:.2e}")
        assert abs(closed - float(drawn.mean())) <= 5 * se, name


def _mlp(delta=0.05):
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(16, 24), torch.nn.GELU(), torch.nn.Linear(24, 8))
    return bf.to_bayesian(net, delta=delta)


def test_switch_sets_every_linear_and_returns_the_count():
    model = _mlp()
    layers = [m for m in model.modules() if isinstance(m, bnn.Linear)]
    assert len(layers) == 2 and not any(l.local for l in layers)
    assert bf.local_reparameterization(model) == 2
    assert all(l.local and l.local_kl == "sampled" for l in layers)
    assert bf.local_reparameterization(model, True, kl="analytic") == 2
    assert all(l.local_kl == "analytic" for l in layers)
    assert bf.local_reparameterization(model, False) == 2
    assert not any(l.local for l in layers) and all(l.local_kl == "sampled" for l in layers)
    assert "local_reparameterization" in bf.__all__
    with pytest.raises(ValueError, match="sampled"):
        bf.local_reparameterization(model, True, kl="exact")
    # LoRA adapters and embeddings are not touched
    lora = bnn.Model(torch.nn.Sequential(bnn.LoRALinear(8, 8, r=8)))
    assert bf.local_reparameterization(lora) == 0


def test_analytic_kl_refusals():
    with pytest.raises(ValueError, match="Gaussian prior"):
        bf.local_reparameterization(_mlp(delta=None), True, kl="analytic")  # the default mixture prior
    bf.set_kl_gradient(True)
    try:
        with pytest.raises(ValueError, match="set_kl_gradient"):
            bf.local_reparameterization(_mlp(), True, kl="analytic")
        assert bf.local_reparameterization(_mlp(), True) == 2  # kl="sampled" works unchanged
    finally:
        bf.set_kl_gradient(False)


def test_generation_and_kept_weights_refuse_local_layers():
    model = _mlp().eval()
    bf.local_reparameterization(model)
    from bayeformers_amd.sampling import sample_generate

    with torch.no_grad():
        with pytest.raises(ValueError, match="local reparameterisation"):
            sample_generate(model, torch.zeros((1, 4), dtype=torch.long), samples=2, max_new_tokens=2)
        with model.monte_carlo(2):
            with pytest.raises(ValueError, match="local reparameterisation"):
                with model.pinned_samples(keep_weights=True):
                    pass


def test_lrt_supported_is_the_kernels_class():
    assert ops.lrt_supported(torch.bfloat16, 8, 8) and ops.lrt_supported(torch.bfloat16, 200, 136)
    assert not ops.lrt_supported(torch.float16, 64, 64)
    assert not ops.lrt_supported(torch.float32, 64, 64)
    assert not ops.lrt_supported(torch.bfloat16, 60, 64)
    assert not ops.lrt_supported(torch.bfloat16, 64, 60)
    assert set(ops.LRT_CALLS) >= {"fwd", "bwd", "composite_fwd", "composite_bwd"}


def test_header_declares_the_bound_entries():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "bayeformers_amd_lrt.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(bf_(?:lrt|kl_gaussian|sample_logprob_like)\w*)\s*\(", text))
    assert declared == set(_C.LRT_SYMBOLS)
    others = [_C.SYMBOLS, _C.SOFTCAP_SYMBOLS, _C.FAMILY_BLOCK_SYMBOLS, _C.FAMILY_BLOCK_BWD_SYMBOLS, _C.PACKED_SYMBOLS,
              _C.FP8_SYMBOLS, _C.KV8_SYMBOLS, _C.CHUNK_SYMBOLS, _C.ENCODER_ANY_SYMBOLS, _C.LORA_SYMBOLS]
    assert not any(set(_C.LRT_SYMBOLS) & set(t) for t in others)
    philox = open(os.path.join(root, "bayeformers_amd", "csrc", "bf_philox.h")).read()
    assert re.search(r"#define\s+BF_LRT_STREAM\s+0x20000000u", philox) and _C.BF_LRT_STREAM == 0x20000000
    lib = _C.lib()
    for name, (res, args) in _C.LRT_SYMBOLS.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    # the size twins answer without a device; refusals come before any launch and name the condition
    assert lib.bf_lrt_grad_prepare_workspace_bytes(64, 8) > 0 and lib.bf_kl_gaussian_workspace_bytes() > 0
    for (dt, N, K), word in (((_C.BF_DT_BF16, 60, 64), "N % 8 == 0"), ((_C.BF_DT_BF16, 64, 60), "K % 8 == 0"),
                             ((_C.BF_DT_F16, 64, 64), "BF_DT_BF16")):
        rc = lib.bf_lrt_operands(None, None, None, None, None, None, dt, N, K, None)
        assert rc == 1 and word in lib.bf_last_error().decode()
    rc = lib.bf_lrt_combine(None, None, None, None, None, _C.BF_DT_BF16, 1, 1, 8, 7, 0, 0, 0, None)
    assert rc == 1 and "activation" in lib.bf_last_error().decode()
