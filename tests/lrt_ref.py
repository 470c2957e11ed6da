"""A float64 restatement of the local reparameterisation contract (include/bayeformers_amd_lrt.h), for the tests.

    m = x mu^T + mu_b        v = x^2 (sigma^2)^T + sigma_b^2        y[s][i][n] = act(m + sqrt(v) * zeta),  sigma = softplus(rho)
    dm = g,  dv = g zeta / (2 sqrt(v)) (0 where v == 0),  g = dy * act'(pre)
    dx = dm mu + 2 x o (dv sigma^2),  dmu = dm^T x,  dsigma^2 = dv^T x^2,  drho = dsigma^2 * 2 sigma sigmoid(rho)
    dmu_b = colsum(dm),  drho_b = colsum(dv) * 2 sigma_b sigmoid(rho_b)

zeta comes from the library's host twin of the device generator (bf_philox_normal_host) on stream BF_LRT_STREAM | layer_id:
element e = i * N + n of sample s.  Everything else is torch on the CPU.  Also the weight-space estimator's gradients on
host eps (for the variance comparison) and the closed-form Gaussian KL terms of bf_kl_gaussian.
"""
import math

import torch

from bayeformers_amd import _C, ops

LOG_SQRT_2PI = 0.5 * math.log(2.0 * math.pi)


def zeta_host(S: int, M: int, N: int, seed: int, sample_base: int, layer_id: int) -> torch.Tensor:
    """[S*M, N] float64: zeta of samples sample_base .. sample_base + S - 1 of layer `layer_id`."""
    stream = _C.BF_LRT_STREAM | int(layer_id)
    return torch.cat([ops.philox_normal_host(M * N, seed, sample_base + s, stream).double().view(M, N) for s in range(S)])


def gelu(x: torch.Tensor) -> torch.Tensor:
    return 0.5 * x * torch.erfc(-x / math.sqrt(2.0))


def gelu_grad(x: torch.Tensor) -> torch.Tensor:
    return 0.5 * torch.erfc(-x / math.sqrt(2.0)) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def moments(x, mu, rho, mu_b=None, rho_b=None):
    """(m, v) [R, N] in float64."""
    x, mu = x.double(), mu.double()
    sig2 = torch.nn.functional.softplus(rho.double()) ** 2
    m, v = x @ mu.t(), (x * x) @ sig2.t()
    if mu_b is not None:
        m = m + mu_b.double()
        v = v + torch.nn.functional.softplus(rho_b.double()) ** 2
    return m, v


def combine(m, v, zeta, act: bool = False):
    """(y, pre) from the moments."""
    pre = m.double() + torch.sqrt(v.double()) * zeta.double()
    return (gelu(pre) if act else pre), pre


def forward(x, mu, rho, mu_b, rho_b, zeta, act: bool = False):
    """(y, pre, v) [R, N] in float64; differentiable in x, mu, rho, mu_b, rho_b."""
    m, v = moments(x, mu, rho, mu_b, rho_b)
    y, pre = combine(m, v, zeta, act)
    return y, pre, v


def grad_prepare(dy, zeta, sd, pre=None):
    """(dm, dv): g = dy (* gelu'(pre)), dv = g zeta / (2 sd), 0 where sd == 0."""
    g = dy.double()
    if pre is not None:
        g = g * gelu_grad(pre.double())
    sd = sd.double()
    safe = torch.where(sd > 0, sd, torch.ones_like(sd))
    dv = torch.where(sd > 0, g * zeta.double() / (2.0 * safe), torch.zeros_like(g))
    return g, dv


def backward(x, dy, mu, rho, mu_b, rho_b, zeta, v, pre=None):
    """The hand-written gradients in float64: dict with dx, dmu, drho, dmu_b, drho_b (the bias entries None without one)."""
    x, mu, rho = x.double(), mu.double(), rho.double()
    sigma = torch.nn.functional.softplus(rho)
    dm, dv = grad_prepare(dy, zeta, torch.sqrt(v.double()), pre)
    out = {"dm": dm, "dv": dv,
           "dx": dm @ mu + 2.0 * x * (dv @ (sigma * sigma)),
           "dmu": dm.t() @ x,
           "drho": (dv.t() @ (x * x)) * 2.0 * sigma * torch.sigmoid(rho),
           "dmu_b": None, "drho_b": None}
    if mu_b is not None:
        rb = rho_b.double()
        out["dmu_b"] = dm.sum(0)
        out["drho_b"] = dv.sum(0) * 2.0 * torch.nn.functional.softplus(rb) * torch.sigmoid(rb)
    return out


def weight_space_grads(x, t, mu, rho, eps):
    """(dmu, drho) of the weight-space estimator for the loss 1/2 |y - t|^2, y = x (mu + sigma eps)^T, one sample, float64."""
    x, t, mu, rho, eps = x.double(), t.double(), mu.double(), rho.double(), eps.double()
    sigma = torch.nn.functional.softplus(rho)
    dw = ((x @ (mu + sigma * eps).t()) - t).t() @ x
    return dw, dw * eps * torch.sigmoid(rho)


def local_grads(x, t, mu, rho, zeta):
    """(dmu, drho) of the local reparameterisation estimator for the same loss, one sample, float64."""
    y, _, v = forward(x, mu, rho, None, None, zeta)
    g = backward(x, y - t.double(), mu, rho, None, None, zeta, v)
    return g["dmu"], g["drho"]


def kl_gaussian(mu, rho, prior_mu, prior_rho):
    """(E_q log p, E_q log q) of one tensor under the prior N(prior_mu, softplus(prior_rho)), closed form, float64."""
    sg = torch.nn.functional.softplus(rho.double())
    sp = torch.nn.functional.softplus(prior_rho.double())
    d = mu.double() - prior_mu.double()
    lp = -(torch.log(sp) + LOG_SQRT_2PI + (sg * sg + d * d) / (2.0 * sp * sp))
    lq = -(torch.log(sg) + LOG_SQRT_2PI + 0.5)
    return float(lp.sum()), float(lq.sum()), float(lp.abs().sum()), float(lq.abs().sum())
