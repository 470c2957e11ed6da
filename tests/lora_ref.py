"""A float64 restatement of the Bayesian LoRA contract (include/bayeformers_amd_lora.h), for the tests.

    A_s  = mu_A + softplus(rho_A) * eps(seed, sample_base + s, stream 2 * layer_id, e)
    h[s] = x[s] A_s^T
    y[s] = x[s] W0^T + b0 + scale * h[s] B^T
    g[s] = dy[s] B;  dx[s] = dy[s] W0 + scale * g[s] A_s;  dA_s = scale * g[s]^T x[s];  dB = scale * sum_s dy[s]^T h[s]
    dmu_A = sum_s dA_s;  drho_A = (sum_s dA_s o eps_s) o softplus'(rho_A)

eps comes from the library's host twin of the device generator (bf_philox_normal_host); everything else is torch on the CPU.
"""
import torch

from bayeformers_amd import ops


def eps_host(shape, seed: int, sample_base: int, S: int, stream_id: int) -> torch.Tensor:
    """[S, *shape] float64: the epsilon of samples sample_base .. sample_base + S - 1 on Philox stream `stream_id`."""
    n = 1
    for d in shape:
        n *= int(d)
    return torch.stack([ops.philox_normal_host(n, seed, sample_base + s, stream_id).double().view(*shape) for s in range(S)])


def sample_a(mu: torch.Tensor, rho: torch.Tensor, eps: torch.Tensor) -> torch.Tensor:
    """A_s [S, r, K] float64.  The device forms mu + softplus(rho) * eps in fp32; so does this, before widening."""
    sigma = torch.nn.functional.softplus(rho.float())
    return (mu.float()[None] + sigma[None] * eps.float()).double()


def forward(x, a_s, b, w0, b0, scale: float, S: int):
    """(y [S*M, N], h [S*M, r]) in float64.  x: [S*M, K]; a_s: [S, r, K]; b: [N, r]; w0: [N, K]; b0: [N] or None."""
    x, a_s, b, w0 = x.double(), a_s.double(), b.double(), w0.double()
    M = x.shape[0] // S
    h = torch.bmm(x.view(S, M, -1), a_s.transpose(1, 2))
    y = x @ w0.t()
    if b0 is not None:
        y = y + b0.double()
    y = y.view(S, M, -1) + scale * (h @ b.t())
    return y.reshape(S * M, -1), h.reshape(S * M, -1)


def backward(x, dy, a_s, b, w0, scale: float, S: int, eps=None, rho=None):
    """The hand-written gradients in float64: dict with dx [S*M, K], dA [S, r, K], dB [N, r], g [S*M, r] and, given eps
    [S, r, K] and rho [r, K], dmu / drho [r, K]."""
    x, dy, a_s, b, w0 = x.double(), dy.double(), a_s.double(), b.double(), w0.double()
    M = x.shape[0] // S
    xs, dys = x.view(S, M, -1), dy.view(S, M, -1)
    g = dys @ b
    h = torch.bmm(xs, a_s.transpose(1, 2))
    out = {"g": g.reshape(S * M, -1),
           "dx": (dy @ w0).view(S, M, -1).add(scale * torch.bmm(g, a_s)).reshape(S * M, -1),
           "dA": scale * torch.bmm(g.transpose(1, 2), xs),
           "dB": scale * torch.einsum("smn,smr->nr", dys, h)}
    if eps is not None:
        out["dmu"] = out["dA"].sum(0)
        out["drho"] = (out["dA"] * eps.double()).sum(0) * torch.sigmoid(rho.double())
    return out
