"""Host-side plumbing between torch tensors and the C-ABI (include/bayeformers_amd.h).

torch is used here for device memory, the current HIP stream and autograd bookkeeping only; every arithmetic
step of the Monte-Carlo forward path runs in the HIP kernels of csrc/.  There is no CPU fallback: tensors that
are not on a ROCm device raise.
"""
import ctypes
import math
from typing import Optional, Union

import torch
from torch import Tensor

from . import _C
from . import random as bfr

_TORCH2BF = {torch.float32: _C.BF_DT_F32, torch.bfloat16: _C.BF_DT_BF16, torch.float16: _C.BF_DT_F16}

_WORKSPACES = {}


def _require_device(t: Tensor, what: str) -> None:
    if not t.is_cuda:
        raise _C.BayeFormersAMDError(
            f"{what} lives on '{t.device}': the bayeformers_amd forward path runs only on a ROCm device "
            "(HIP kernels, no CPU fallback) — move the module and its inputs to 'cuda'")


def _stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


def workspace(device: torch.device, nbytes: int) -> Tensor:
    """Per-(device, stream) scratch buffer, grown on demand (stream-ordered reuse is safe on one stream)."""
    key = (device.index if device.index is not None else torch.cuda.current_device(), _stream_ptr())
    ws = _WORKSPACES.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        _WORKSPACES[key] = ws
    return ws


def philox_normal_host(n: int, seed: int, sample: int, stream_id: int, offset: int = 0) -> Tensor:
    """Host twin of the device epsilon (bf_philox_normal_host): fp32 CPU tensor of n normals."""
    out = torch.empty(int(n), dtype=torch.float32)
    _C.check(_C.lib().bf_philox_normal_host(out.data_ptr(), int(n), int(seed), int(sample) & 0xFFFFFFFF,
                                            int(stream_id), int(offset)), "bf_philox_normal_host")
    return out


def fused_small_rows(N: int, K: int) -> int:
    """Rows per sample up to which bf_linear_fwd runs an N x K layer as ONE fused kernel (bf_fused_small_rows_for: the
    measured crossover, capped by bf_set_fused_small_max_rows)."""
    return _C.lib().bf_fused_small_rows_for(int(N), int(K))


def philox_normal(n: int, S: int, seed: int, sample_base: int, stream_id: int, device="cuda") -> Tensor:
    """Device epsilon: [S, n] fp32 (test hook for the RNG contract)."""
    out = torch.empty((int(S), int(n)), dtype=torch.float32, device=device)
    _C.check(_C.lib().bf_philox_normal(out.data_ptr(), int(n), int(S), int(seed), int(sample_base) & 0xFFFFFFFF,
                                       int(stream_id), _stream_ptr()), "bf_philox_normal")
    return out


def prior_alias(gaussian, prior) -> Optional[float]:
    """sigma_p when `prior` is the MOPED prior of a FROZEN mean — Gaussian(mu = the posterior's mean, rho = one constant),
    /root/reference/bayeformers/nn/layers/linear.py:147-150 with freeze=True — else None.  The sampling kernel then reads
    8 instead of 16 bytes per scalar (bf_prior_t.pi == 1).  Checked on the tensors' CONTENTS (after a device move the two
    means are equal copies, no longer one storage), once per state: the verdict is cached with the tensors' addresses and
    version counters, so an in-place edit of either (an optimizer step on a trainable mean, load_state_dict) is seen and
    re-checked.  A trainable mean is never aliased: it leaves the prior's at its first update.
    An edit through `.data` (the reference's idiom, layers/linear.py:140-150) moves no version counter: the sampling kernels
    therefore spot-check the assertion on the device (one element per wave against prior.mu / prior.rho), poison the
    log-prior and bump the library's stale counter when it fails; `stale_priors_seen()` notices that at the next forward
    and `invalidate_caches(model)` drops every cached verdict."""
    mu, pmu, prho = gaussian.mu, prior.mu, prior.rho
    if mu.requires_grad or pmu.shape != mu.shape or prho.shape != mu.shape or pmu.dtype != torch.float32:
        return None
    state = (mu.data_ptr(), mu._version, pmu.data_ptr(), pmu._version, prho.data_ptr(), prho._version, bfr.STATE.stale_epoch)
    hit = getattr(prior, "_bf_alias", None)
    if hit is not None and hit[0] == state:
        return hit[1]
    with torch.no_grad():
        sigma_p, rho_p = None, 0.0
        lo, hi = torch.aminmax(prho)
        if bool(lo == hi) and (pmu.data_ptr() == mu.data_ptr() or torch.equal(pmu, mu)):
            sigma_p, rho_p = float(torch.nn.functional.softplus(lo.float())), float(lo)
            if not (sigma_p > 0.0 and sigma_p < float("inf")):
                sigma_p = None
    prior._bf_alias = (state, sigma_p, rho_p)
    return sigma_p


_WARNED_EPOCH = [0]


def stale_epoch() -> int:
    """The library's stale-prior counter (bf_stale_counter) as of the running forward: some kernel bumps it when it finds a
    prior's baked constants — an asserted MOPED alias, a mixture's pi / sigma1 / sigma2 — different from the tensors they
    were read from (an in-place edit through `.data`).  Every cached copy of prior state (`prior_alias`,
    `ScaledGaussianMixture.constants`, the sampling plan) remembers the epoch it was made in and is void in a later one —
    whichever module, model or bare layer it belongs to.  `refresh_stale_epoch()` reads the counter (a word of pinned host
    memory: no synchronisation) once per forward."""
    return bfr.STATE.stale_epoch


def refresh_stale_epoch() -> None:
    now = _C.stale_counter()
    if now != bfr.STATE.stale_epoch:
        bfr.STATE.stale_epoch = now
        if now != _WARNED_EPOCH[0]:
            import warnings

            _WARNED_EPOCH[0] = now
            warnings.warn("bayeformers_amd: a prior's tensors were edited in place through `.data` after a forward had "
                          "cached their state; the log_prior of the forward(s) since the edit is NaN — every cached copy "
                          "is void from now on (call bayeformers_amd.invalidate_caches(model) right after such an edit)")


def invalidate_caches(module) -> None:
    """Forget every host-side copy of `module`'s prior state: the MOPED-alias verdicts (`prior_alias`), the mixture priors'
    constants (`ScaledGaussianMixture.constants`) and the sampling plans built on them.  Call it after editing a prior's or
    a frozen mean's tensors in place through `.data` — every other edit (optimizer steps, load_state_dict, `.to()`,
    in-place ops on the parameter itself) is seen through the version counters and addresses."""
    from .nn.model import Model
    from .nn.parameters.gaussian import Gaussian, ScaledGaussianMixture

    for m in module.modules():
        if isinstance(m, Gaussian):
            m.__dict__.pop("_bf_alias", None)
        elif isinstance(m, ScaledGaussianMixture):
            m._consts = None
        elif isinstance(m, Model):
            m._plan = None
        m.__dict__.pop("_mean_cache", None)  # (a bnn.Linear's 16-bit copy of its posterior mean: Model.posterior_mean)
        m.__dict__.pop("_mean_cache_lrt", None)  # (... and of [mu; sigma^2]: a local layer's forwards without gradients)


def fill_prior(dst: "_C.bf_prior_t", prior, gaussian=None) -> bool:
    """Describe a prior module to the kernels.  Returns False for a user-defined Parameter (generic path)."""
    from .nn.parameters.base import NoneParameter
    from .nn.parameters.gaussian import Gaussian, ScaledGaussianMixture

    if isinstance(prior, ScaledGaussianMixture):
        pi, s1, s2 = prior.constants()
        dst.kind, dst.pi, dst.sigma1, dst.sigma2 = _C.BF_PRIOR_MIXTURE, pi, s1, s2
        dst.d_mu = dst.d_rho = None
        # the kernels compare the three values with the device scalars they are a copy of (an edit through .data is
        # invisible to the host-side cache; host-resident scalars are re-read by constants() on every call instead)
        on_dev = prior.pi.is_cuda and prior.sigma1.is_cuda and prior.sigma2.is_cuda
        dst.d_pi, dst.d_sigma1, dst.d_sigma2 = ((prior.pi.data_ptr(), prior.sigma1.data_ptr(), prior.sigma2.data_ptr())
                                                if on_dev else (None, None, None))
        return True
    if isinstance(prior, Gaussian):
        _require_device(prior.mu, "prior.mu")
        dst.kind = _C.BF_PRIOR_GAUSSIAN
        dst.d_mu, dst.d_rho = prior.mu.data_ptr(), prior.rho.data_ptr()
        sigma_p = prior_alias(gaussian, prior) if gaussian is not None else None
        # (asserted alias: sigma2 carries the constant rho the kernels spot-check prior.rho against)
        dst.pi, dst.sigma1, dst.sigma2 = (1.0, sigma_p, prior._bf_alias[2]) if sigma_p is not None else (0.0, 0.0, 0.0)
        dst.d_pi = dst.d_sigma1 = dst.d_sigma2 = None
        return True
    if prior is None or isinstance(prior, NoneParameter):
        dst.kind = _C.BF_PRIOR_NONE
        dst.d_mu = dst.d_rho = dst.d_pi = dst.d_sigma1 = dst.d_sigma2 = None
        return True
    return False


def fill_tensor(dst: "_C.bf_tensor_t", gaussian, prior, stream_id: int) -> bool:
    mu, rho = gaussian.mu, gaussian.rho
    _require_device(mu, "mu")
    if not (mu.is_contiguous() and rho.is_contiguous() and mu.dtype == torch.float32 and rho.dtype == torch.float32):
        raise _C.BayeFormersAMDError("mu/rho must be contiguous fp32 tensors")
    dst.d_mu, dst.d_rho, dst.n = mu.data_ptr(), rho.data_ptr(), mu.numel()
    dst.stream_id = stream_id
    dst.d_sample_out = None
    dst.out_dtype = _C.BF_DT_F32
    if isinstance(prior, type(gaussian)) and prior.mu.numel() != mu.numel():
        raise _C.BayeFormersAMDError("Gaussian prior must have the shape of the parameter it is a prior of")
    return fill_prior(dst.prior, prior, gaussian)


def sample_logprob(gaussians, priors, stream_ids, S: int, seed: int, sample_base: int, out_dtype=None, like_dtype=None):
    """Fused sampling + log-probs of 1 or 2 Gaussian parameters (bf_sample_logprob).

    Returns (samples, logprob) where samples is a list of [S, *shape] tensors (or None when out_dtype is None)
    and logprob is a [S, 2] float64 tensor {log_prior, log_variational_posterior} summed over the parameters.
    like_dtype (with out_dtype None): nothing is written, and the log-probs have the bits of the per-layer forward that
    draws `like_dtype` weights (bf_sample_logprob_like)."""
    n = len(gaussians)
    arr = (_C.bf_tensor_t * n)()
    dev = gaussians[0].mu.device
    outs = []
    for i, (g, pr, sid) in enumerate(zip(gaussians, priors, stream_ids)):
        if not fill_tensor(arr[i], g, pr, sid):
            raise _C.BayeFormersAMDError("sample_logprob: user-defined priors go through Linear's generic path")
        if out_dtype is not None:
            o = torch.empty((S,) + tuple(g.mu.shape), dtype=out_dtype, device=dev)
            arr[i].d_sample_out, arr[i].out_dtype = o.data_ptr(), _TORCH2BF[out_dtype]
            outs.append(o)
    lib = _C.lib()
    need = lib.bf_sample_logprob_workspace_bytes(arr, n, S)
    ws = workspace(dev, need)
    lp = torch.empty((S, 2), dtype=torch.float64, device=dev)
    if out_dtype is None and like_dtype is not None:
        _C.check(lib.bf_sample_logprob_like(arr, n, S, seed, sample_base & 0xFFFFFFFF, lp.data_ptr(), ws.data_ptr(),
                                            ws.numel(), _TORCH2BF[like_dtype], _stream_ptr()), "bf_sample_logprob_like")
        return None, lp
    _C.check(lib.bf_sample_logprob(arr, n, S, seed, sample_base & 0xFFFFFFFF, lp.data_ptr(), ws.data_ptr(),
                                   ws.numel(), _stream_ptr()), "bf_sample_logprob")
    return (outs if out_dtype is not None else None), lp


def gemm_nt(x: Tensor, w: Tensor, bias: Optional[Tensor], S: int, M: int, N: int, K: int, x_sample_stride: int,
            y_dtype: torch.dtype, act: int = 0, out: Optional[Tensor] = None) -> Tensor:
    """y[s] = act(x[s] w[s]^T + bias[s]) on the matrix cores (bf_gemm_nt_act).  w: [S,N,K]; returns [S,M,N] (`out`: a
    contiguous [S,M,N] tensor of y_dtype to write into — a window of a larger sample-major buffer)."""
    y = out if out is not None else torch.empty((S, M, N), dtype=y_dtype, device=x.device)
    _C.check(_C.lib().bf_gemm_nt_act(x.data_ptr(), _TORCH2BF[x.dtype], x_sample_stride, w.data_ptr(),
                                     _TORCH2BF[w.dtype], bias.data_ptr() if bias is not None else None, y.data_ptr(),
                                     _TORCH2BF[y_dtype], S, M, N, K, act, _stream_ptr()), "bf_gemm_nt_act")
    return y


def gemm_nt_act_pre(x: Tensor, w: Tensor, bias: Optional[Tensor], S: int, M: int, N: int, K: int, x_sample_stride: int,
                    y_dtype: torch.dtype, act: int):
    """(act(y), y) with y[s] = x[s] w[s]^T + bias[s] (bf_gemm_nt_act_pre): the forward of a training step keeps the
    pre-activation for the backward of the fused activation.  Both [S,M,N]."""
    y = torch.empty((S, M, N), dtype=y_dtype, device=x.device)
    pre = torch.empty((S, M, N), dtype=y_dtype, device=x.device)
    _C.check(_C.lib().bf_gemm_nt_act_pre(x.data_ptr(), _TORCH2BF[x.dtype], x_sample_stride, w.data_ptr(),
                                         _TORCH2BF[w.dtype], bias.data_ptr() if bias is not None else None,
                                         y.data_ptr(), pre.data_ptr(), _TORCH2BF[y_dtype], S, M, N, K, act,
                                         _stream_ptr()), "bf_gemm_nt_act_pre")
    return y, pre


def gemm_nt_layers(x: Tensor, w: Tensor, bias: Optional[Tensor], L: int, S: int, M: int, N: int, K: int,
                   x_sample_stride: int, y_dtype: torch.dtype, act: int = 0) -> Tensor:
    """y[l][s] = act(x[s] w[l][s]^T + bias[l][s]) for L layers sharing x, one launch (bf_gemm_nt_layers).
    w: [L,S,N,K]; bias: [L,S,N] fp32 or None; returns [L,S,M,N]."""
    y = torch.empty((L, S, M, N), dtype=y_dtype, device=x.device)
    _C.check(_C.lib().bf_gemm_nt_layers(x.data_ptr(), _TORCH2BF[x.dtype], x_sample_stride, w.data_ptr(),
                                        _TORCH2BF[w.dtype], bias.data_ptr() if bias is not None else None,
                                        y.data_ptr(), _TORCH2BF[y_dtype], L, S, M, N, K, act, _stream_ptr()),
             "bf_gemm_nt_layers")
    return y


def gemm_tn(a: Tensor, b: Tensor) -> Tensor:
    """out[i] = a[i]^T b[i] in fp32 (bf_gemm_tn): the weight-gradient GEMM dW = dy^T x.  a: [batch, Mc, N],
    b: [batch, Mc, K], 16-bit; returns [batch, N, K] float32."""
    _require_device(a, "a")
    batch, Mc, N = a.shape
    K = b.shape[2]
    if b.shape[:2] != a.shape[:2] or a.dtype != b.dtype or not (a.is_contiguous() and b.is_contiguous()):
        raise _C.BayeFormersAMDError("gemm_tn: a [batch,Mc,N] and b [batch,Mc,K] must be contiguous, same dtype")
    out = torch.empty((batch, N, K), dtype=torch.float32, device=a.device)
    _C.check(_C.lib().bf_gemm_tn(a.data_ptr(), b.data_ptr(), out.data_ptr(), _TORCH2BF[a.dtype], batch, Mc, N, K,
                                 _stream_ptr()), "bf_gemm_tn")
    return out


def gemm_nn(x: Tensor, w: Tensor) -> Tensor:
    """y[s] = x[s] w[s] (bf_gemm_nn): the input-gradient GEMM dx = dy W_s.  x: [S, M, N], w: [S, N, K], 16-bit;
    returns [S, M, K] of the same dtype."""
    _require_device(x, "x")
    S, M, N = x.shape
    K = w.shape[2]
    if w.shape[:2] != (S, N) or x.dtype != w.dtype or not (x.is_contiguous() and w.is_contiguous()):
        raise _C.BayeFormersAMDError("gemm_nn: x [S,M,N] and w [S,N,K] must be contiguous, same dtype")
    y = torch.empty((S, M, K), dtype=x.dtype, device=x.device)
    _C.check(_C.lib().bf_gemm_nn(x.data_ptr(), w.data_ptr(), y.data_ptr(), _TORCH2BF[x.dtype], S, M, N, K,
                                 _stream_ptr()), "bf_gemm_nn")
    return y


def gemm_nn_actgrad_supported(x: Tensor, w: Tensor, pre: Tensor) -> bool:
    S, M, N = x.shape
    K = w.shape[2]
    if not (x.is_cuda and x.dtype in (torch.bfloat16, torch.float16) and w.dtype == x.dtype and pre.dtype == x.dtype
            and x.is_contiguous() and w.is_contiguous() and pre.is_contiguous() and pre.numel() == S * M * K):
        return False
    return bool(_C.lib().bf_gemm_nn_actgrad_supported(x.data_ptr(), w.data_ptr(), x.data_ptr(), pre.data_ptr(), _TORCH2BF[x.dtype],
                                                      S, M, N, K))


def gemm_nn_actgrad(x: Tensor, w: Tensor, pre: Tensor, act: int = 1) -> Tensor:
    """y[s] = (x[s] w[s]) o act'(pre[s]) (bf_gemm_nn_actgrad): the input-gradient GEMM of a layer whose input was act(pre), with
    the activation's derivative in its epilogue.  x: [S, M, N], w: [S, N, K], pre: [S, M, K] (or [S*M, K]); returns [S, M, K]."""
    S, M, N = x.shape
    K = w.shape[2]
    y = torch.empty((S, M, K), dtype=x.dtype, device=x.device)
    _C.check(_C.lib().bf_gemm_nn_actgrad(x.data_ptr(), w.data_ptr(), y.data_ptr(), pre.data_ptr(), _TORCH2BF[x.dtype], S, M, N, K,
                                         int(act), _stream_ptr()), "bf_gemm_nn_actgrad")
    return y


def gemm_nn_layers(x: Tensor, w: Tensor) -> Tensor:
    """y[s] = sum_l x[l][s] w[l][s] (bf_gemm_nn_layers): the one input gradient of L layers that read the same
    activations.  x: [L, S, M, N], w: [L, S, N, K], 16-bit; returns [S, M, K]."""
    _require_device(x, "x")
    L, S, M, N = x.shape
    K = w.shape[3]
    if w.shape[:3] != (L, S, N) or x.dtype != w.dtype or not (x.is_contiguous() and w.is_contiguous()):
        raise _C.BayeFormersAMDError("gemm_nn_layers: x [L,S,M,N] and w [L,S,N,K] must be contiguous, same dtype")
    y = torch.empty((S, M, K), dtype=x.dtype, device=x.device)
    _C.check(_C.lib().bf_gemm_nn_layers(x.data_ptr(), w.data_ptr(), y.data_ptr(), _TORCH2BF[x.dtype], L, S, M, N, K,
                                        _stream_ptr()), "bf_gemm_nn_layers")
    return y


class LinearPlan:
    """Cached ctypes descriptors of one bnn.Linear (pointers are refreshed per call; structs are reused).  A cache only:
    copying or pickling the layer starts it afresh (ctypes structs holding pointers can be neither)."""

    def __deepcopy__(self, memo):
        return LinearPlan()

    def __reduce__(self):
        return (LinearPlan, ())

    def __init__(self):
        self.w = _C.bf_tensor_t()
        self.b = _C.bf_tensor_t()


def linear_forward(layer, x: Tensor, S: int, seed: int, sample_base: int, lp_out: Tensor) -> Tensor:
    """Linear.forward for S samples: y[s] = x[s] W_s^T + b_s and lp_out[s] = {log_prior, log_q}.

    x: [S*M, K] (sample-major) or [M, K] with S == 1.  lp_out: [S, 2] float64 on x's device."""
    from .nn.parameters.base import NoneParameter

    _require_device(x, "input")
    K, N = layer.in_features, layer.out_features
    if x.dtype not in _TORCH2BF:
        raise _C.BayeFormersAMDError(f"unsupported input dtype {x.dtype}")
    if not x.is_contiguous():
        x = x.contiguous()
    rows = x.numel() // K
    if rows % S:
        raise _C.BayeFormersAMDError(f"input rows ({rows}) are not a multiple of the sample count S={S}")
    M = rows // S
    cdt = layer.compute_dtype or bfr.get_compute_dtype()
    if x.dtype != torch.float32 and x.dtype != cdt:
        raise _C.BayeFormersAMDError(f"input dtype {x.dtype} does not match compute dtype {cdt} (fp32 inputs always do)")
    if cdt == torch.float32 and x.dtype != torch.float32:
        raise _C.BayeFormersAMDError("compute dtype fp32 needs fp32 inputs")
    has_bias = not isinstance(layer.bias, NoneParameter)
    plan = layer._plan
    known = fill_tensor(plan.w, layer.weight, layer.weight_prior, 2 * layer.layer_id)
    if has_bias:
        known = fill_tensor(plan.b, layer.bias, layer.bias_prior, 2 * layer.layer_id + 1) and known
    if not known:
        return _linear_forward_generic(layer, x, S, M, N, K, seed, sample_base, lp_out, cdt, has_bias)
    lib = _C.lib()
    y = torch.empty((S * M, N), dtype=x.dtype, device=x.device)
    need = lib.bf_linear_fwd_workspace_bytes(S, M, N, K, int(has_bias), _TORCH2BF[cdt], _TORCH2BF[x.dtype])
    ws = workspace(x.device, need)
    _C.check(lib.bf_linear_fwd(x.data_ptr(), _TORCH2BF[x.dtype], M * K, ctypes.byref(plan.w),
                               ctypes.byref(plan.b) if has_bias else None, y.data_ptr(), _TORCH2BF[x.dtype],
                               _TORCH2BF[cdt], S, M, N, K, seed, sample_base & 0xFFFFFFFF, lp_out.data_ptr(),
                               ws.data_ptr(), ws.numel(), _stream_ptr()), "bf_linear_fwd")
    return y


def _linear_forward_generic(layer, x, S, M, N, K, seed, sample_base, lp_out, cdt, has_bias):
    """User-defined prior (any Parameter with log_prob): the kernels sample W_s/b_s in fp32 and produce log q;
    the prior's own log_prob is then called on each sample, as the reference does (layers/linear.py:99-100)."""
    from .nn.parameters.base import NoneParameter

    gs = [layer.weight] + ([layer.bias] if has_bias else [])
    sids = [2 * layer.layer_id] + ([2 * layer.layer_id + 1] if has_bias else [])
    outs, lp = sample_logprob(gs, [NoneParameter()] * len(gs), sids, S, seed, sample_base, out_dtype=torch.float32)
    for s in range(S):
        v = layer.weight_prior.log_prob(outs[0][s])
        if has_bias:
            v = v + layer.bias_prior.log_prob(outs[1][s])
        lp[s, 0] = v
    lp_out.copy_(lp)
    w = outs[0] if cdt == torch.float32 else outs[0].to(cdt)
    y = gemm_nt(x, w, outs[1] if has_bias else None, S, M, N, K, M * K, x.dtype)
    return y.view(S * M, N)


def planned_linear_forward(x: Tensor, w_s: Tensor, b_s: Optional[Tensor], S: int, N: int, K: int, act: int = 0,
                           want_pre: bool = False):
    """y[s] = act(x[s] W_s^T + b_s) with W_s/b_s already sampled by the model's cross-layer plan (plan.SamplePlan).
    want_pre: return (y, pre-activation) — what the backward of a fused activation needs."""
    _require_device(x, "input")
    if x.dtype not in _TORCH2BF:
        raise _C.BayeFormersAMDError(f"unsupported input dtype {x.dtype}")
    if x.dtype != torch.float32 and x.dtype != w_s.dtype:
        raise _C.BayeFormersAMDError(
            f"input dtype {x.dtype} does not match compute dtype {w_s.dtype} (fp32 inputs always do)")
    if not x.is_contiguous():
        x = x.contiguous()
    rows = x.numel() // K
    if rows % S:
        raise _C.BayeFormersAMDError(f"input rows ({rows}) are not a multiple of the sample count S={S}")
    M = rows // S
    if want_pre:
        y, pre = gemm_nt_act_pre(x, w_s, b_s, S, M, N, K, M * K, x.dtype, act)
        return y.view(S * M, N), pre.view(S * M, N)
    return gemm_nt(x, w_s, b_s, S, M, N, K, M * K, x.dtype, act).view(S * M, N)


# Rows per sample up to which a layer of a keep_weights block (nn.Model.pinned_samples) runs bf_gemm_nt_skinny rather than the
# tiled GEMM (bf_gemm_nt_act): the kernel takes up to bf_gemm_nt_skinny_max_rows() = 64, but at 64 rows the tiled GEMM is faster on
# the wide layers (32000 x 1024: 43 against 92 us at S 4); at 16 rows the skinny kernel wins or ties every layer of the DESIGN 4.5
# decoder but the head (46 against 41 us) — the measured crossover (profiles/kept_weights_decode.md).
SKINNY_ROWS = 16
SKINNY_CALLS = [0]  # launches of bf_gemm_nt_skinny through skinny_linear_forward (tests, diagnostics)


def skinny_supported(x: Tensor, w_s: Tensor, S: int, K: int) -> bool:
    """Does skinny_linear_forward take x ([S*M, K]) with these kept weights?  16-bit x of the weights' dtype, K % 32 == 0,
    1 <= M <= SKINNY_ROWS, 16-byte aligned operands."""
    if w_s.dtype not in (torch.bfloat16, torch.float16) or x.dtype != w_s.dtype or K % 32 or S > 65535:
        return False
    rows = x.shape[0]
    if rows % S or not 1 <= rows // S <= min(SKINNY_ROWS, _C.lib().bf_gemm_nt_skinny_max_rows()):
        return False
    return x.is_contiguous() and (x.data_ptr() | w_s.data_ptr()) % 16 == 0


def skinny_linear_forward(x: Tensor, w_s: Tensor, b_s: Optional[Tensor], S: int, N: int, K: int, act: int = 0,
                          x_sample_stride: Optional[int] = None, out: Optional[Tensor] = None) -> Tensor:
    """y[s] = act(x[s] W_s^T + b_s) for a few rows per sample on weights already in memory (bf_gemm_nt_skinny).  x: [S*M, K]
    (or any storage with `x_sample_stride` elements between samples), w_s: [S, N, K] 16-bit, b_s: [S, N] fp32 or None;
    returns [S*M, N] of x's dtype.  The split-K scratch comes from the stream's workspace."""
    _require_device(x, "input")
    lib = _C.lib()
    if x_sample_stride is None:
        if not x.is_contiguous():
            x = x.contiguous()
        rows = x.numel() // K
        if rows % S:
            raise _C.BayeFormersAMDError(f"input rows ({rows}) are not a multiple of the sample count S={S}")
        M = rows // S
        x_sample_stride = M * K
    else:
        M = x.shape[-2]
    y = out if out is not None else torch.empty((S * M, N), dtype=x.dtype, device=x.device)
    need = lib.bf_gemm_nt_skinny_workspace_bytes(S, M, N, K)
    ws = workspace(x.device, need) if need else None
    _C.check(lib.bf_gemm_nt_skinny(x.data_ptr(), _TORCH2BF[x.dtype], int(x_sample_stride), w_s.data_ptr(), _TORCH2BF[w_s.dtype],
                                   b_s.data_ptr() if b_s is not None else None, y.data_ptr(), _TORCH2BF[y.dtype], S, M, N, K,
                                   int(act), ws.data_ptr() if ws is not None else None, ws.numel() if ws is not None else 0,
                                   _stream_ptr()), "bf_gemm_nt_skinny")
    SKINNY_CALLS[0] += 1
    return y


SKINNY_FP8_CALLS = [0]  # launches of bf_gemm_nt_skinny_fp8 through skinny_linear_forward_fp8 (tests, diagnostics)


def _fp8_rows_check(what: str, S: int, N: int, K: int, **tensors) -> None:
    """Dtype, shape, device and contiguity of the operands of the FP8 row entries (include/bayeformers_amd_fp8.h)."""
    want = {"w": (torch.bfloat16, (S, N, K)), "center": (torch.bfloat16, (N, K)), "q": (torch.uint8, (S, N, K)),
            "scale": (torch.float32, (S, N))}
    for name, t in tensors.items():
        _require_device(t, name)
        dt, shape = want[name]
        if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
            raise _C.BayeFormersAMDError(f"{what}: {name} must be a contiguous {dt} tensor of shape {shape} (got {t.dtype} "
                                         f"{tuple(t.shape)}; fp16 and fp32 weights are not taken)")


def quantize_rows_fp8(w: Tensor, center: Tensor, q: Optional[Tensor] = None, scale: Optional[Tensor] = None):
    """Centred FP8 rows of sampled weights (bf_fp8_rows_quantize): w [S, N, K] bf16 draws, center [N, K] bf16 ->
    (q [S, N, K] uint8 holding e4m3fn bytes of w - center over a power-of-two scale per row, scale [S, N] fp32)."""
    S, N, K = w.shape
    q = torch.empty((S, N, K), dtype=torch.uint8, device=w.device) if q is None else q
    scale = torch.empty((S, N), dtype=torch.float32, device=w.device) if scale is None else scale
    _fp8_rows_check("quantize_rows_fp8", S, N, K, w=w, center=center, q=q, scale=scale)
    _C.check(_C.lib().bf_fp8_rows_quantize(w.data_ptr(), _C.BF_DT_BF16, center.data_ptr(), q.data_ptr(), scale.data_ptr(),
                                           S, N, K, _stream_ptr()), "bf_fp8_rows_quantize")
    return q, scale


def dequantize_rows_fp8(q: Tensor, scale: Tensor, center: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """W^ = bf16(fp32(q * scale + center)) [S, N, K] (bf_fp8_rows_dequantize): the weights every layer of a
    keep_weights="fp8" block multiplies by, written out for the GEMMs that read 16-bit weights."""
    S, N, K = q.shape
    out = torch.empty((S, N, K), dtype=torch.bfloat16, device=q.device) if out is None else out
    _fp8_rows_check("dequantize_rows_fp8", S, N, K, w=out, center=center, q=q, scale=scale)
    _C.check(_C.lib().bf_fp8_rows_dequantize(q.data_ptr(), scale.data_ptr(), center.data_ptr(), out.data_ptr(),
                                             _C.BF_DT_BF16, S, N, K, _stream_ptr()), "bf_fp8_rows_dequantize")
    return out


def skinny_fp8_supported(x: Tensor, q: Tensor, center: Tensor, S: int, K: int) -> bool:
    """Does skinny_linear_forward_fp8 take x ([S*M, K]) with these quantised rows?  skinny_supported's conditions at bf16."""
    if x.dtype != torch.bfloat16 or center.dtype != torch.bfloat16 or K % 32 or S > 65535:
        return False
    rows = x.shape[0]
    if rows % S or not 1 <= rows // S <= min(SKINNY_ROWS, _C.lib().bf_gemm_nt_skinny_max_rows()):
        return False
    return x.is_contiguous() and (x.data_ptr() | q.data_ptr() | center.data_ptr()) % 16 == 0


def skinny_linear_forward_fp8(x: Tensor, q: Tensor, scale: Tensor, center: Tensor, b_s: Optional[Tensor], S: int, N: int,
                              K: int, act: int = 0, x_sample_stride: Optional[int] = None,
                              out: Optional[Tensor] = None) -> Tensor:
    """y[s] = act(x[s] W^_s^T + b_s) for a few rows per sample on centred FP8 rows (bf_gemm_nt_skinny_fp8): x [S*M, K] bf16
    (or any storage with `x_sample_stride` elements between samples), q [S, N, K] uint8, scale [S, N] fp32, center [N, K]
    bf16, b_s [S, N] fp32 or None; returns [S*M, N] bf16.  The split-K scratch comes from the stream's workspace."""
    _require_device(x, "input")
    lib = _C.lib()
    if x.dtype not in _TORCH2BF:
        raise _C.BayeFormersAMDError(f"unsupported input dtype {x.dtype}")
    if x_sample_stride is None:
        if not x.is_contiguous():
            x = x.contiguous()
        rows = x.numel() // K
        if rows % S:
            raise _C.BayeFormersAMDError(f"input rows ({rows}) are not a multiple of the sample count S={S}")
        M = rows // S
        x_sample_stride = M * K
    else:
        M = x.shape[-2]
    y = out if out is not None else torch.empty((S * M, N), dtype=x.dtype, device=x.device)
    need = lib.bf_gemm_nt_skinny_fp8_workspace_bytes(S, M, N, K)
    ws = workspace(x.device, need) if need else None
    _C.check(lib.bf_gemm_nt_skinny_fp8(x.data_ptr(), _TORCH2BF[x.dtype], int(x_sample_stride), q.data_ptr(), scale.data_ptr(),
                                       center.data_ptr(), b_s.data_ptr() if b_s is not None else None, y.data_ptr(),
                                       _TORCH2BF[y.dtype], S, M, N, K, int(act),
                                       ws.data_ptr() if ws is not None else None, ws.numel() if ws is not None else 0,
                                       _stream_ptr()), "bf_gemm_nt_skinny_fp8")
    SKINNY_FP8_CALLS[0] += 1
    return y


# launches of the row-subset entries from this process (tests, diagnostics): bf_gemm_nt_rows, bf_attention_fwd_rows,
# bf_add_layernorm_rows — what the last encoder layer under a pooled head runs (bayeformers_amd._pooled_last_layer_forward)
ROWS_CALLS = {"gemm": 0, "attention": 0, "layernorm": 0}


def gemm_nt_rows(x: Tensor, w_s: Tensor, b_s: Optional[Tensor], S: int, M: int, N: int, K: int, x_sample_stride: int,
                 x_row_stride: int, act: int = 0, out: Optional[Tensor] = None) -> Tensor:
    """y[s] = act(x[s] W_s^T + b_s) for M rows per sample that lie `x_row_stride` elements apart (bf_gemm_nt_rows): row m
    of sample s starts at x.data_ptr() + (s * x_sample_stride + m * x_row_stride) elements — the [CLS] rows of a
    [S*B, L, K] activation at x_row_stride = L*K, read where they are.  w_s: [S, N, K] 16-bit, b_s: [S, N] fp32 or None;
    returns the compact [S*M, N] of x's dtype.  A tiled-GEMM launch for bf_profile_*; the split-K scratch comes from the
    stream's workspace."""
    _require_device(x, "input")
    lib = _C.lib()
    y = out if out is not None else torch.empty((S * M, N), dtype=x.dtype, device=x.device)
    need = lib.bf_gemm_nt_rows_workspace_bytes(_TORCH2BF[w_s.dtype], S, M, N, K)
    ws = workspace(x.device, need) if need else None
    _C.check(lib.bf_gemm_nt_rows(x.data_ptr(), _TORCH2BF[x.dtype], int(x_sample_stride), int(x_row_stride), w_s.data_ptr(),
                                 _TORCH2BF[w_s.dtype], b_s.data_ptr() if b_s is not None else None, y.data_ptr(),
                                 _TORCH2BF[y.dtype], S, M, N, K, int(act), ws.data_ptr() if ws is not None else None,
                                 ws.numel() if ws is not None else 0, _stream_ptr()), "bf_gemm_nt_rows")
    ROWS_CALLS["gemm"] += 1
    return y


COLSUMS_FOLDED = [0]  # bias gradients whose column sums came with the output gradient (tests, diagnostics)

# Column sums a gradient's PRODUCER left for its consumer (attention_backward -> linear_backward of query / key / value).
# Between the two the gradient passes through autograd — as the same tensor object or as views of it (HF's head split /
# merge) — so the hand-over is keyed by where the gradient lives: (storage address, byte offset, elements), valid while that
# very storage is alive AND unmodified: autograd's engine may add a second gradient into the producer's tensor IN PLACE
# (an output with two consumers); that moves the version counter every view of the storage shares, and the offer is void.
# An offer is taken once; a new bnn.Model forward drops what nobody took.
_COLSUM_OFFERS = {}


def _offer_key(t: Tensor):
    return (t.untyped_storage().data_ptr(), t.storage_offset() * t.element_size(), t.numel(), t.dtype)


def offer_colsum(grad: Tensor, colsum: Tensor) -> None:
    """`colsum` [S, N] fp32 = per-sample column sums of the contiguous gradient `grad` ([S*M, N] rows), as stored."""
    from torch.multiprocessing.reductions import StorageWeakRef

    if len(_COLSUM_OFFERS) > 64:
        _COLSUM_OFFERS.clear()
    _COLSUM_OFFERS[_offer_key(grad)] = (StorageWeakRef(grad.untyped_storage()), colsum, grad._version)


def take_colsum(grad: Tensor, S: int, N: int) -> Optional[Tensor]:
    if not _COLSUM_OFFERS or not grad.is_contiguous():
        return None
    hit = _COLSUM_OFFERS.pop(_offer_key(grad), None)
    if hit is None:
        return None
    ref, colsum, version = hit
    if ref.expired() or grad._version != version or tuple(colsum.shape) != (S, N) or colsum.device != grad.device:
        return None  # the storage the offer described is gone (its address may have been reused) or shapes do not match
    return colsum


def linear_backward(layer, x: Tensor, grad_y: Tensor, S: int, seed: int, sample_base: int, cdt: torch.dtype,
                    need_x: bool, need_mu_w: bool, need_mu_b: bool, w_samples: Optional[Tensor] = None,
                    act: int = 0, act_pre: Optional[Tensor] = None, dy_colsum: Optional[Tensor] = None):
    """Gradients of the sampled-weight linear layer (bf_linear_bwd).  Returns (dx, dmu_w, drho_w, dmu_b, drho_b);
    entries that are not needed are None.  x: [S*M, K] as saved by the forward; grad_y: [S*M, N].
    act / act_pre: the forward fused act() into its GEMM and kept the pre-activation [S*M, N]: grad_y is the gradient
    of act(y)."""
    from .nn.parameters.base import NoneParameter

    K, N = layer.in_features, layer.out_features
    M = x.shape[0] // S
    has_bias = not isinstance(layer.bias, NoneParameter)
    if dy_colsum is None and has_bias and not act:
        # the kernel that produced grad_y may have left its per-sample column sums with it (attention_backward): valid for
        # exactly this tensor, as it is (same dtype: no rounding in between)
        cs = take_colsum(grad_y, S, N) if (grad_y.dtype == cdt and grad_y.numel() == S * M * N) else None
        if cs is not None:
            dy_colsum = cs
            COLSUMS_FOLDED[0] += 1
    xg = (x if x.dtype == cdt else x.to(cdt)).contiguous()
    dy = grad_y.reshape(S * M, N)
    dy = (dy if dy.dtype == cdt else dy.to(cdt)).contiguous()
    dev = x.device
    w, b = _C.bf_tensor_t(), _C.bf_tensor_t()
    fill_tensor(w, layer.weight, NoneParameter(), 2 * layer.layer_id)
    if w_samples is not None and w_samples.dtype == cdt:
        # the forward's W_s are still resident (sampling plan): read instead of regenerated
        w.d_sample_out, w.out_dtype = w_samples.data_ptr(), _TORCH2BF[cdt]
    if has_bias:
        fill_tensor(b, layer.bias, NoneParameter(), 2 * layer.layer_id + 1)
    dx = torch.empty((S * M, K), dtype=cdt, device=dev) if need_x else None
    # A parameter whose gradient has a standing destination — its slot in a flat all-reduce bucket
    # (training.GradientBuckets, between zero() and finish()) — gets the kernel's result written there: no copy into the
    # bucket afterwards, and autograd is handed None for it (the slot IS the accumulated gradient).
    sunk = []

    def dest(param, shape, needed=True):
        if not needed:
            return None
        sink = getattr(param, "_bf_grad_sink", None)
        slot = sink.slot(param) if sink is not None else None
        if slot is not None and slot.dtype == torch.float32 and slot.shape == shape and slot.device == dev:
            sunk.append((sink, param))
            return slot
        return torch.empty(shape, dtype=torch.float32, device=dev)

    # A layer whose weight reduction is DEFERRED (training.DeferredParamGrads, armed for this step): bf_linear_bwd leaves the
    # per-sample gradients dW_s in the manager's buffer and skips the reduction; ONE bf_param_grad_table launch after the
    # backward pass reduces every such layer into the manager's gradient buffers.  Autograd is handed None for mu / rho.
    defer = getattr(layer, "_bf_pg_defer", None)
    dw_keep = defer.keep_buffer(layer, S, M, cdt, seed, sample_base) if defer is not None else None
    db_keep = None
    if dw_keep is not None:
        dmu_w = drho_w = None
        db_keep = defer.keep_bias_buffer(layer, dy_colsum if not act else None) if has_bias else None
    else:
        dmu_w = dest(layer.weight.mu, (N, K), need_mu_w)
        drho_w = dest(layer.weight.rho, (N, K))
    if db_keep is not None:
        dmu_b = drho_b = None
    else:
        dmu_b = dest(layer.bias.mu, (N,), has_bias and need_mu_b) if has_bias else None
        drho_b = dest(layer.bias.rho, (N,)) if has_bias else None
    lib = _C.lib()
    if act:
        if act_pre is None or act_pre.dtype != cdt or act_pre.numel() != S * M * N:
            raise _C.BayeFormersAMDError("linear_backward: a fused activation needs the forward's pre-activation "
                                         f"as a [{S * M}, {N}] {cdt} tensor")
        act_pre = act_pre.contiguous()
    need = lib.bf_linear_bwd_workspace_bytes(S, M, N, K, int(has_bias), _TORCH2BF[cdt], act)
    ws = workspace(dev, need)
    ptr = lambda t: t.data_ptr() if t is not None else None
    if dw_keep is not None:
        drho_keep = defer.grad_view(layer.weight.rho)  # (where the table launch will write; nothing is written there now)
    _C.check(lib.bf_linear_bwd(xg.data_ptr(), M * K, dy.data_ptr(), _TORCH2BF[cdt], ctypes.byref(w),
                               ctypes.byref(b) if has_bias else None, ptr(dx), ptr(dmu_w),
                               ptr(drho_w) if dw_keep is None else drho_keep.data_ptr(), ptr(dmu_b),
                               ptr(drho_b) if db_keep is None else defer.grad_view(layer.bias.rho).data_ptr(), S, M, N, K, seed,
                               sample_base & 0xFFFFFFFF, act, ptr(act_pre) if act else None,
                               ptr(dy_colsum), ptr(dw_keep), ptr(db_keep), ws.data_ptr(), ws.numel(), _stream_ptr()), "bf_linear_bwd")
    if dx is not None and dx.dtype != x.dtype:
        dx = dx.to(x.dtype)
    if sunk:
        gone = {id(p) for _, p in sunk}
        for sink, param in sunk:
            sink.arrived(param)
        if has_bias:
            dmu_b = None if (dmu_b is not None and id(layer.bias.mu) in gone) else dmu_b
            drho_b = None if id(layer.bias.rho) in gone else drho_b
        dmu_w = None if (dmu_w is not None and id(layer.weight.mu) in gone) else dmu_w
        drho_w = None if id(layer.weight.rho) in gone else drho_w
    return dx, dmu_w, drho_w, dmu_b, drho_b


def kl_grad(gaussian, prior, stream_id: int, S: int, seed: int, sample_base: int, g: Tensor, need_mu: bool):
    """Gradient of sum_s g[s,0]*log_prior_s + g[s,1]*log_q_s w.r.t. one Gaussian's (mu, rho) (bf_kl_grad)."""
    t = _C.bf_tensor_t()
    if not fill_tensor(t, gaussian, prior, stream_id):
        raise _C.BayeFormersAMDError("kl_grad: user-defined priors have no kernel gradient")
    dev = gaussian.mu.device
    dmu = torch.empty_like(gaussian.mu, dtype=torch.float32) if need_mu else None
    drho = torch.empty_like(gaussian.rho, dtype=torch.float32)
    _C.check(_C.lib().bf_kl_grad(ctypes.byref(t), S, seed, sample_base & 0xFFFFFFFF, g.data_ptr(),
                                 dmu.data_ptr() if dmu is not None else None, drho.data_ptr(), _stream_ptr()),
             "bf_kl_grad")
    return dmu, drho


def embedding_forward(ids: Tensor, mu: Tensor, rho: Tensor, out_dtype: torch.dtype, S: int, seed: int,
                      sample_base: int, stream_id: int) -> Tensor:
    """Rows ids of S table draws W_s = mu + softplus(rho)*eps_s (bf_embedding_fwd); ids is [S*T] sample-major."""
    _require_device(mu, "Embedding.weight.mu")
    _require_device(ids, "Embedding input")
    V, D = mu.shape
    n = ids.numel()
    if n % S:
        raise _C.BayeFormersAMDError(f"embedding_forward: {n} tokens are not a multiple of S={S}")
    out = torch.empty((n, D), dtype=out_dtype, device=mu.device)
    if n:
        _C.check(_C.lib().bf_embedding_fwd(ids.data_ptr(), mu.data_ptr(), rho.data_ptr(), out.data_ptr(),
                                           _TORCH2BF[out_dtype], n, n // S, V, D, seed, sample_base & 0xFFFFFFFF,
                                           stream_id, _stream_ptr()), "bf_embedding_fwd")
    return out


def embedding_backward(ids: Tensor, grad: Tensor, mu: Tensor, rho: Tensor, S: int, seed: int, sample_base: int,
                       stream_id: int, need_mu: bool, need_rho: bool):
    """Scatter-add of the output gradient into (dmu, drho) of the table (bf_embedding_bwd)."""
    V, D = mu.shape
    n = ids.numel()
    grad = grad.contiguous()
    dmu = torch.zeros_like(mu, dtype=torch.float32) if need_mu else None
    drho = torch.zeros_like(rho, dtype=torch.float32) if need_rho else None
    if n and (need_mu or need_rho):
        _C.check(_C.lib().bf_embedding_bwd(ids.data_ptr(), grad.data_ptr(), _TORCH2BF[grad.dtype], rho.data_ptr(),
                                           dmu.data_ptr() if need_mu else None, drho.data_ptr() if need_rho else None,
                                           n, n // S, V, D, seed, sample_base & 0xFFFFFFFF, stream_id, _stream_ptr()),
                 "bf_embedding_bwd")
    return dmu, drho


class Dropout:
    """One dropout of the training-mode forward, as the kernels take it (the dropout contract of csrc/bf_philox.h):
    rate p, the Philox seed, `call` = the number of the forward it belongs to (reserved with the forward's sample indices, so
    a backward pass and the recomputation of a checkpointed block find the same mask) and `site` = the module.
    `origin` = (first global sample of this process's shard, samples in the shard): the kernels number their groups from
    first_sample x (groups per sample), so a sample's masks do not depend on which rank runs it (random.dropout_origin).
    `counter`: device-counter mode (random.use_device_counter) — a 1-element int32 device tensor, the forward's copy of the
    device-resident call counter, which the kernels add to `call` (then 0): forward, backward and a recomputed block read
    the same copy, and a step replayed from a HIP graph draws fresh masks every replay (random.dropout_counter)."""
    __slots__ = ("p", "seed", "call", "site", "origin", "counter")

    def __init__(self, p: float, seed: int, call: int, site: int, origin=(0, 1), counter=None):
        self.p, self.seed, self.call, self.site = float(p), int(seed), int(call) & 0xFFFFFFFF, int(site) & 0x7FFFFFFF
        self.origin = (int(origin[0]), max(1, int(origin[1])))
        self.counter = counter

    @property
    def d_call(self):
        return self.counter.data_ptr() if self.counter is not None else None

    def first_group(self, units: int, groups_per_unit: int) -> int:
        """Global index of the first group of a tensor made of `units` rows (or sequences) of `groups_per_unit` groups each,
        the units being this shard's samples in equal slabs."""
        start, s_local = self.origin
        if start == 0:
            return 0
        if units % s_local:
            # a shard that does not start at sample 0 must know how many units one sample has: numbering its groups from 0
            # instead would draw the masks of global samples 0.. — correlated across ranks, and silently
            raise _C.BayeFormersAMDError(
                f"dropout: a tensor of {units} rows / sequences cannot be split into this shard's {s_local} Monte-Carlo samples "
                f"(first global sample {start}); the dropped tensor must hold the samples in equal, sample-major slabs")
        return start * (units // s_local) * int(groups_per_unit)

    @property
    def keep_scale(self) -> float:
        thresh = min(65535, int(self.p * 65536.0 + 0.5))
        return 1.0 / (1.0 - thresh / 65536.0)


def dropout_keep_host(first_group: int, n_groups: int, d: "Dropout") -> Tensor:
    """Host twin of the kernels' keep decisions (bf_dropout_keep_host): uint8 [n_groups, 8], 1 = kept."""
    out = torch.empty((int(n_groups), 8), dtype=torch.uint8)
    _C.check(_C.lib().bf_dropout_keep_host(out.data_ptr(), int(first_group), int(n_groups), d.p, d.seed, d.call, d.site),
             "bf_dropout_keep_host")
    return out


def add_layernorm(x: Tensor, residual: Optional[Tensor], gamma: Tensor, beta: Tensor, eps: float,
                  drop: Optional[Dropout] = None) -> Tensor:
    """LayerNorm(x + residual) over the last axis in one pass (bf_add_layernorm); residual may be None.
    drop: LayerNorm(dropout(x) + residual) (bf_add_layernorm_dropout)."""
    _require_device(x, "add_layernorm input")
    N = x.shape[-1]
    x2 = x.reshape(-1, N)
    x2 = x2 if x2.is_contiguous() else x2.contiguous()
    r2 = None
    if residual is not None:
        if residual.shape != x.shape or residual.dtype != x.dtype:
            raise _C.BayeFormersAMDError("add_layernorm: residual must match the input's shape and dtype")
        r2 = residual.reshape(-1, N)
        r2 = r2 if r2.is_contiguous() else r2.contiguous()
    if gamma.dtype != beta.dtype or gamma.dtype not in (torch.float32, x.dtype):
        raise _C.BayeFormersAMDError("add_layernorm: gamma/beta must be float32 or have the input's dtype")
    out = torch.empty_like(x2)
    if drop is not None and drop.p > 0.0:
        _C.check(_C.lib().bf_add_layernorm_dropout(x2.data_ptr(), r2.data_ptr() if r2 is not None else None, gamma.data_ptr(),
                                                   beta.data_ptr(), _TORCH2BF[gamma.dtype], out.data_ptr(),
                                                   _TORCH2BF[x.dtype], x2.shape[0], N, float(eps), drop.p, drop.seed,
                                                   drop.call, drop.site, drop.first_group(x2.shape[0], N // 8), drop.d_call,
                                                   _stream_ptr()),
                 "bf_add_layernorm_dropout")
        return out.view(x.shape)
    _C.check(_C.lib().bf_add_layernorm(x2.data_ptr(), r2.data_ptr() if r2 is not None else None, gamma.data_ptr(),
                                       beta.data_ptr(), _TORCH2BF[gamma.dtype], out.data_ptr(), _TORCH2BF[x.dtype],
                                       x2.shape[0], N, float(eps), _stream_ptr()), "bf_add_layernorm")
    return out.view(x.shape)


def add_layernorm_rows(x: Tensor, residual: Tensor, residual_row_stride: int, gamma: Tensor, beta: Tensor,
                       eps: float) -> Tensor:
    """LayerNorm(x + residual) with residual rows `residual_row_stride` elements apart (bf_add_layernorm_rows): x is the
    compact [rows, N], row r of the residual starts at residual.data_ptr() + r * residual_row_stride elements.  Returns the
    compact [rows, N]; per row the arithmetic of add_layernorm."""
    _require_device(x, "add_layernorm_rows input")
    rows, N = x.shape
    if not x.is_contiguous() or residual.dtype != x.dtype:
        raise _C.BayeFormersAMDError("add_layernorm_rows: x must be contiguous [rows, N] and the residual of its dtype")
    if gamma.dtype != beta.dtype or gamma.dtype not in (torch.float32, x.dtype):
        raise _C.BayeFormersAMDError("add_layernorm_rows: gamma/beta must be float32 or have the input's dtype")
    out = torch.empty_like(x)
    _C.check(_C.lib().bf_add_layernorm_rows(x.data_ptr(), residual.data_ptr(), int(residual_row_stride), gamma.data_ptr(),
                                            beta.data_ptr(), _TORCH2BF[gamma.dtype], out.data_ptr(), _TORCH2BF[x.dtype],
                                            rows, N, float(eps), _stream_ptr()), "bf_add_layernorm_rows")
    ROWS_CALLS["layernorm"] += 1
    return out


def embed_layernorm(ids: Tensor, type_ids: Optional[Tensor], pos_ids: Optional[Tensor], word: Tensor, type_table: Tensor,
                    pos_table: Tensor, gamma: Tensor, beta: Tensor, eps: float) -> Tensor:
    """LayerNorm(word[ids] + type[type_ids or 0] + pos[pos_ids or position in sequence]) in one pass
    (bf_embed_layernorm).  ids: [B, L] int64; type_ids: [B, L] or None; pos_ids: [1 or B, L] or None; returns [B, L, N].
    An id outside its table gives a NaN output row (no out-of-bounds read)."""
    _require_device(ids, "embed_layernorm ids")
    B, L = ids.shape
    N = word.shape[1]
    ids = ids.contiguous()
    if type_ids is not None:
        type_ids = type_ids.expand(B, L).contiguous()
    pos_rows = 0
    if pos_ids is not None:
        pos_ids = pos_ids.contiguous()
        pos_rows = pos_ids.numel()  # [1, L]: r % L; [B, L]: r
    out = torch.empty((B, L, N), dtype=word.dtype, device=word.device)
    ptr = lambda t: t.data_ptr() if t is not None else None
    _C.check(_C.lib().bf_embed_layernorm(ids.data_ptr(), ptr(type_ids), ptr(pos_ids), word.data_ptr(), type_table.data_ptr(),
                                         pos_table.data_ptr(), gamma.data_ptr(), beta.data_ptr(), _TORCH2BF[gamma.dtype],
                                         out.data_ptr(), _TORCH2BF[word.dtype], B * L, N, L, pos_rows, word.shape[0],
                                         type_table.shape[0], pos_table.shape[0], float(eps),
                                         _stream_ptr()), "bf_embed_layernorm")
    return out


def attention_supported(q: Tensor, k: Tensor, v: Tensor, causal: bool = False, kv_heads: Optional[int] = None) -> bool:
    """q, k, v as the attention hook gets them: [B, H, T, 64] views of the projections' [B*T, H*64] outputs
    (bf_attention_fwd).  With causal=True or kv_heads given: what bf_attention_fwd_gqa takes instead — q [B, H, T, D],
    k and v [B, Hkv, T, D] with Hkv (= kv_heads) dividing H, D 64, 128 or 256, any T >= 1, each with its own
    (batch, head, token) strides and a contiguous feature dimension."""
    if not (q.is_cuda and q.dtype in (torch.bfloat16, torch.float16) and k.dtype == q.dtype and v.dtype == q.dtype):
        return False
    if causal or kv_heads is not None:
        return _gqa_supported(q, k, v, kv_heads)
    if q.dim() != 4 or q.shape != k.shape or q.shape != v.shape:
        return False
    B, H, T, D = q.shape
    if D != 64 or T < 128 or T % 128 or B > 65535 or H > 65535:
        return False
    st = (T * H * D, D, H * D, 1)  # BHTD view of a contiguous [B, T, H, D] tensor
    return all(t.stride() == st and t.data_ptr() % 16 == 0 for t in (q, k, v))


def _gqa_supported(q: Tensor, k: Tensor, v: Tensor, kv_heads: Optional[int]) -> bool:
    if q.dim() != 4 or k.dim() != 4 or k.shape != v.shape:
        return False
    B, H, T, D = q.shape
    Hkv = k.shape[1] if kv_heads is None else int(kv_heads)
    if tuple(k.shape) != (B, Hkv, T, D) or Hkv < 1 or H % Hkv:
        return False
    if D not in (64, 128, 256) or T < 1 or B > 65535 or H > 65535:  # (any length: T % 128 != 0 runs the kernels' tail forms)
        return False
    return all(t.stride(3) == 1 and all(s >= 0 and s % 8 == 0 for s in t.stride()[:3]) and t.data_ptr() % 16 == 0
               for t in (q, k, v))


# launches of bf_attention_fwd_gqa / bf_attention_bwd_gqa from this process (a test can assert that the causal path ran);
# "fwd_window" / "bwd_window": of their sliding-window siblings bf_attention_fwd_gqa_window / bf_attention_bwd_gqa_window
GQA_CALLS = {"fwd": 0, "bwd": 0, "fwd_window": 0, "bwd_window": 0}
# launches of the soft-cap entries (bf_attention_fwd_gqa_softcap / bf_attention_bwd_gqa_softcap /
# bf_attention_decode_gqa_softcap without and with a kv_len), with or without a window; they count here alone
SOFTCAP_CALLS = {"fwd": 0, "bwd": 0, "decode": 0, "decode_len": 0}


def _gqa_shape(q: Tensor, k: Tensor, v: Tensor, causal: bool):
    B, H, T, D = q.shape
    s = _C.bf_attn_gqa_t(B, T, H, k.shape[1], D, int(bool(causal)))
    for name, t in (("q_stride", q), ("k_stride", k), ("v_stride", v)):
        getattr(s, name)[:] = [t.stride(0), t.stride(1), t.stride(2)]
    return s


def attention_forward_gqa(q: Tensor, k: Tensor, v: Tensor, key_mask: Optional[Tensor], scaling: float, causal: bool = True,
                          mask_off: Optional[Tensor] = None, want_lse: bool = False, window: Optional[int] = None,
                          softcap: Optional[float] = None):
    """Causal and / or grouped-query attention (bf_attention_fwd_gqa): q [B, H, T, D], k / v [B, Hkv, T, D] as described by
    attention_supported(..., causal=True); key_mask: additive fp32 [B, T] or None.  Returns [B, T, H, D] contiguous (a
    query with no visible key gives 0) — and, with want_lse, the [B, H, T] fp32 log-sum-exp rows of the backward.
    window: a sliding window of that many keys (bf_attention_fwd_gqa_window; causal only): query i sees keys
    i - window + 1 .. i.
    softcap: the logits become softcap * tanh(scaling q.k / softcap) before the mask (bf_attention_fwd_gqa_softcap, with
    or without a window; causal only); None is the call without it."""
    B, H, T, D = q.shape
    out = torch.empty((B, T, H, D), dtype=q.dtype, device=q.device)
    lse = torch.empty((B, H, T), dtype=torch.float32, device=q.device) if want_lse else None
    shape = _gqa_shape(q, k, v, causal)
    args = (q.data_ptr(), k.data_ptr(), v.data_ptr(), key_mask.data_ptr() if key_mask is not None else None,
            mask_off.data_ptr() if mask_off is not None else None, out.data_ptr(),
            lse.data_ptr() if lse is not None else None, _TORCH2BF[q.dtype], ctypes.byref(shape))
    if softcap is not None:
        _C.check(_C.lib().bf_attention_fwd_gqa_softcap(*args, int(window or 0), float(softcap), float(scaling),
                                                       _stream_ptr()), "bf_attention_fwd_gqa_softcap")
        SOFTCAP_CALLS["fwd"] += 1
    elif window is None:
        _C.check(_C.lib().bf_attention_fwd_gqa(*args, float(scaling), _stream_ptr()), "bf_attention_fwd_gqa")
        GQA_CALLS["fwd"] += 1
    else:
        _C.check(_C.lib().bf_attention_fwd_gqa_window(*args, int(window), float(scaling), _stream_ptr()),
                 "bf_attention_fwd_gqa_window")
        GQA_CALLS["fwd_window"] += 1
    return (out, lse) if want_lse else out


def attention_backward_gqa(q: Tensor, k: Tensor, v: Tensor, key_mask: Optional[Tensor], mask_off: Optional[Tensor],
                           out: Tensor, grad_out: Tensor, lse: Tensor, scaling: float, causal: bool = True,
                           window: Optional[int] = None, softcap: Optional[float] = None):
    """Gradients of attention_forward_gqa (bf_attention_bwd_gqa, bf_attention_bwd_gqa_window with a window, or
    bf_attention_bwd_gqa_softcap with a softcap: `lse` is then the capped forward's):
    (dq [B, T, H, D], dk [B, T, Hkv, D], dv [B, T, Hkv, D]), contiguous; dk / dv summed over the query heads of each
    group."""
    B, H, T, D = q.shape
    Hkv = k.shape[1]
    go = grad_out if (grad_out.dtype == q.dtype and grad_out.is_contiguous()) else grad_out.to(q.dtype).contiguous()
    dq = torch.empty((B, T, H, D), dtype=q.dtype, device=q.device)
    dkv = torch.empty((2, B, T, Hkv, D), dtype=q.dtype, device=q.device)
    delta = torch.empty((B, H, T), dtype=torch.float32, device=q.device)
    shape = _gqa_shape(q, k, v, causal)
    args = (q.data_ptr(), k.data_ptr(), v.data_ptr(), key_mask.data_ptr() if key_mask is not None else None,
            mask_off.data_ptr() if mask_off is not None else None, out.data_ptr(), go.data_ptr(), lse.data_ptr(),
            delta.data_ptr(), dq.data_ptr(), dkv[0].data_ptr(), dkv[1].data_ptr(), _TORCH2BF[q.dtype], ctypes.byref(shape))
    if softcap is not None:
        _C.check(_C.lib().bf_attention_bwd_gqa_softcap(*args, int(window or 0), float(softcap), float(scaling),
                                                       _stream_ptr()), "bf_attention_bwd_gqa_softcap")
        SOFTCAP_CALLS["bwd"] += 1
    elif window is None:
        _C.check(_C.lib().bf_attention_bwd_gqa(*args, float(scaling), _stream_ptr()), "bf_attention_bwd_gqa")
        GQA_CALLS["bwd"] += 1
    else:
        _C.check(_C.lib().bf_attention_bwd_gqa_window(*args, int(window), float(scaling), _stream_ptr()),
                 "bf_attention_bwd_gqa_window")
        GQA_CALLS["bwd_window"] += 1
    return dq, dkv[0], dkv[1]


# launches of the band entries (bf_attention_fwd_gqa_band / bf_attention_bwd_gqa_band: packed sequences); they count here
# alone
PACKED_CALLS = {"fwd": 0, "bwd": 0}


def band_bounds(doc_ids: Tensor, window: Optional[int] = None):
    """The bounds of banded causal attention (include/bayeformers_amd_packed.h) for packed documents: doc_ids [B, T] (or
    [T]) integers, non-decreasing along T, equal within a document (transformers' find_packed_sequence_indices).  Returns
    (lo, hi), int32 of doc_ids' shape on its device, without a host synchronisation: query i sees the keys lo[i] .. i and
    key j is seen by the queries j .. hi[j], where lo[i] = max(doc_start(i), i - window + 1) and
    hi[j] = min(doc_end(j), j + window - 1) (window None: the documents alone)."""
    if window is not None and window < 1:
        raise ValueError(f"band_bounds: window={window} must be at least 1")
    ids = doc_ids.contiguous()
    pos = torch.arange(ids.shape[-1], device=ids.device)
    lo = torch.searchsorted(ids, ids, right=False)     # the first token of each token's document
    hi = torch.searchsorted(ids, ids, right=True) - 1  # ... and the last
    if window is not None:
        lo = torch.maximum(lo, pos - (window - 1))
        hi = torch.minimum(hi, pos + (window - 1))
    return lo.to(torch.int32), hi.to(torch.int32)


def attention_forward_gqa_band(q: Tensor, k: Tensor, v: Tensor, lo: Tensor, scaling: float, want_lse: bool = False):
    """Banded causal grouped-query attention (bf_attention_fwd_gqa_band): q, k, v as attention_forward_gqa takes them, lo
    [B, T] int32 as band_bounds returns it — query i sees the keys lo[b, i] .. i; no key mask.  Returns [B, T, H, D]
    contiguous and, with want_lse, the [B, H, T] fp32 log-sum-exp rows of the backward."""
    B, H, T, D = q.shape
    _check_bound(lo, "lo", B, T, q.device)
    out = torch.empty((B, T, H, D), dtype=q.dtype, device=q.device)
    lse = torch.empty((B, H, T), dtype=torch.float32, device=q.device) if want_lse else None
    shape = _gqa_shape(q, k, v, True)
    _C.check(_C.lib().bf_attention_fwd_gqa_band(q.data_ptr(), k.data_ptr(), v.data_ptr(), lo.data_ptr(), out.data_ptr(),
                                                lse.data_ptr() if lse is not None else None, _TORCH2BF[q.dtype],
                                                ctypes.byref(shape), float(scaling), _stream_ptr()),
             "bf_attention_fwd_gqa_band")
    PACKED_CALLS["fwd"] += 1
    return (out, lse) if want_lse else out


def attention_backward_gqa_band(q: Tensor, k: Tensor, v: Tensor, lo: Tensor, hi: Tensor, out: Tensor, grad_out: Tensor,
                                lse: Tensor, scaling: float):
    """Gradients of attention_forward_gqa_band (bf_attention_bwd_gqa_band; hi: band_bounds' second result):
    (dq [B, T, H, D], dk [B, T, Hkv, D], dv [B, T, Hkv, D]), contiguous, as attention_backward_gqa returns them."""
    B, H, T, D = q.shape
    Hkv = k.shape[1]
    _check_bound(lo, "lo", B, T, q.device)
    _check_bound(hi, "hi", B, T, q.device)
    go = grad_out if (grad_out.dtype == q.dtype and grad_out.is_contiguous()) else grad_out.to(q.dtype).contiguous()
    dq = torch.empty((B, T, H, D), dtype=q.dtype, device=q.device)
    dkv = torch.empty((2, B, T, Hkv, D), dtype=q.dtype, device=q.device)
    delta = torch.empty((B, H, T), dtype=torch.float32, device=q.device)
    shape = _gqa_shape(q, k, v, True)
    _C.check(_C.lib().bf_attention_bwd_gqa_band(q.data_ptr(), k.data_ptr(), v.data_ptr(), lo.data_ptr(), hi.data_ptr(),
                                                out.data_ptr(), go.data_ptr(), lse.data_ptr(), delta.data_ptr(),
                                                dq.data_ptr(), dkv[0].data_ptr(), dkv[1].data_ptr(), _TORCH2BF[q.dtype],
                                                ctypes.byref(shape), float(scaling), _stream_ptr()),
             "bf_attention_bwd_gqa_band")
    PACKED_CALLS["bwd"] += 1
    return dq, dkv[0], dkv[1]


def _check_bound(t: Tensor, name: str, B: int, T: int, device) -> None:
    if t.dtype != torch.int32 or tuple(t.shape) != (B, T) or not t.is_contiguous() or t.device != device:
        raise ValueError(f"band attention: {name} must be a contiguous int32 [{B}, {T}] tensor on {device}, got "
                         f"{t.dtype} {tuple(t.shape)} on {t.device}")


# launches of bf_attention_decode_gqa from this process (a test can assert that a cached decode step ran on the kernel);
# "len": of bf_attention_decode_gqa_len (a step against a fixed-capacity cache, attention_forward_decode_len);
# "window" / "len_window": of their sliding-window siblings
DECODE_CALLS = {"fwd": 0, "len": 0, "window": 0, "len_window": 0}
DECODE_MAX_QUERIES = 16


def _cached_layout_ok(q: Tensor, k: Tensor, v: Tensor, check_device: bool, fp8: bool, chunk: bool) -> bool:
    """The one layout test behind the four `*_supported` predicates of the cached entries: q [N, H, Tq, D], k and v
    [N, Hkv, Tk, D] with Hkv dividing H, D 64, 128 or 256, a contiguous feature dimension, 16-byte aligned, and (batch, head,
    token) strides that are non-negative multiples of 16 bytes — 8 elements of q and of a 16-bit cache (bf16 or fp16, one
    dtype), 16 of an e4m3 one (fp8: q bfloat16, k / v uint8).  chunk: any 1 <= Tq <= Tk; else a decode step, Tq at most
    DECODE_MAX_QUERIES.  check_device=False judges the shapes, dtypes and strides alone (CPU or meta tensors)."""
    if check_device and not (q.is_cuda and k.is_cuda and v.is_cuda):
        return False
    if fp8:
        if q.dtype != torch.bfloat16 or k.dtype != torch.uint8 or v.dtype != torch.uint8:
            return False
    elif q.dtype not in (torch.bfloat16, torch.float16) or k.dtype != q.dtype or v.dtype != q.dtype:
        return False
    if q.dim() != 4 or k.dim() != 4 or k.shape != v.shape:
        return False
    N, H, Tq, D = q.shape
    Hkv, Tk = k.shape[1], k.shape[2]
    if k.shape[0] != N or k.shape[3] != D or Hkv < 1 or H % Hkv or D not in KV8_HEAD_SIZES or not 1 <= Tq <= Tk:
        return False
    if (N > 65535 or H > 65535 or Tk >= 2 ** 31) if chunk else (Tq > DECODE_MAX_QUERIES or N * Hkv > 65535):  # the grids
        return False
    return all(t.stride(3) == 1 and all(st >= 0 and st % granule == 0 for st in t.stride()[:3]) and t.data_ptr() % 16 == 0
               for t, granule in ((q, 8), (k, 16 if fp8 else 8), (v, 16 if fp8 else 8)))


def attention_decode_supported(q: Tensor, k: Tensor, v: Tensor, check_device: bool = True) -> bool:
    """What bf_attention_decode_gqa takes: q [N, H, Tq, D] (1 <= Tq <= 16), k and v [N, Hkv, Tk, D] with Tq <= Tk, Hkv
    dividing H, D 64, 128 or 256, bf16 or fp16, each with its own (batch, head, token) strides (non-negative multiples of 8
    elements) and a contiguous feature dimension.  check_device=False judges the shapes, dtypes and strides alone (CPU or
    meta tensors)."""
    return _cached_layout_ok(q, k, v, check_device, fp8=False, chunk=False)


def decode_kernel_wins(H: int, Hkv: int, Tq: int, Tk: int, D: int) -> bool:
    """The dispatch rule of cached decode steps, from the measurement of profiles/decode_attention.md: every measured class
    runs faster on bf_attention_decode_gqa than on the framework's SDPA except one query per sequence on plain multi-head
    attention (one query row per workgroup of 64) with head size 128 and a short cache (Tk 512: 0.93x), which stays on SDPA.
    Head size 256 rests on profiles/head256_attention.md: every measured class (H / Hkv 8 / 4, 16 / 16 and 8 / 1, Tq 1 and 4,
    Tk 512 .. 32768) runs 1.12x .. 14x faster on the kernel — the smallest margin is that same class, multi-head, one query,
    Tk 512 (37 against 43 us, within SDPA's spread there) — so none of them is sent to SDPA."""
    return not (H == Hkv and Tq == 1 and D == 128 and Tk <= 512)


def prefill_kernel_wins(H: int, Hkv: int, T: int, D: int, backward: bool, window: Optional[int] = None,
                        masked: bool = False) -> bool:
    """The dispatch rule of cache-free causal calls (prefill, training), beside decode_kernel_wins: True = the kernels,
    False = the framework's SDPA as the fallback would call it.  `masked`: the call carries a mask, so the fallback would run
    SDPA over _padding_mask_interface's dense [B, 1, T, T] mask and not its is_causal form.  Head sizes 64 and 128 run the
    kernels everywhere (profiles/causal_attention.md, ragged_attention.md, sliding_window.md).  Head size 256 rests on
    profiles/head256_attention.md (bf16, B 4, H / Hkv 8 / 4, 16 / 16 and 8 / 1 at T 512, 2048, 8192, 8 / 4 also at 256,
    each with and without a padded row, against sdpa_attention_forward in one process; x = SDPA time / kernel time):
      * a sliding window shorter than T wins all six measured points (8 / 4 only; W 256 .. 4096, T 512 .. 8192: forward
        1.6x .. 4.8x, forward + backward 1.7x .. 10.9x); other head layouts are extrapolated from them;
      * forward + backward wins every class (1.19x .. 3.07x) but one: one K/V head, T 512, padded (0.70x), sent to SDPA;
      * the forward with a mask wins (1.07x .. 1.52x) except multi-head at T 512 (0.95x against spreads of 1.4 / 2.3 %),
        sent to SDPA;
      * the forward without a mask loses to SDPA's is_causal form by more than the spread in seven of ten classes
        (0.40x .. 0.86x) and ties it, inside the spread, in three (8 / 4 at T 256: 0.95x, 16 / 16 at 512: 1.00x, 8 / 1 at
        2048: 0.97x) whose neighbours in T on either side lose: the ties go with their neighbours, so the whole class is on
        SDPA and the rule stays monotone in T.
    T 512 verdicts hold up to 1024, the midpoint (in ratio) to the next measured length; nothing below 256 was timed.
    Packed rows (`_packed_attention`: masked=True, the fallback being SDPA over the dense document mask) follow the same
    rule.  profiles/packed_attention.md timed head size 256 for them at H / Hkv 8 / 4, T 2048 and 8192 (documents of 512,
    mixed, one document; with and without W 1024): every class wins (forward 1.37x .. 12.9x, forward + backward 2.64x ..
    29x, spreads under 5 %), so none is sent to SDPA on that account; the two masked classes above (T <= 1024) were not
    timed with documents and keep their padding-mask verdicts."""
    if D != 256 or (window is not None and window < T):
        return True
    if backward:
        return not (masked and Hkv == 1 and T <= 1024)
    if masked:
        return not (H == Hkv and T <= 1024)
    return False


def chunk_kernel_wins(H: int, Hkv: int, Tq: int, Tk: int, D: int, window: Optional[int] = None) -> bool:
    """The dispatch rule of cached chunks (more than 16 new queries against a cache, under `chunked_attention()`), beside
    prefill_kernel_wins: True = bf_attention_chunk_gqa, False = the framework's SDPA over the dense [N, 1, Tq, Tk] mask.
    From profiles/chunked_prefill.md (bf16, N 8, H / Hkv 16 / 4, Tq 512 and 2048 against L 4096 and 16384 cached keys, with
    and without W 1024, both in one process; x = SDPA time / kernel time):
      * head sizes 64 and 128 win every class: 2.1x .. 2.8x without a window, 5.2x .. 28x with one;
      * head size 256 (one wave per SIMD, 64-key tiles) with a window wins 3.4x .. 16.1x; without one it wins at L 4096
        (1.11x at Tq 512 inside the kernel's 19 % spread there, 1.63x at Tq 2048) and at L 16384 loses at Tq 512 (0.79x) and
        ties at Tq 2048 (1.01x, spreads under 1.5 %): the tie goes with its neighbour, so head size 256 without a window goes
        to SDPA from 8192 keys on, the midpoint (in ratio) of the two measured lengths.
    The crossover itself was NOT measured: nothing between 4096 and 16384 keys was timed.
    Tk is what the fallback would read: the capacity of a fixed-capacity cache.  The soft-cap and FP8-cache callers do not
    consult it (the framework's attention does not compute the cap, and nothing else reads the FP8 rows)."""
    if D != 256 or (window is not None and window < Tk):
        return True
    return Tk < 8192


def _decode_shape(q: Tensor, k: Tensor, v: Tensor):
    N, H, Tq, D = q.shape
    s = _C.bf_attn_decode_t(N, Tq, k.shape[2], H, k.shape[1], D)
    for name, t in (("q_stride", q), ("k_stride", k), ("v_stride", v)):
        getattr(s, name)[:] = [t.stride(0), t.stride(1), t.stride(2)]
    return s


def attention_decode_workspace_bytes(q: Tensor, k: Tensor, v: Tensor) -> int:
    """Scratch bytes attention_forward_decode needs at this shape (bf_attention_decode_workspace_bytes)."""
    n = int(_C.lib().bf_attention_decode_workspace_bytes(ctypes.byref(_decode_shape(q, k, v))))
    if n < 0:
        _C.check(1, "bf_attention_decode_workspace_bytes")
    return n


def _cached_call(name: str, q: Tensor, k: Tensor, v: Tensor, scales, kv_len: Optional[Tensor], key_mask: Optional[Tensor],
                 workspace: Optional[Tensor] = None, decode: bool = True, Tk: Optional[int] = None):
    """What the decode, ring and chunk wrappers check and allocate alike, 16-bit and FP8; `name` is the caller's, for the
    messages.  q [N, H, Tq, D] against k / v [N, Hkv, rows, D] on one ROCm device with contiguous feature dimensions — one
    16-bit dtype, or with `scales` = (k_scale, v_scale) q bfloat16 and the four tensors of an FP8 cache; kv_len None or one
    int64 on the device; key_mask None or contiguous fp32 [N, Tk] there, Tk being the rows unless stated (a ring states its
    logical capacity, which the grid, the splits and the workspace follow too).  Returns (out [N, Tq, H, D], the
    bf_attn_decode_t shape, ws); decode: ws is `workspace` or a fresh tensor of bf_attention_decode_workspace_bytes (None
    when the shape needs none), else None."""
    _require_device(q, f"{name}: q")
    if scales is not None:
        if q.dtype != torch.bfloat16:
            raise _C.BayeFormersAMDError(f"{name}: q must be bfloat16 (got {q.dtype}): the FP8 cache's dequantised rows are "
                                         "exact in bfloat16 alone")
        _kv8_cache_check(name, k, v, *scales)
    elif q.dtype not in (torch.bfloat16, torch.float16) or k.dtype != q.dtype or v.dtype != q.dtype:
        raise _C.BayeFormersAMDError(f"{name}: q, k and v must share one dtype, bfloat16 or float16 (got {q.dtype}, "
                                     f"{k.dtype}, {v.dtype})")
    if q.dim() != 4 or k.dim() != 4 or tuple(v.shape) != tuple(k.shape) or k.shape[0] != q.shape[0] \
            or k.shape[3] != q.shape[3]:
        raise _C.BayeFormersAMDError(f"{name}: q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)} "
                                     "are not [N, H, Tq, D], [N, Hkv, Tk, D], [N, Hkv, Tk, D]")
    if not (k.is_cuda and v.is_cuda) or k.device != q.device or v.device != q.device:
        raise _C.BayeFormersAMDError(f"{name}: q, k and v must share one device")
    if q.stride(3) != 1 or k.stride(3) != 1 or v.stride(3) != 1:
        raise _C.BayeFormersAMDError(f"{name}: the feature dimension of q, k and v must be contiguous")
    if kv_len is not None and (kv_len.dtype != torch.int64 or kv_len.numel() != 1 or kv_len.device != q.device):
        raise _C.BayeFormersAMDError(f"{name}: kv_len must be one int64 on the device of q")
    N, H, Tq, D = q.shape
    shape = _decode_shape(q, k, v)
    if Tk is not None:
        shape.Tk = int(Tk)
    if key_mask is not None and (key_mask.dtype != torch.float32 or tuple(key_mask.shape) != (N, shape.Tk)
                                 or not key_mask.is_contiguous() or key_mask.device != q.device):
        raise _C.BayeFormersAMDError(f"{name}: key_mask must be contiguous fp32 [N, Tk] = {(N, shape.Tk)} on the device of q")
    out = torch.empty((N, Tq, H, D), dtype=q.dtype, device=q.device)
    ws = None
    if decode:
        nbytes = int(_C.lib().bf_attention_decode_workspace_bytes(ctypes.byref(shape)))
        if nbytes < 0:
            _C.check(1, "bf_attention_decode_workspace_bytes")
        if nbytes:
            ws = workspace if workspace is not None else torch.empty(nbytes, dtype=torch.uint8, device=q.device)
            if ws.numel() * ws.element_size() < nbytes or not ws.is_cuda:
                raise _C.BayeFormersAMDError(f"{name}: the workspace needs {nbytes} device bytes")
    return out, shape, ws


def _attention_decode(name: str, q: Tensor, k: Tensor, v: Tensor, kv_len: Optional[Tensor], key_mask: Optional[Tensor],
                      scaling: float, mask_off: Optional[Tensor], workspace: Optional[Tensor],
                      window: Optional[int], softcap: Optional[float] = None) -> Tensor:
    """attention_forward_decode (kv_len None) and attention_forward_decode_len; `name` is the caller's, for the messages."""
    out, shape, ws = _cached_call(name, q, k, v, None, kv_len, key_mask, workspace)
    args = [q.data_ptr(), k.data_ptr(), v.data_ptr(), key_mask.data_ptr() if key_mask is not None else None,
            mask_off.data_ptr() if mask_off is not None else None, out.data_ptr(), ws.data_ptr() if ws is not None else None,
            _TORCH2BF[q.dtype], ctypes.byref(shape)]
    if softcap is not None:  # one entry: a nullable kv_len, window 0 = none
        args.insert(5, kv_len.data_ptr() if kv_len is not None else None)
        _C.check(_C.lib().bf_attention_decode_gqa_softcap(*args, int(window or 0), float(softcap), float(scaling),
                                                          _stream_ptr()), "bf_attention_decode_gqa_softcap")
        SOFTCAP_CALLS["decode" if kv_len is None else "decode_len"] += 1
        return out
    entry, key = "bf_attention_decode_gqa", "fwd"
    if kv_len is not None:
        args.insert(5, kv_len.data_ptr())
        entry, key = entry + "_len", "len"
    if window is not None:
        args.append(int(window))
        entry, key = entry + "_window", "window" if kv_len is None else "len_window"
    _C.check(getattr(_C.lib(), entry)(*args, float(scaling), _stream_ptr()), entry)
    DECODE_CALLS[key] += 1
    return out


def attention_forward_decode(q: Tensor, k: Tensor, v: Tensor, key_mask: Optional[Tensor], scaling: float,
                             mask_off: Optional[Tensor] = None, workspace: Optional[Tensor] = None,
                             window: Optional[int] = None, softcap: Optional[float] = None) -> Tensor:
    """Causal attention of Tq new queries against a KV cache (bf_attention_decode_gqa): q [N, H, Tq, D], k / v
    [N, Hkv, Tk, D] as described by attention_decode_supported; query i sees keys 0 .. Tk - Tq + i.  key_mask: additive
    fp32 [N, Tk] or None; mask_off: optional 1-element device flag, true = the mask hides nothing.  Returns [N, Tq, H, D]
    contiguous (a query with no visible key gives 0).  The split partials go to `workspace` (uint8, at least
    attention_decode_workspace_bytes) or to a fresh tensor of the caching allocator — either way capturable.  window: a
    sliding window of that many keys (bf_attention_decode_gqa_window): query i sees keys Tk - Tq + i - window + 1 ..
    Tk - Tq + i; the workspace is the same.  softcap: soft-capped logits as attention_forward_gqa's
    (bf_attention_decode_gqa_softcap), the same workspace again."""
    return _attention_decode("attention_forward_decode", q, k, v, None, key_mask, scaling, mask_off, workspace, window,
                             softcap)


def attention_forward_decode_len(q: Tensor, k: Tensor, v: Tensor, kv_len: Tensor, key_mask: Optional[Tensor],
                                 scaling: float, mask_off: Optional[Tensor] = None,
                                 workspace: Optional[Tensor] = None, window: Optional[int] = None,
                                 softcap: Optional[float] = None) -> Tensor:
    """attention_forward_decode over a fixed-capacity cache (bf_attention_decode_gqa_len): k / v [N, Hkv, capacity, D] of
    which the first L = kv_len keys are filled, kv_len a one-element int64 device tensor read by the kernel (keys past it
    are never read).  Query i sees keys 0 .. L - Tq + i; key_mask is [N, capacity].  One launch serves every L, so a
    captured call replays correctly while the cache fills; at L == capacity it is bitwise attention_forward_decode.
    window: a sliding window of that many keys (bf_attention_decode_gqa_len_window): query i sees keys
    L - Tq + i - window + 1 .. L - Tq + i, and the key split is laid over the keys some query sees.  softcap:
    soft-capped logits (bf_attention_decode_gqa_softcap with the kv_len)."""
    if kv_len is None:
        raise _C.BayeFormersAMDError("attention_forward_decode_len: kv_len must be one int64 on the device of q")
    return _attention_decode("attention_forward_decode_len", q, k, v, kv_len, key_mask, scaling, mask_off, workspace, window,
                             softcap)


# launches of the FP8 KV-cache entries (include/bayeformers_amd_kv8.h) from this process: bf_kv8_append, bf_attention_decode_gqa_kv8,
# bf_kv8_dequantize.  The kv8 decode bumps neither DECODE_CALLS nor SOFTCAP_CALLS.
KV8_CALLS = {"append": 0, "decode": 0, "dequantize": 0}
KV8_HEAD_SIZES = (64, 128, 256)


def _kv8_cache_check(what: str, kq: Tensor, vq: Tensor, k_scale: Tensor, v_scale: Tensor) -> None:
    """The four tensors of an FP8 cache: kq / vq [N, Hkv, capacity, D] uint8 and k_scale / v_scale [N, Hkv, capacity] fp32 on
    one ROCm device."""
    for name, t in (("kq", kq), ("vq", vq), ("k_scale", k_scale), ("v_scale", v_scale)):
        _require_device(t, f"{what}: {name}")
    if kq.dtype != torch.uint8 or vq.dtype != torch.uint8 or kq.dim() != 4 or tuple(vq.shape) != tuple(kq.shape):
        raise _C.BayeFormersAMDError(f"{what}: kq and vq must be uint8 [N, Hkv, capacity, D] of one shape (got {kq.dtype} "
                                     f"{tuple(kq.shape)}, {vq.dtype} {tuple(vq.shape)})")
    for name, t in (("k_scale", k_scale), ("v_scale", v_scale)):
        if t.dtype != torch.float32 or tuple(t.shape) != tuple(kq.shape[:3]) or not t.is_contiguous():
            raise _C.BayeFormersAMDError(f"{what}: {name} must be contiguous fp32 {tuple(kq.shape[:3])} (got {t.dtype} "
                                         f"{tuple(t.shape)})")
    if len({t.device for t in (kq, vq, k_scale, v_scale)}) != 1:
        raise _C.BayeFormersAMDError(f"{what}: the cache tensors must share one device")


def kv8_append(k: Tensor, v: Tensor, kq: Tensor, vq: Tensor, k_scale: Tensor, v_scale: Tensor, pos: Tensor) -> None:
    """Quantise the new K and V rows of a forward into an FP8 cache (bf_kv8_append): k, v [N, Hkv, Tq, D] bf16 with any
    (batch, head, token) strides that are multiples of 8 and a contiguous feature dimension (HF's transposed projections
    as they come); kq, vq [N, Hkv, capacity, D] uint8 and k_scale, v_scale [N, Hkv, capacity] fp32, contiguous.  Row i goes
    to slot pos + i, pos a one-element int64 device tensor the kernel reads (a slot outside the capacity is skipped).  Each
    row is D e4m3fn bytes over a power-of-two scale: include/bayeformers_amd_kv8.h."""
    what = "kv8_append"
    _require_device(k, f"{what}: k")
    _require_device(v, f"{what}: v")
    if k.dtype != torch.bfloat16 or v.dtype != torch.bfloat16:
        raise _C.BayeFormersAMDError(f"{what}: k and v must be bfloat16 (got {k.dtype}, {v.dtype}): the FP8 cache's "
                                     "dequantised rows are exact in bfloat16 alone")
    _kv8_cache_check(what, kq, vq, k_scale, v_scale)
    if k.dim() != 4 or tuple(v.shape) != tuple(k.shape) or tuple(k.shape[:2]) != tuple(kq.shape[:2]) \
            or k.shape[3] != kq.shape[3]:
        raise _C.BayeFormersAMDError(f"{what}: k {tuple(k.shape)}, v {tuple(v.shape)} are not [N, Hkv, Tq, D] rows of the "
                                     f"cache {tuple(kq.shape)}")
    N, Hkv, Tq, D = k.shape
    if D not in KV8_HEAD_SIZES:
        raise _C.BayeFormersAMDError(f"{what}: head size {D} (64, 128 or 256)")
    if Tq < 1:
        raise _C.BayeFormersAMDError(f"{what}: Tq={Tq} new rows (at least 1)")
    if not (kq.is_contiguous() and vq.is_contiguous()):
        raise _C.BayeFormersAMDError(f"{what}: kq and vq must be contiguous")
    if k.stride(3) != 1 or v.stride(3) != 1 or any(st < 0 or st % 8 for t in (k, v) for st in t.stride()[:3]):
        raise _C.BayeFormersAMDError(f"{what}: k and v need a contiguous feature dimension and (batch, head, token) strides "
                                     "that are non-negative multiples of 8")
    if pos.dtype != torch.int64 or pos.numel() != 1 or pos.device != k.device or kq.device != k.device:
        raise _C.BayeFormersAMDError(f"{what}: pos must be one int64 on the device of k and of the cache")
    strides = [(ctypes.c_int64 * 3)(*t.stride()[:3]) for t in (k, v)]
    _C.check(_C.lib().bf_kv8_append(k.data_ptr(), v.data_ptr(), _C.BF_DT_BF16, strides[0], strides[1], kq.data_ptr(),
                                    vq.data_ptr(), k_scale.data_ptr(), v_scale.data_ptr(), pos.data_ptr(), N, Hkv, Tq, D,
                                    int(kq.shape[2]), _stream_ptr()), "bf_kv8_append")
    KV8_CALLS["append"] += 1


def kv8_dequantize(q: Tensor, scale: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """bf16 rows of an FP8 cache (bf_kv8_dequantize): q [..., D] uint8 contiguous, scale [...] fp32 contiguous -> [..., D]
    bfloat16, float(q) * scale, exact.  For the callers that read a 16-bit cache (every attention route but the kv8 decode
    kernel) and for the tests."""
    what = "kv8_dequantize"
    _require_device(q, f"{what}: q")
    _require_device(scale, f"{what}: scale")
    if q.dtype != torch.uint8 or scale.dtype != torch.float32 or q.dim() < 1 or tuple(scale.shape) != tuple(q.shape[:-1]) \
            or not q.is_contiguous() or not scale.is_contiguous() or scale.device != q.device:
        raise _C.BayeFormersAMDError(f"{what}: q must be contiguous uint8 [..., D] and scale contiguous fp32 [...] on its "
                                     f"device (got {q.dtype} {tuple(q.shape)}, {scale.dtype} {tuple(scale.shape)})")
    D = q.shape[-1]
    if D < 16 or D % 16:
        raise _C.BayeFormersAMDError(f"{what}: D={D} must be a positive multiple of 16")
    if out is None:
        out = torch.empty(q.shape, dtype=torch.bfloat16, device=q.device)
    elif out.dtype != torch.bfloat16 or tuple(out.shape) != tuple(q.shape) or not out.is_contiguous() or out.device != q.device:
        raise _C.BayeFormersAMDError(f"{what}: out must be contiguous bfloat16 {tuple(q.shape)} on the device of q")
    rows = q.numel() // D
    if rows:
        _C.check(_C.lib().bf_kv8_dequantize(q.data_ptr(), scale.data_ptr(), out.data_ptr(), _C.BF_DT_BF16, rows, D,
                                            _stream_ptr()), "bf_kv8_dequantize")
        KV8_CALLS["dequantize"] += 1
    return out


def attention_decode_kv8_supported(q: Tensor, kq: Tensor, vq: Tensor, check_device: bool = True) -> bool:
    """What bf_attention_decode_gqa_kv8 takes: attention_decode_supported's shapes with q bfloat16 and kq / vq uint8
    [N, Hkv, Tk, D] whose (batch, head, token) strides are multiples of 16 bytes."""
    return _cached_layout_ok(q, kq, vq, check_device, fp8=True, chunk=False)


def attention_forward_decode_kv8(q: Tensor, kq: Tensor, vq: Tensor, k_scale: Tensor, v_scale: Tensor,
                                 kv_len: Optional[Tensor], key_mask: Optional[Tensor], scaling: float,
                                 mask_off: Optional[Tensor] = None, workspace: Optional[Tensor] = None,
                                 window: Optional[int] = None, softcap: Optional[float] = None) -> Tensor:
    """attention_forward_decode (kv_len None) / attention_forward_decode_len on an FP8 cache (bf_attention_decode_gqa_kv8):
    q [N, H, Tq, D] bfloat16, kq / vq [N, Hkv, Tk, D] uint8 (e4m3fn rows), k_scale / v_scale [N, Hkv, Tk] fp32 contiguous.
    key_mask, mask_off, workspace (attention_decode_workspace_bytes of the shape), window and softcap as there.  The rows
    are dequantised in registers on their way to LDS; the result is bitwise that of the bf16 entry on
    kv8_dequantize(kq, k_scale), kv8_dequantize(vq, v_scale)."""
    out, shape, ws = _cached_call("attention_forward_decode_kv8", q, kq, vq, (k_scale, v_scale), kv_len, key_mask, workspace)
    _C.check(_C.lib().bf_attention_decode_gqa_kv8(
        q.data_ptr(), kq.data_ptr(), vq.data_ptr(), k_scale.data_ptr(), v_scale.data_ptr(),
        key_mask.data_ptr() if key_mask is not None else None, mask_off.data_ptr() if mask_off is not None else None,
        kv_len.data_ptr() if kv_len is not None else None, out.data_ptr(), ws.data_ptr() if ws is not None else None,
        _C.BF_DT_BF16, ctypes.byref(shape), int(window or 0), float(softcap or 0.0), float(scaling), _stream_ptr()),
        "bf_attention_decode_gqa_kv8")
    KV8_CALLS["decode"] += 1
    return out


# launches of the ring-buffer KV-cache entries (include/bayeformers_amd_ring.h) from this process: bf_kv_ring_append,
# bf_kv8_ring_append, bf_attention_decode_gqa_ring, bf_attention_decode_gqa_ring_kv8.  They bump no other counter.
RING_CALLS = {"append": 0, "kv8_append": 0, "decode": 0, "kv8_decode": 0}


def ring_slots(window: Optional[int], capacity: int) -> Optional[int]:
    """The slots C a sliding-window layer's ring buffer holds (sample_generate(sliding_cache="ring")), or None where the
    layer stays a plain full-capacity one: no window, or C >= capacity.  C = window + DECODE_MAX_QUERIES - 1: a step that
    appends Tq <= 16 rows at fill L reads the keys [L - window + 1, L + Tq) at most — window + Tq - 1 <= C of them — so none
    of the keys it reads was overwritten by the rows it appended.  The one place the rule lives."""
    if window is None:
        return None
    window, capacity = int(window), int(capacity)
    if window < 1 or capacity < 1:
        raise ValueError(f"ring_slots: window={window}, capacity={capacity} (each at least 1)")
    C = window + DECODE_MAX_QUERIES - 1
    return C if C < capacity else None


def _ring_append_check(what: str, k: Tensor, v: Tensor, kc: Tensor, vc: Tensor, pos: Tensor) -> None:
    """The arguments the two ring appends share: k, v [N, Hkv, T, D] rows for the contiguous caches kc, vc
    [N, Hkv, ring_slots, D] on one ROCm device, pos one int64 on it."""
    for name, t in (("k", k), ("v", v), ("kc", kc), ("vc", vc)):
        _require_device(t, f"{what}: {name}")
    if kc.dim() != 4 or tuple(vc.shape) != tuple(kc.shape) or not (kc.is_contiguous() and vc.is_contiguous()):
        raise _C.BayeFormersAMDError(f"{what}: the cache tensors must be contiguous [N, Hkv, ring_slots, D] of one shape "
                                     f"(got {tuple(kc.shape)}, {tuple(vc.shape)})")
    if k.dim() != 4 or tuple(v.shape) != tuple(k.shape) or tuple(k.shape[:2]) != tuple(kc.shape[:2]) \
            or k.shape[3] != kc.shape[3]:
        raise _C.BayeFormersAMDError(f"{what}: k {tuple(k.shape)}, v {tuple(v.shape)} are not [N, Hkv, T, D] rows of the "
                                     f"cache {tuple(kc.shape)}")
    if k.shape[3] not in KV8_HEAD_SIZES:
        raise _C.BayeFormersAMDError(f"{what}: head size {k.shape[3]} (64, 128 or 256)")
    if k.shape[2] < 1:
        raise _C.BayeFormersAMDError(f"{what}: T={k.shape[2]} new rows (at least 1)")
    if k.stride(3) != 1 or v.stride(3) != 1 or any(st < 0 or st % 8 for t in (k, v) for st in t.stride()[:3]):
        raise _C.BayeFormersAMDError(f"{what}: k and v need a contiguous feature dimension and (batch, head, token) strides "
                                     "that are non-negative multiples of 8")
    if pos.dtype != torch.int64 or pos.numel() != 1 or len({t.device for t in (k, v, kc, vc, pos)}) != 1:
        raise _C.BayeFormersAMDError(f"{what}: pos must be one int64 on the device of k, v and the cache")


def kv_ring_append(k: Tensor, v: Tensor, kc: Tensor, vc: Tensor, pos: Tensor) -> None:
    """Append the new K and V rows of a forward to a ring-buffer cache (bf_kv_ring_append): k, v [N, Hkv, T, D] bf16 or
    fp16 with any (batch, head, token) strides that are multiples of 8 and a contiguous feature dimension; kc, vc
    [N, Hkv, ring_slots, D] of the same dtype, contiguous.  Row i goes to slot (pos + i) % ring_slots, pos a one-element
    int64 device tensor the kernel reads; of T > ring_slots rows only the last ring_slots are written.  One launch."""
    what = "kv_ring_append"
    _ring_append_check(what, k, v, kc, vc, pos)
    if k.dtype not in (torch.bfloat16, torch.float16) or len({k.dtype, v.dtype, kc.dtype, vc.dtype}) != 1:
        raise _C.BayeFormersAMDError(f"{what}: k, v and the cache must share bfloat16 or float16 (got {k.dtype}, {v.dtype}, "
                                     f"{kc.dtype}, {vc.dtype})")
    N, Hkv, T, D = k.shape
    strides = [(ctypes.c_int64 * 3)(*t.stride()[:3]) for t in (k, v)]
    _C.check(_C.lib().bf_kv_ring_append(k.data_ptr(), v.data_ptr(), _TORCH2BF[k.dtype], strides[0], strides[1],
                                        kc.data_ptr(), vc.data_ptr(), pos.data_ptr(), N, Hkv, T, D, int(kc.shape[2]),
                                        _stream_ptr()), "bf_kv_ring_append")
    RING_CALLS["append"] += 1


def kv8_ring_append(k: Tensor, v: Tensor, kq: Tensor, vq: Tensor, k_scale: Tensor, v_scale: Tensor, pos: Tensor) -> None:
    """kv_ring_append into an FP8 ring (bf_kv8_ring_append): kv8_append's quantisation and arguments — k, v bfloat16, kq /
    vq [N, Hkv, ring_slots, D] uint8, k_scale / v_scale [N, Hkv, ring_slots] fp32 — with row i bound for slot
    (pos + i) % ring_slots and, of T > ring_slots rows, only the last ring_slots written."""
    what = "kv8_ring_append"
    _kv8_cache_check(what, kq, vq, k_scale, v_scale)
    _ring_append_check(what, k, v, kq, vq, pos)
    if k.dtype != torch.bfloat16 or v.dtype != torch.bfloat16:
        raise _C.BayeFormersAMDError(f"{what}: k and v must be bfloat16 (got {k.dtype}, {v.dtype}): the FP8 cache's "
                                     "dequantised rows are exact in bfloat16 alone")
    N, Hkv, T, D = k.shape
    strides = [(ctypes.c_int64 * 3)(*t.stride()[:3]) for t in (k, v)]
    _C.check(_C.lib().bf_kv8_ring_append(k.data_ptr(), v.data_ptr(), _C.BF_DT_BF16, strides[0], strides[1], kq.data_ptr(),
                                         vq.data_ptr(), k_scale.data_ptr(), v_scale.data_ptr(), pos.data_ptr(), N, Hkv, T,
                                         D, int(kq.shape[2]), _stream_ptr()), "bf_kv8_ring_append")
    RING_CALLS["kv8_append"] += 1


def _ring_call(name: str, q: Tensor, k: Tensor, v: Tensor, scales, kv_len: Tensor, key_mask: Optional[Tensor],
               workspace: Optional[Tensor], window: int, slots: Optional[int], capacity: Optional[int]):
    """_cached_call for the two ring decodes — k / v [N, Hkv, ring_slots, D], the shape carrying the logical capacity as its
    Tk — behind what a ring alone requires: the fill, and a window that fits the slots with the queries."""
    if slots is None or capacity is None:
        raise _C.BayeFormersAMDError(f"{name}: ring_slots and capacity are required")
    if kv_len is None:
        raise _C.BayeFormersAMDError(f"{name}: kv_len must be one int64 on the device of q")
    out, shape, ws = _cached_call(name, q, k, v, scales, kv_len, key_mask, workspace, Tk=capacity)
    if k.shape[2] != int(slots):
        raise _C.BayeFormersAMDError(f"{name}: k and v hold {k.shape[2]} rows, not ring_slots={int(slots)}")
    if window is None or int(window) < 1 or int(window) + q.shape[2] - 1 > int(slots):
        raise _C.BayeFormersAMDError(f"{name}: window={window} with Tq={q.shape[2]} needs window >= 1 and "
                                     f"window + Tq - 1 <= ring_slots={int(slots)}")
    return out, shape, ws


def attention_forward_decode_ring(q: Tensor, k: Tensor, v: Tensor, kv_len: Tensor, key_mask: Optional[Tensor],
                                  scaling: float, mask_off: Optional[Tensor] = None, workspace: Optional[Tensor] = None,
                                  window: Optional[int] = None, ring_slots: Optional[int] = None,
                                  capacity: Optional[int] = None, softcap: Optional[float] = None) -> Tensor:
    """attention_forward_decode_len with a window over a ring-buffer cache (bf_attention_decode_gqa_ring): k / v
    [N, Hkv, ring_slots, D] hold the key with sequence index j in row j % ring_slots; kv_len is the fill L (every row ever
    appended: it does not wrap), `capacity` the logical capacity — the grid, the key split, the workspace
    (attention_decode_workspace_bytes of a [N, Hkv, capacity, D] cache) and key_mask [N, capacity] follow it.  Query i
    sees keys L - Tq + i - window + 1 .. L - Tq + i; window >= 1 and window + Tq - 1 <= ring_slots.  The result is bitwise
    attention_forward_decode_len(..., window=window)'s on the same keys in a linear cache of `capacity` rows."""
    out, shape, ws = _ring_call("attention_forward_decode_ring", q, k, v, None, kv_len, key_mask, workspace, window, ring_slots,
                                capacity)
    _C.check(_C.lib().bf_attention_decode_gqa_ring(
        q.data_ptr(), k.data_ptr(), v.data_ptr(), key_mask.data_ptr() if key_mask is not None else None,
        mask_off.data_ptr() if mask_off is not None else None, kv_len.data_ptr(), out.data_ptr(),
        ws.data_ptr() if ws is not None else None, _TORCH2BF[q.dtype], ctypes.byref(shape), int(ring_slots), int(window),
        float(softcap or 0.0), float(scaling), _stream_ptr()), "bf_attention_decode_gqa_ring")
    RING_CALLS["decode"] += 1
    return out


def attention_forward_decode_ring_kv8(q: Tensor, kq: Tensor, vq: Tensor, k_scale: Tensor, v_scale: Tensor, kv_len: Tensor,
                                      key_mask: Optional[Tensor], scaling: float, mask_off: Optional[Tensor] = None,
                                      workspace: Optional[Tensor] = None, window: Optional[int] = None,
                                      ring_slots: Optional[int] = None, capacity: Optional[int] = None,
                                      softcap: Optional[float] = None) -> Tensor:
    """attention_forward_decode_ring on an FP8 ring (bf_attention_decode_gqa_ring_kv8): q bfloat16, kq / vq
    [N, Hkv, ring_slots, D] uint8 (e4m3fn rows), k_scale / v_scale [N, Hkv, ring_slots] fp32 contiguous.  Bitwise
    attention_forward_decode_kv8(..., window=window)'s result on the same rows in a linear FP8 cache of `capacity` rows."""
    out, shape, ws = _ring_call("attention_forward_decode_ring_kv8", q, kq, vq, (k_scale, v_scale), kv_len, key_mask, workspace,
                                window, ring_slots, capacity)
    _C.check(_C.lib().bf_attention_decode_gqa_ring_kv8(
        q.data_ptr(), kq.data_ptr(), vq.data_ptr(), k_scale.data_ptr(), v_scale.data_ptr(),
        key_mask.data_ptr() if key_mask is not None else None, mask_off.data_ptr() if mask_off is not None else None,
        kv_len.data_ptr(), out.data_ptr(), ws.data_ptr() if ws is not None else None, _C.BF_DT_BF16, ctypes.byref(shape),
        int(ring_slots), int(window), float(softcap or 0.0), float(scaling), _stream_ptr()),
        "bf_attention_decode_gqa_ring_kv8")
    RING_CALLS["kv8_decode"] += 1
    return out


# launches of the cached-chunk attention entries (include/bayeformers_amd_chunk.h) from this process: "fwd" of
# bf_attention_chunk_gqa, "kv8" of bf_attention_chunk_gqa_kv8.  They bump no other counter.
CHUNK_CALLS = {"fwd": 0, "kv8": 0}


def attention_chunk_supported(q: Tensor, k: Tensor, v: Tensor, check_device: bool = True) -> bool:
    """What bf_attention_chunk_gqa takes: q [N, H, Tq, D] with any 1 <= Tq <= Tk, k and v [N, Hkv, Tk, D], Hkv dividing H, D
    64, 128 or 256, bf16 or fp16, each with its own (batch, head, token) strides (non-negative multiples of 8 elements) and a
    contiguous feature dimension.  check_device=False judges the shapes, dtypes and strides alone (CPU or meta tensors)."""
    return _cached_layout_ok(q, k, v, check_device, fp8=False, chunk=True)


def attention_chunk_kv8_supported(q: Tensor, kq: Tensor, vq: Tensor, check_device: bool = True) -> bool:
    """What bf_attention_chunk_gqa_kv8 takes: attention_chunk_supported's shapes with q bfloat16 and kq / vq uint8
    [N, Hkv, Tk, D] whose (batch, head, token) strides are multiples of 16 bytes."""
    return _cached_layout_ok(q, kq, vq, check_device, fp8=True, chunk=True)


def _chunk_call(name: str, q: Tensor, k: Tensor, v: Tensor, scales, kv_len: Optional[Tensor], key_mask: Optional[Tensor],
                mask_off: Optional[Tensor], window: Optional[int], softcap: Optional[float], key_origin: int):
    """_cached_call for the two chunk wrappers (no workspace), and the arguments only they check."""
    out, shape, _ = _cached_call(name, q, k, v, scales, kv_len, key_mask, decode=False)
    if not 1 <= q.shape[2] <= k.shape[2]:
        raise _C.BayeFormersAMDError(f"{name}: Tq={q.shape[2]} new queries against Tk={k.shape[2]} cached keys "
                                     "(1 <= Tq <= Tk)")
    if mask_off is not None and (mask_off.numel() != 1 or mask_off.element_size() != 1 or mask_off.device != q.device):
        raise _C.BayeFormersAMDError(f"{name}: mask_off must be one byte on the device of q")
    if window is not None and (isinstance(window, bool) or not isinstance(window, int) or window < 1):
        raise _C.BayeFormersAMDError(f"{name}: window={window!r} (None or an int >= 1)")
    if softcap is not None and not (math.isfinite(softcap) and softcap > 0.0):
        raise _C.BayeFormersAMDError(f"{name}: softcap={softcap!r} (None or finite and positive)")
    if isinstance(key_origin, bool) or not isinstance(key_origin, int) or not 0 <= key_origin < 2 ** 31:
        raise _C.BayeFormersAMDError(f"{name}: key_origin={key_origin!r} (an int >= 0)")
    return out, shape


def attention_forward_chunk(q: Tensor, k: Tensor, v: Tensor, kv_len: Optional[Tensor], key_mask: Optional[Tensor],
                            scaling: float, mask_off: Optional[Tensor] = None, window: Optional[int] = None,
                            softcap: Optional[float] = None, key_origin: int = 0) -> Tensor:
    """Causal attention of a chunk of Tq new queries against a KV cache (bf_attention_chunk_gqa): q [N, H, Tq, D], k / v
    [N, Hkv, Tk, D] as described by attention_chunk_supported.  kv_len: None (L = Tk) or a one-element int64 device tensor
    read by the kernel, the fill L of a fixed-capacity cache after this call's rows were appended (keys past it are never
    read; one captured launch serves every L).  Query i has position L - Tq + i and sees the keys up to it — with `window`
    the last `window` of them — that key_mask (additive fp32 [N, Tk] or None; mask_off: optional 1-element device flag,
    true = the mask hides nothing) leaves visible.  softcap: soft-capped logits as attention_forward_gqa's.  key_origin: the
    index in its sequence of k's key 0 (a sliding-window cache that kept its last keys only): the kernel lays its key tiles on
    the sequence's tile grid, so the rows round as the same rows of attention_forward_gqa over the whole sequence.  Forward only.
    Returns [N, Tq, H, D] contiguous (a query with no visible key gives 0)."""
    out, shape = _chunk_call("attention_forward_chunk", q, k, v, None, kv_len, key_mask, mask_off, window, softcap, key_origin)
    _C.check(_C.lib().bf_attention_chunk_gqa(
        q.data_ptr(), k.data_ptr(), v.data_ptr(), key_mask.data_ptr() if key_mask is not None else None,
        mask_off.data_ptr() if mask_off is not None else None, kv_len.data_ptr() if kv_len is not None else None,
        out.data_ptr(), _TORCH2BF[q.dtype], ctypes.byref(shape), int(window or 0), key_origin, float(softcap or 0.0), float(scaling),
        _stream_ptr()), "bf_attention_chunk_gqa")
    CHUNK_CALLS["fwd"] += 1
    return out


def attention_forward_chunk_kv8(q: Tensor, kq: Tensor, vq: Tensor, k_scale: Tensor, v_scale: Tensor,
                                kv_len: Optional[Tensor], key_mask: Optional[Tensor], scaling: float,
                                mask_off: Optional[Tensor] = None, window: Optional[int] = None,
                                softcap: Optional[float] = None, key_origin: int = 0) -> Tensor:
    """attention_forward_chunk on an FP8 cache (bf_attention_chunk_gqa_kv8): q [N, H, Tq, D] bfloat16, kq / vq
    [N, Hkv, Tk, D] uint8 (e4m3fn rows), k_scale / v_scale [N, Hkv, Tk] fp32 contiguous; the other arguments as there.  The
    rows are dequantised in registers on their way to LDS — rows and scales past the fill are never read — and the result
    is bitwise that of attention_forward_chunk on kv8_dequantize(kq, k_scale), kv8_dequantize(vq, v_scale)."""
    out, shape = _chunk_call("attention_forward_chunk_kv8", q, kq, vq, (k_scale, v_scale), kv_len, key_mask, mask_off, window,
                             softcap, key_origin)
    _C.check(_C.lib().bf_attention_chunk_gqa_kv8(
        q.data_ptr(), kq.data_ptr(), vq.data_ptr(), k_scale.data_ptr(), v_scale.data_ptr(),
        key_mask.data_ptr() if key_mask is not None else None, mask_off.data_ptr() if mask_off is not None else None,
        kv_len.data_ptr() if kv_len is not None else None, out.data_ptr(), _C.BF_DT_BF16, ctypes.byref(shape),
        int(window or 0), key_origin, float(softcap or 0.0), float(scaling), _stream_ptr()), "bf_attention_chunk_gqa_kv8")
    CHUNK_CALLS["kv8"] += 1
    return out


GENERATE_CALLS = [0]  # launches of bf_generate_step through generate_step (tests, diagnostics)


def generate_step(probs: Tensor, predictive_entropy: Tensor, expected_entropy: Tensor, mutual_information: Tensor,
                  samples: int, state: Tensor, sequences: Tensor, T0: int, stats: Tensor, finished: Optional[Tensor],
                  lengths: Tensor, next_ids: Tensor, positions: Optional[Tensor], eos_token_id: Optional[int],
                  pad_token_id: int, seed: Optional[Tensor] = None, stat_probs: Optional[Tensor] = None) -> None:
    """One generation step's epilogue in one launch (bf_generate_step), at the step state[0]: the token of each of the B
    rows of probs [B, V] (fp32: the lowest-index argmax, or with `seed` — a one-element int64 device tensor — an
    inverse-CDF draw of a Philox uniform), written into sequences [B, T0 + n] at T0 + step, the four statistics
    (predictive_entropy, expected_entropy, mutual_information [B], the token's probability) into stats [4, B, n] at step
    (zero for rows finished before it), finished [B] bool and lengths [B] int64 updated as sample_generate's loop does
    with eos_token_id (None: every row counts the token), the token into next_ids [samples * B] (sample-major) and
    positions [samples * B] (or None) advanced by one; state [2] int64 {step, 0} advances by one.  With stat_probs
    ([B, V] like probs; bf_generate_step_stat_probs) the token's probability statistic is read from it instead of from
    probs: the token is chosen from processed rows, its probability is the unprocessed one.  No host synchronisation:
    capturable."""
    _require_device(probs, "generate_step: probs")
    if probs.dim() != 2 or probs.dtype != torch.float32 or not probs.is_contiguous():
        raise _C.BayeFormersAMDError("generate_step: probs must be contiguous fp32 [B, V]")
    B, V = probs.shape
    n = stats.shape[-1] if stats.dim() == 3 else 0
    dev = probs.device

    def need(t, what, dtype, shape):
        if t is None or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev:
            raise _C.BayeFormersAMDError(f"generate_step: {what} must be contiguous {dtype} {list(shape)} on {dev}")

    for t, what in ((predictive_entropy, "predictive_entropy"), (expected_entropy, "expected_entropy"),
                    (mutual_information, "mutual_information")):
        need(t, what, torch.float32, (B,))
    need(stats, "stats", torch.float32, (4, B, n))
    need(state, "state", torch.int64, (2,))
    need(lengths, "lengths", torch.int64, (B,))
    need(next_ids, "next_ids", torch.int64, (int(samples) * B,))
    if positions is not None:
        need(positions, "positions", torch.int64, (int(samples) * B,))
    if sequences.dim() != 2 or sequences.shape[0] != B or sequences.stride(1) != 1 or sequences.dtype != torch.int64 \
            or sequences.device != dev:
        raise _C.BayeFormersAMDError("generate_step: sequences must be int64 [B, T0 + n] with contiguous rows")
    if eos_token_id is not None:
        need(finished, "finished", torch.bool, (B,))
    if seed is not None:
        need(seed, "seed", torch.int64, (1,))
    args = (predictive_entropy.data_ptr(), expected_entropy.data_ptr(), mutual_information.data_ptr(), B, V, int(samples),
            state.data_ptr(), n, sequences.data_ptr(), sequences.stride(0), int(T0), stats.data_ptr(),
            finished.data_ptr() if finished is not None else None, lengths.data_ptr(), next_ids.data_ptr(),
            positions.data_ptr() if positions is not None else None,
            int(eos_token_id) if eos_token_id is not None else -1, int(pad_token_id), 1 if seed is not None else 0,
            seed.data_ptr() if seed is not None else None, _stream_ptr())
    if stat_probs is None:
        _C.check(_C.lib().bf_generate_step(probs.data_ptr(), *args), "bf_generate_step")
    else:
        need(stat_probs, "stat_probs", torch.float32, (B, V))
        _C.check(_C.lib().bf_generate_step_stat_probs(probs.data_ptr(), stat_probs.data_ptr(), *args),
                 "bf_generate_step_stat_probs")
    GENERATE_CALLS[0] += 1


SPEC_ACCEPT_CALLS = [0]  # launches of bf_spec_accept through speculative_accept (tests, diagnostics)


def speculative_accept(argmax: Tensor, draft: Tensor, probs: Tensor, predictive_entropy: Tensor, expected_entropy: Tensor,
                       mutual_information: Tensor, samples: int, state: Tensor, sequences: Tensor, T0: int, stats: Tensor,
                       finished: Optional[Tensor], lengths: Tensor, verify_ids: Tensor, verify_positions: Optional[Tensor],
                       draft_ids: Tensor, draft_positions: Optional[Tensor], rewind: Tensor, speculation: Tensor,
                       eos_token_id: Optional[int], pad_token_id: int) -> None:
    """The epilogue of one speculative iteration in one launch (bf_spec_accept; contract in include/bayeformers_amd_spec.h), at
    the step state[0]: argmax [B, γ+1] int64 (the model-average argmax of each verified position), draft [B, γ] int64,
    probs [B·(γ+1), V] fp32 and the three entropies [B·(γ+1)] → the a + 1 kept tokens of every row (a: the shortest run
    of agreeing drafts over the unfinished rows, clipped to the tokens left) into sequences [B, T0 + n] and stats
    [4, B, n], finished [B] bool and lengths [B] int64 as generate_step updates them; column 0 of verify_ids
    [samples·B, γ+1], draft_ids [B, 2], a + 1 added to verify_positions [samples·B, γ+1] and draft_positions [B, γ+1]
    (or None), state[0] += a + 1, rewind [1] = γ − a and speculation [3] += {1, drafts that had room, a}.  No host
    synchronisation: capturable."""
    _require_device(probs, "speculative_accept: probs")
    if probs.dim() != 2 or probs.dtype != torch.float32 or not probs.is_contiguous():
        raise _C.BayeFormersAMDError("speculative_accept: probs must be contiguous fp32 [B * (gamma + 1), V]")
    if draft.dim() != 2 or draft.shape[0] < 1 or draft.shape[1] < 1:
        raise _C.BayeFormersAMDError("speculative_accept: draft must be int64 [B, gamma] with B, gamma >= 1")
    B, G = draft.shape
    R, V = probs.shape
    n = stats.shape[-1] if stats.dim() == 3 else 0
    S, dev = int(samples), probs.device
    if R != B * (G + 1) or R > SKINNY_ROWS:
        raise _C.BayeFormersAMDError(f"speculative_accept: probs has {R} rows for B={B}, gamma={G}: B * (gamma + 1), at "
                                     f"most {SKINNY_ROWS}")

    def need(t, what, dtype, shape):
        if t is None or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev:
            raise _C.BayeFormersAMDError(f"speculative_accept: {what} must be contiguous {dtype} {list(shape)} on {dev}")

    need(argmax, "argmax", torch.int64, (B, G + 1))
    need(draft, "draft", torch.int64, (B, G))
    for t, what in ((predictive_entropy, "predictive_entropy"), (expected_entropy, "expected_entropy"),
                    (mutual_information, "mutual_information")):
        need(t, what, torch.float32, (R,))
    need(stats, "stats", torch.float32, (4, B, n))
    need(state, "state", torch.int64, (2,))
    need(lengths, "lengths", torch.int64, (B,))
    need(verify_ids, "verify_ids", torch.int64, (S * B, G + 1))
    need(draft_ids, "draft_ids", torch.int64, (B, 2))
    if verify_positions is not None:
        need(verify_positions, "verify_positions", torch.int64, (S * B, G + 1))
    if draft_positions is not None:
        need(draft_positions, "draft_positions", torch.int64, (B, G + 1))
    need(rewind, "rewind", torch.int64, (1,))
    need(speculation, "speculation", torch.int64, (3,))
    if sequences.dim() != 2 or sequences.shape[0] != B or sequences.stride(1) != 1 or sequences.dtype != torch.int64 \
            or sequences.device != dev:
        raise _C.BayeFormersAMDError("speculative_accept: sequences must be int64 [B, T0 + n] with contiguous rows")
    if eos_token_id is not None:
        need(finished, "finished", torch.bool, (B,))
    _C.check(_C.lib().bf_spec_accept(
        argmax.data_ptr(), draft.data_ptr(), probs.data_ptr(), predictive_entropy.data_ptr(), expected_entropy.data_ptr(),
        mutual_information.data_ptr(), B, G, V, S, state.data_ptr(), n, sequences.data_ptr(), sequences.stride(0), int(T0),
        stats.data_ptr(), finished.data_ptr() if finished is not None else None, lengths.data_ptr(), verify_ids.data_ptr(),
        verify_positions.data_ptr() if verify_positions is not None else None, draft_ids.data_ptr(),
        draft_positions.data_ptr() if draft_positions is not None else None, rewind.data_ptr(), speculation.data_ptr(),
        int(eos_token_id) if eos_token_id is not None else -1, int(pad_token_id), _stream_ptr()), "bf_spec_accept")
    SPEC_ACCEPT_CALLS[0] += 1


TRUNCATE_CALLS = [0]  # launches of bf_probs_truncate through truncate_probs (tests, diagnostics)
TRUNCATE_MAX_V = 524288


def truncate_probs(probs: Tensor, top_k: Optional[int] = None, top_p: Optional[float] = None,
                   min_p: Optional[float] = None, out: Optional[Tensor] = None) -> Tensor:
    """probs [R, V] (contiguous fp32 on the device) truncated for sampling in one launch (bf_probs_truncate): HF's order,
    top-k, then top-p on the renormalised top-k set, then min-p; kept entries are bitwise the input, the others 0 (the
    contract, its tie rule and its fixed-point mass: include/bayeformers_amd.h).  None turns a criterion off.  Writes
    `out` (same shape; may be probs itself) or a new tensor, and returns it.  No host synchronisation: capturable."""
    _require_device(probs, "truncate_probs: probs")
    if probs.dim() != 2 or probs.dtype != torch.float32 or not probs.is_contiguous():
        raise _C.BayeFormersAMDError("truncate_probs: probs must be contiguous fp32 [R, V]")
    R, V = probs.shape
    if V > TRUNCATE_MAX_V:
        raise _C.BayeFormersAMDError(f"truncate_probs: V={V} exceeds {TRUNCATE_MAX_V}")
    if out is None:
        out = torch.empty_like(probs)
    elif out.shape != probs.shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != probs.device:
        raise _C.BayeFormersAMDError(f"truncate_probs: out must be contiguous fp32 {list(probs.shape)} on {probs.device}")
    _C.check(_C.lib().bf_probs_truncate(probs.data_ptr(), out.data_ptr(), R, V, int(top_k) if top_k is not None else 0,
                                        float(top_p) if top_p is not None else 1.0,
                                        float(min_p) if min_p is not None else 0.0, _stream_ptr()), "bf_probs_truncate")
    TRUNCATE_CALLS[0] += 1
    return out


PROCESS_CALLS = [0]  # launches of bf_logits_process through process_logits (tests, diagnostics)
PROCESS_MAX_V = 524288
PROCESS_MAX_NGRAM = 64


def process_logits(logits: Tensor, sequences: Tensor, T0: int, step: Union[int, Tensor], samples: int,
                   repetition_penalty: Optional[float] = None, no_repeat_ngram_size: Optional[int] = None,
                   min_new_tokens: Optional[int] = None, eos_token_id: Optional[int] = None, temperature: float = 1.0,
                   out: Optional[Tensor] = None) -> Tensor:
    """HF's logits processors, then the temperature, in one launch (bf_logits_process): the repetition penalty, the
    no-repeat n-gram ban, the min_new_tokens eos ban and / temperature, bitwise transformers' chain on the fp32 upcast
    (the contract: include/bayeformers_amd.h).  logits [samples * B, V] (bf16, fp16 or fp32, sample-major, unit column
    stride, any row stride: the prefill's out.logits[:, -1, :] is read in place); sequences [B, seq_stride] int64, the
    history of row b being sequences[b, :T0 + step]; step an int, or a device int64 tensor whose first element is read by
    the kernel (sample_generate's step counter: a captured launch follows the replays).  None turns a processor off.
    Writes `out` (contiguous fp32 [samples * B, V]) or a new tensor, and returns it.  No host synchronisation:
    capturable."""
    _require_device(logits, "process_logits: logits")
    if logits.dim() != 2 or logits.dtype not in _TORCH2BF or logits.stride(1) != 1 or logits.shape[1] < 1:
        raise _C.BayeFormersAMDError("process_logits: logits must be bf16, fp16 or fp32 [R, V] with unit column stride")
    R, V = logits.shape
    if V > PROCESS_MAX_V:
        raise _C.BayeFormersAMDError(f"process_logits: V={V} exceeds {PROCESS_MAX_V}")
    if sequences.dim() != 2 or sequences.dtype != torch.int64 or sequences.stride(1) != 1 \
            or sequences.device != logits.device:
        raise _C.BayeFormersAMDError(f"process_logits: sequences must be int64 [B, T] with contiguous rows on "
                                     f"{logits.device}")
    B = sequences.shape[0]
    if R != int(samples) * B:
        raise _C.BayeFormersAMDError(f"process_logits: logits has {R} rows, not samples * B = {int(samples) * B}")
    if isinstance(step, Tensor):
        if step.dtype != torch.int64 or step.numel() < 1 or step.device != logits.device:
            raise _C.BayeFormersAMDError(f"process_logits: a device step must be an int64 tensor on {logits.device}")
        d_step, host_step = step.data_ptr(), 0
    else:
        d_step, host_step = None, int(step)
    if out is None:
        out = torch.empty((R, V), dtype=torch.float32, device=logits.device)
    elif out.shape != (R, V) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != logits.device:
        raise _C.BayeFormersAMDError(f"process_logits: out must be contiguous fp32 [{R}, {V}] on {logits.device}")
    _C.check(_C.lib().bf_logits_process(logits.data_ptr(), _TORCH2BF[logits.dtype], R, V, logits.stride(0),
                                        out.data_ptr(), sequences.data_ptr(), B, sequences.stride(0), int(T0), d_step,
                                        host_step, float(repetition_penalty) if repetition_penalty is not None else 1.0,
                                        int(no_repeat_ngram_size or 0), int(min_new_tokens or 0),
                                        int(eos_token_id) if eos_token_id is not None else -1, float(temperature),
                                        _stream_ptr()), "bf_logits_process")
    PROCESS_CALLS[0] += 1
    return out


class AttentionGqaFn(torch.autograd.Function):
    """attention_forward_gqa with attention_backward_gqa as its backward (no dropout: decoder configs run attention
    without it).  Keeps q, k, v, the output and one fp32 row statistic per query."""

    @staticmethod
    def forward(ctx, q, k, v, key_mask, mask_off, scaling, causal=True, window=None, softcap=None):
        cap = {} if softcap is None else {"softcap": softcap}
        out, lse = attention_forward_gqa(q, k, v, key_mask, scaling, causal, mask_off, want_lse=True, window=window, **cap)
        ctx.save_for_backward(q, k, v, out, lse)
        ctx.key_mask, ctx.mask_off, ctx.scaling, ctx.causal, ctx.window = key_mask, mask_off, scaling, causal, window
        ctx.cap = cap
        return out

    @staticmethod
    def backward(ctx, grad_out):
        q, k, v, out, lse = ctx.saved_tensors
        dq, dk, dv = attention_backward_gqa(q, k, v, ctx.key_mask, ctx.mask_off, out, grad_out, lse, ctx.scaling, ctx.causal,
                                            ctx.window, **ctx.cap)
        return dq.transpose(1, 2), dk.transpose(1, 2), dv.transpose(1, 2), None, None, None, None, None, None


class AttentionGqaBandFn(torch.autograd.Function):
    """attention_forward_gqa_band with attention_backward_gqa_band as its backward.  Keeps q, k, v, the output, one fp32
    row statistic per query and the two bounds."""

    @staticmethod
    def forward(ctx, q, k, v, lo, hi, scaling):
        out, lse = attention_forward_gqa_band(q, k, v, lo, scaling, want_lse=True)
        ctx.save_for_backward(q, k, v, out, lse, lo, hi)
        ctx.scaling = scaling
        return out

    @staticmethod
    def backward(ctx, grad_out):
        q, k, v, out, lse, lo, hi = ctx.saved_tensors
        dq, dk, dv = attention_backward_gqa_band(q, k, v, lo, hi, out, grad_out, lse, ctx.scaling)
        return dq.transpose(1, 2), dk.transpose(1, 2), dv.transpose(1, 2), None, None, None


def attention_forward(q: Tensor, k: Tensor, v: Tensor, key_mask: Optional[Tensor], scaling: float,
                      mask_off: Optional[Tensor] = None, want_lse: bool = False, drop: Optional[Dropout] = None,
                      want_keep: bool = False):
    """softmax(q k^T * scaling + key_mask) v (bf_attention_fwd).  q, k, v: [B, H, T, 64] views as described by
    attention_supported; key_mask: additive fp32 [B, T] or None; mask_off: optional 1-element bool/uint8 device tensor,
    true = the mask is all zeros (the kernel then skips it).  Returns [B, T, H, 64] contiguous — and, with want_lse, the
    [B, H, T] fp32 log-sum-exp rows bf_attention_bwd needs."""
    B, H, T, D = q.shape
    out = torch.empty((B, T, H, D), dtype=q.dtype, device=q.device)
    lse = torch.empty((B, H, T), dtype=torch.float32, device=q.device) if want_lse else None
    if drop is not None and drop.p > 0.0:
        # attention_probs_dropout in the kernel (bf_attention_fwd_dropout); with want_keep the decisions come back as one
        # bit per probability ([B, H, T, T/32] int32) for bf_attention_bwd_dropout
        keep = torch.empty((B, H, T, T // 32), dtype=torch.int32, device=q.device) if want_keep else None
        _C.check(_C.lib().bf_attention_fwd_dropout(q.data_ptr(), k.data_ptr(), v.data_ptr(),
                                                   key_mask.data_ptr() if key_mask is not None else None,
                                                   mask_off.data_ptr() if mask_off is not None else None, out.data_ptr(),
                                                   lse.data_ptr() if lse is not None else None, _TORCH2BF[q.dtype], B, T, H,
                                                   D, H * D, float(scaling), drop.p, drop.seed, drop.call, drop.site,
                                                   drop.first_group(B, H * T * (T // 32) * 4),
                                                   keep.data_ptr() if keep is not None else None, drop.d_call, _stream_ptr()),
                 "bf_attention_fwd_dropout")
        res = (out,) + ((lse,) if want_lse else ()) + ((keep,) if want_keep else ())
        return res if len(res) > 1 else out
    _C.check(_C.lib().bf_attention_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(),
                                       key_mask.data_ptr() if key_mask is not None else None,
                                       mask_off.data_ptr() if mask_off is not None else None, out.data_ptr(),
                                       lse.data_ptr() if lse is not None else None,
                                       _TORCH2BF[q.dtype], B, T, H, D, H * D, float(scaling), _stream_ptr()),
             "bf_attention_fwd")
    return (out, lse) if want_lse else out


ATTENTION_MAX_Q_ROWS = 16


def attention_forward_rows(q: Tensor, k: Tensor, v: Tensor, key_mask: Optional[Tensor], scaling: float,
                           mask_off: Optional[Tensor] = None, q_rows: int = 1) -> Tensor:
    """attention_forward for the first `q_rows` (1 .. 16) queries of every (sequence, head) against all T keys and values
    (bf_attention_fwd_rows).  q, k, v, key_mask, mask_off as attention_forward takes them; returns the compact
    [B, q_rows, H, 64], bit for bit rows 0 .. q_rows - 1 of attention_forward's output."""
    B, H, T, D = q.shape
    if not 1 <= int(q_rows) <= ATTENTION_MAX_Q_ROWS:
        raise _C.BayeFormersAMDError(f"attention_forward_rows: q_rows={q_rows} (1 .. {ATTENTION_MAX_Q_ROWS})")
    out = torch.empty((B, int(q_rows), H, D), dtype=q.dtype, device=q.device)
    _C.check(_C.lib().bf_attention_fwd_rows(q.data_ptr(), k.data_ptr(), v.data_ptr(),
                                            key_mask.data_ptr() if key_mask is not None else None,
                                            mask_off.data_ptr() if mask_off is not None else None, out.data_ptr(),
                                            _TORCH2BF[q.dtype], B, T, H, D, H * D, int(q_rows), float(scaling),
                                            _stream_ptr()), "bf_attention_fwd_rows")
    ROWS_CALLS["attention"] += 1
    return out


def attention_backward(q: Tensor, k: Tensor, v: Tensor, key_mask: Optional[Tensor], mask_off: Optional[Tensor],
                       out: Tensor, grad_out: Tensor, lse: Tensor, scaling: float, drop_p: float = 0.0,
                       keep: Optional[Tensor] = None, colsum_samples: int = 0):
    """Gradients of attention_forward (bf_attention_bwd).  Returns (dq, dk, dv), each [B, T, H, 64] contiguous.
    colsum_samples = S (one-tile sequences, B % S == 0): the per-sample column sums of dq / dk / dv come out of the same
    launch (bf_attention_bwd_colsum) and are offered to the backward of the layers that produced q, k, v (offer_colsum)."""
    B, H, T, D = q.shape
    go = grad_out if (grad_out.dtype == q.dtype and grad_out.is_contiguous()) else grad_out.to(q.dtype).contiguous()
    # one buffer, three slabs: the gradients of a stacked query / key / value launch arrive as one [3, ...] tensor
    dqkv = torch.empty((3, B, T, H, D), dtype=q.dtype, device=q.device)
    dq, dk, dv = dqkv[0], dqkv[1], dqkv[2]
    delta = torch.empty((B, H, T), dtype=torch.float32, device=q.device)
    if colsum_samples > 0 and T == 128 and B % colsum_samples == 0 and not _NO_COLSUM_FOLD:
        S = int(colsum_samples)
        partial = workspace(q.device, B * H * 3 * D * 4)
        colsum = torch.empty((3, S, H * D), dtype=torch.float32, device=q.device)
        _C.check(_C.lib().bf_attention_bwd_colsum(q.data_ptr(), k.data_ptr(), v.data_ptr(),
                                                  key_mask.data_ptr() if key_mask is not None else None,
                                                  mask_off.data_ptr() if mask_off is not None else None, out.data_ptr(),
                                                  go.data_ptr(), lse.data_ptr(), delta.data_ptr(), dq.data_ptr(),
                                                  dk.data_ptr(), dv.data_ptr(), _TORCH2BF[q.dtype], B, T, H, D, H * D,
                                                  float(scaling), float(drop_p), keep.data_ptr() if drop_p > 0.0 else None,
                                                  S, partial.data_ptr(), colsum.data_ptr(), _stream_ptr()),
                 "bf_attention_bwd_colsum")
        for t, g in enumerate((dq, dk, dv)):
            offer_colsum(g, colsum[t])
        return dq, dk, dv
    if drop_p > 0.0:
        _C.check(_C.lib().bf_attention_bwd_dropout(q.data_ptr(), k.data_ptr(), v.data_ptr(),
                                                   key_mask.data_ptr() if key_mask is not None else None,
                                                   mask_off.data_ptr() if mask_off is not None else None, out.data_ptr(),
                                                   go.data_ptr(), lse.data_ptr(), delta.data_ptr(), dq.data_ptr(),
                                                   dk.data_ptr(), dv.data_ptr(), _TORCH2BF[q.dtype], B, T, H, D, H * D,
                                                   float(scaling), float(drop_p), keep.data_ptr(), _stream_ptr()),
                 "bf_attention_bwd_dropout")
        return dq, dk, dv
    _C.check(_C.lib().bf_attention_bwd(q.data_ptr(), k.data_ptr(), v.data_ptr(),
                                       key_mask.data_ptr() if key_mask is not None else None,
                                       mask_off.data_ptr() if mask_off is not None else None, out.data_ptr(),
                                       go.data_ptr(), lse.data_ptr(), delta.data_ptr(), dq.data_ptr(), dk.data_ptr(),
                                       dv.data_ptr(), _TORCH2BF[q.dtype], B, T, H, D, H * D, float(scaling),
                                       _stream_ptr()), "bf_attention_bwd")
    return dq, dk, dv


class AttentionFn(torch.autograd.Function):
    """bf_attention_fwd with bf_attention_bwd as its backward: nothing but q, k, v, the output and one fp32 row
    statistic per query is kept; the probabilities are recomputed in the backward kernels."""

    @staticmethod
    def forward(ctx, q, k, v, key_mask, mask_off, scaling, drop=None):
        ctx.drop_p = drop.p if drop is not None else 0.0
        fwd = bfr.STATE.ctx   # inside an S-sample forward: the backward also leaves dq / dk / dv's per-sample column sums
        ctx.cs_samples = fwd.S if fwd is not None else 0
        if ctx.drop_p > 0.0:  # training mode: probabilities dropped in the kernel, one keep bit each kept for the backward
            out, lse, keep = attention_forward(q, k, v, key_mask, scaling, mask_off, want_lse=True, drop=drop, want_keep=True)
            ctx.save_for_backward(q, k, v, out, lse, keep)
        else:
            out, lse = attention_forward(q, k, v, key_mask, scaling, mask_off, want_lse=True)
            ctx.save_for_backward(q, k, v, out, lse)
        ctx.key_mask, ctx.mask_off, ctx.scaling = key_mask, mask_off, scaling
        return out

    @staticmethod
    def backward(ctx, grad_out):
        q, k, v, out, lse = ctx.saved_tensors[:5]
        keep = ctx.saved_tensors[5] if ctx.drop_p > 0.0 else None
        dq, dk, dv = attention_backward(q, k, v, ctx.key_mask, ctx.mask_off, out, grad_out, lse, ctx.scaling, ctx.drop_p, keep,
                                        colsum_samples=ctx.cs_samples)
        # q, k, v came in as [B, H, T, 64] views of [B, T, H*64] projections: hand the gradients back in that view
        return dq.transpose(1, 2), dk.transpose(1, 2), dv.transpose(1, 2), None, None, None, None


# launches of the any-length encoder attention entries (include/bayeformers_amd_encoder_any.h) from this process: "fwd" of
# bf_attention_fwd_any / bf_attention_fwd_any_dropout, "bwd" of bf_attention_bwd_any / bf_attention_bwd_any_dropout, "rows"
# of bf_attention_fwd_any_rows
ENCODER_ANY_CALLS = {"fwd": 0, "bwd": 0, "rows": 0}


def attention_any_supported(q: Tensor, k: Tensor, v: Tensor) -> bool:
    """attention_supported's non-causal checks without the conditions on T (any T >= 1): what the bf_attention_*_any
    entries take — [B, H, T, 64] views of contiguous [B, T, H, 64] projections, bf16 or fp16, 16-byte aligned."""
    if not (q.is_cuda and q.dtype in (torch.bfloat16, torch.float16) and k.dtype == q.dtype and v.dtype == q.dtype):
        return False
    if q.dim() != 4 or q.shape != k.shape or q.shape != v.shape:
        return False
    B, H, T, D = q.shape
    if D != 64 or T < 1 or B < 1 or H < 1 or B > 65535 or H > 65535:
        return False
    st = (T * H * D, D, H * D, 1)  # BHTD view of a contiguous [B, T, H, D] tensor
    return all(t.stride() == st and t.data_ptr() % 16 == 0 for t in (q, k, v))


def _keep_words_any(T: int) -> int:
    """Keep words per query of the any-length entries: Tp / 32 with Tp = T rounded up to the key tile of 128."""
    return 4 * ((T + 127) // 128)


def attention_forward_any(q: Tensor, k: Tensor, v: Tensor, key_mask: Optional[Tensor], scaling: float,
                          mask_off: Optional[Tensor] = None, want_lse: bool = False, drop: Optional[Dropout] = None,
                          want_keep: bool = False):
    """attention_forward at any sequence length T >= 1 (bf_attention_fwd_any / bf_attention_fwd_any_dropout): operands as
    attention_any_supported describes them, key_mask additive fp32 [B, T] contiguous.  With want_keep the dropout
    decisions come back as [B, H, T, Tp/32] int32 words, Tp = T rounded up to 128.  At T % 128 == 0 the entries launch
    attention_forward's kernels: the same bits."""
    B, H, T, D = q.shape
    out = torch.empty((B, T, H, D), dtype=q.dtype, device=q.device)
    lse = torch.empty((B, H, T), dtype=torch.float32, device=q.device) if want_lse else None
    mask_ptr = key_mask.data_ptr() if key_mask is not None else None
    off_ptr = mask_off.data_ptr() if mask_off is not None else None
    lse_ptr = lse.data_ptr() if lse is not None else None
    if drop is not None and drop.p > 0.0:
        words = _keep_words_any(T)
        keep = torch.empty((B, H, T, words), dtype=torch.int32, device=q.device) if want_keep else None
        _C.check(_C.lib().bf_attention_fwd_any_dropout(q.data_ptr(), k.data_ptr(), v.data_ptr(), mask_ptr, off_ptr,
                                                       out.data_ptr(), lse_ptr, _TORCH2BF[q.dtype], B, T, H, D, H * D,
                                                       float(scaling), drop.p, drop.seed, drop.call, drop.site,
                                                       drop.first_group(B, H * T * words * 4),
                                                       keep.data_ptr() if keep is not None else None, drop.d_call,
                                                       _stream_ptr()), "bf_attention_fwd_any_dropout")
        ENCODER_ANY_CALLS["fwd"] += 1
        res = (out,) + ((lse,) if want_lse else ()) + ((keep,) if want_keep else ())
        return res if len(res) > 1 else out
    _C.check(_C.lib().bf_attention_fwd_any(q.data_ptr(), k.data_ptr(), v.data_ptr(), mask_ptr, off_ptr, out.data_ptr(),
                                           lse_ptr, _TORCH2BF[q.dtype], B, T, H, D, H * D, float(scaling), _stream_ptr()),
             "bf_attention_fwd_any")
    ENCODER_ANY_CALLS["fwd"] += 1
    return (out, lse) if want_lse else out


def attention_forward_rows_any(q: Tensor, k: Tensor, v: Tensor, key_mask: Optional[Tensor], scaling: float,
                               mask_off: Optional[Tensor] = None, q_rows: int = 1) -> Tensor:
    """attention_forward_rows at any sequence length T >= q_rows (bf_attention_fwd_any_rows): the compact
    [B, q_rows, H, 64], bit for bit rows 0 .. q_rows - 1 of attention_forward_any's output."""
    B, H, T, D = q.shape
    if not 1 <= int(q_rows) <= min(ATTENTION_MAX_Q_ROWS, T):
        raise _C.BayeFormersAMDError(f"attention_forward_rows_any: q_rows={q_rows} (1 .. {min(ATTENTION_MAX_Q_ROWS, T)})")
    out = torch.empty((B, int(q_rows), H, D), dtype=q.dtype, device=q.device)
    _C.check(_C.lib().bf_attention_fwd_any_rows(q.data_ptr(), k.data_ptr(), v.data_ptr(),
                                                key_mask.data_ptr() if key_mask is not None else None,
                                                mask_off.data_ptr() if mask_off is not None else None, out.data_ptr(),
                                                _TORCH2BF[q.dtype], B, T, H, D, H * D, int(q_rows), float(scaling),
                                                _stream_ptr()), "bf_attention_fwd_any_rows")
    ENCODER_ANY_CALLS["rows"] += 1
    return out


def attention_backward_any(q: Tensor, k: Tensor, v: Tensor, key_mask: Optional[Tensor], mask_off: Optional[Tensor],
                           out: Tensor, grad_out: Tensor, lse: Tensor, scaling: float, drop_p: float = 0.0,
                           keep: Optional[Tensor] = None):
    """Gradients of attention_forward_any (bf_attention_bwd_any / bf_attention_bwd_any_dropout).  Returns (dq, dk, dv), each
    [B, T, H, 64] contiguous; keep: the forward's [B, H, T, Tp/32] words.  No column-sum fold: that is a T = 128 launch."""
    B, H, T, D = q.shape
    go = grad_out if (grad_out.dtype == q.dtype and grad_out.is_contiguous()) else grad_out.to(q.dtype).contiguous()
    dqkv = torch.empty((3, B, T, H, D), dtype=q.dtype, device=q.device)
    dq, dk, dv = dqkv[0], dqkv[1], dqkv[2]
    delta = torch.empty((B, H, T), dtype=torch.float32, device=q.device)
    head = (q.data_ptr(), k.data_ptr(), v.data_ptr(), key_mask.data_ptr() if key_mask is not None else None,
            mask_off.data_ptr() if mask_off is not None else None, out.data_ptr(), go.data_ptr(), lse.data_ptr(),
            delta.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), _TORCH2BF[q.dtype], B, T, H, D, H * D,
            float(scaling))
    if drop_p > 0.0:
        _C.check(_C.lib().bf_attention_bwd_any_dropout(*head, float(drop_p), keep.data_ptr(), _stream_ptr()),
                 "bf_attention_bwd_any_dropout")
    else:
        _C.check(_C.lib().bf_attention_bwd_any(*head, _stream_ptr()), "bf_attention_bwd_any")
    ENCODER_ANY_CALLS["bwd"] += 1
    return dq, dk, dv


class AttentionAnyFn(torch.autograd.Function):
    """AttentionFn on the any-length entries: attention_forward_any with attention_backward_any as its backward; keeps
    q, k, v, the output, one fp32 row statistic per query and, with dropout, the [B, H, T, Tp/32] keep words."""

    @staticmethod
    def forward(ctx, q, k, v, key_mask, mask_off, scaling, drop=None):
        ctx.drop_p = drop.p if drop is not None else 0.0
        if ctx.drop_p > 0.0:
            out, lse, keep = attention_forward_any(q, k, v, key_mask, scaling, mask_off, want_lse=True, drop=drop,
                                                   want_keep=True)
            ctx.save_for_backward(q, k, v, out, lse, keep)
        else:
            out, lse = attention_forward_any(q, k, v, key_mask, scaling, mask_off, want_lse=True)
            ctx.save_for_backward(q, k, v, out, lse)
        ctx.key_mask, ctx.mask_off, ctx.scaling = key_mask, mask_off, scaling
        return out

    @staticmethod
    def backward(ctx, grad_out):
        q, k, v, out, lse = ctx.saved_tensors[:5]
        keep = ctx.saved_tensors[5] if ctx.drop_p > 0.0 else None
        dq, dk, dv = attention_backward_any(q, k, v, ctx.key_mask, ctx.mask_off, out, grad_out, lse, ctx.scaling, ctx.drop_p,
                                            keep)
        return dq.transpose(1, 2), dk.transpose(1, 2), dv.transpose(1, 2), None, None, None, None


def add_layernorm_backward(x: Tensor, residual: Optional[Tensor], gamma: Tensor, grad_out: Tensor, eps: float,
                           drop: Optional[Dropout] = None, grad_out2: Optional[Tensor] = None):
    """Gradients of add_layernorm (bf_add_layernorm_bwd): returns (dz, dgamma, dbeta); dz is the gradient of both x
    and residual, dgamma / dbeta are fp32.  With `drop` (bf_add_layernorm_dropout_bwd) returns (dz, dgamma, dbeta, dx):
    dz is the residual's gradient, dx = dz o keep / (1 - p) the dropped input's.  grad_out2: the gradient of the
    output's second consumer, added to grad_out inside the kernel (bf_add_layernorm_bwd_sum)."""
    N = x.shape[-1]
    x2 = x.reshape(-1, N)
    x2 = x2 if x2.is_contiguous() else x2.contiguous()
    r2 = None
    if residual is not None:
        r2 = residual.reshape(-1, N)
        r2 = r2 if r2.is_contiguous() else r2.contiguous()
    g2 = grad_out.reshape(-1, N)
    g2 = (g2 if g2.dtype == x.dtype else g2.to(x.dtype)).contiguous()
    dz = torch.empty_like(x2)
    dgb = torch.empty((2, N), dtype=torch.float32, device=x.device)  # one buffer: one cast for both in the caller
    dgamma, dbeta = dgb[0], dgb[1]
    lib = _C.lib()
    need = lib.bf_add_layernorm_bwd_workspace_bytes(x2.shape[0], N)
    ws = workspace(x.device, need)
    if grad_out2 is not None:
        h2 = grad_out2.reshape(-1, N)
        h2 = (h2 if h2.dtype == x.dtype else h2.to(x.dtype)).contiguous()
        dropping = drop is not None and drop.p > 0.0
        dx = torch.empty_like(x2) if dropping else None
        _C.check(lib.bf_add_layernorm_bwd_sum(x2.data_ptr(), r2.data_ptr() if r2 is not None else None, gamma.data_ptr(),
                                              _TORCH2BF[gamma.dtype], g2.data_ptr(), h2.data_ptr(), dz.data_ptr(),
                                              dx.data_ptr() if dropping else None, dgamma.data_ptr(), dbeta.data_ptr(),
                                              ws.data_ptr(), ws.numel(), _TORCH2BF[x.dtype], x2.shape[0], N, float(eps),
                                              drop.p if dropping else 0.0, drop.seed if dropping else 0,
                                              drop.call if dropping else 0, drop.site if dropping else 0,
                                              drop.first_group(x2.shape[0], N // 8) if dropping else 0,
                                              drop.d_call if dropping else None, _stream_ptr()),
                 "bf_add_layernorm_bwd_sum")
        return (dz.view(x.shape), dgamma, dbeta, dx.view(x.shape)) if dropping else (dz.view(x.shape), dgamma, dbeta)
    if drop is not None and drop.p > 0.0:
        dx = torch.empty_like(x2)
        _C.check(lib.bf_add_layernorm_dropout_bwd(x2.data_ptr(), r2.data_ptr() if r2 is not None else None, gamma.data_ptr(),
                                                  _TORCH2BF[gamma.dtype], g2.data_ptr(), dz.data_ptr(), dx.data_ptr(),
                                                  dgamma.data_ptr(), dbeta.data_ptr(), ws.data_ptr(), ws.numel(),
                                                  _TORCH2BF[x.dtype], x2.shape[0], N, float(eps), drop.p, drop.seed, drop.call,
                                                  drop.site, drop.first_group(x2.shape[0], N // 8), drop.d_call, _stream_ptr()),
                 "bf_add_layernorm_dropout_bwd")
        return dz.view(x.shape), dgamma, dbeta, dx.view(x.shape)
    _C.check(lib.bf_add_layernorm_bwd(x2.data_ptr(), r2.data_ptr() if r2 is not None else None, gamma.data_ptr(),
                                      _TORCH2BF[gamma.dtype], g2.data_ptr(), dz.data_ptr(), dgamma.data_ptr(),
                                      dbeta.data_ptr(), ws.data_ptr(), ws.numel(), _TORCH2BF[x.dtype], x2.shape[0], N,
                                      float(eps), _stream_ptr()), "bf_add_layernorm_bwd")
    return dz.view(x.shape), dgamma, dbeta


_NO_COLSUM_FOLD = False  # tests' reference path: every bias gradient's column sums by a pass of its own
_NO_TWIN = False  # tests' reference path: let autograd add the two consumers' gradients


class AddLayerNormFn(torch.autograd.Function):
    """LayerNorm(x + residual) * gamma + beta with both directions in the HIP kernels; nothing but the inputs is saved.

    twin=True returns the output TWICE — (y, an alias of y that shares its storage) — for the callers that know the output
    has two consumers (in a transformer layer: the next dense layer and the next residual connection).  Each consumer takes
    its own alias, so autograd hands backward() the two gradients separately and the kernel adds them on load
    (bf_add_layernorm_bwd_sum) instead of autograd adding them with an activation-sized pass of its own.  Whatever the
    graph looks like the result is the plain one: an alias nobody used has no gradient, further consumers of either alias
    are summed by autograd as always."""

    @staticmethod
    def forward(ctx, x, residual, gamma, beta, eps, drop=None, twin=False):
        ctx.eps, ctx.has_res = eps, residual is not None
        ctx.drop = drop if (drop is not None and drop.p > 0.0) else None
        ctx.save_for_backward(x, residual if residual is not None else x, gamma)
        y = add_layernorm(x, residual, gamma, beta, eps, ctx.drop)
        if twin:
            ctx.set_materialize_grads(False)  # an unused alias arrives as None, not as a tensor of zeros
            return y, y.detach()
        return y

    @staticmethod
    def backward(ctx, grad_out, grad_twin=None):
        x, residual, gamma = ctx.saved_tensors
        if grad_out is None:
            grad_out, grad_twin = grad_twin, None
        if grad_out is None:
            return None, None, None, None, None, None, None
        dx = None
        if ctx.drop is not None:  # the mask is regenerated from (seed, call, site): nothing was stored
            dz, dgamma, dbeta, dx = add_layernorm_backward(x, residual if ctx.has_res else None, gamma, grad_out, ctx.eps, ctx.drop,
                                                           grad_out2=grad_twin)
        else:
            dz, dgamma, dbeta = add_layernorm_backward(x, residual if ctx.has_res else None, gamma, grad_out, ctx.eps,
                                                       grad_out2=grad_twin)
        need = ctx.needs_input_grad
        if gamma.dtype != torch.float32 and (need[2] or need[3]):
            # dgamma and dbeta are the two rows of one fp32 buffer: cast them with one launch
            both = dgamma._base.to(gamma.dtype) if dgamma._base is not None else torch.stack((dgamma, dbeta)).to(gamma.dtype)
            dgamma, dbeta = both[0], both[1]
        return ((dx if dx is not None else dz) if need[0] else None, dz if (ctx.has_res and need[1]) else None,
                dgamma if need[2] else None, dbeta if need[3] else None, None, None, None)


def layernorm_supported(x: Tensor, residual: Optional[Tensor], ln) -> bool:
    n = x.shape[-1]
    return (x.is_cuda and x.dtype in (torch.bfloat16, torch.float16, torch.float32) and n % 8 == 0 and n <= 4096 and
            (residual is None or (residual.shape == x.shape and residual.dtype == x.dtype)) and
            ln.weight.dtype in (torch.float32, x.dtype) and ln.bias is not None and ln.bias.dtype == ln.weight.dtype)


# ------------------------------------------------------------------------------- decoder blocks: RMSNorm, RoPE, SwiGLU
# Twelve public ops over six bodies (_norm_forward, _norm_backward, _rope, _glu_forward, _glu_backward and the rotary
# predicate): the Llama / Mistral / Qwen2 ops are the Gemma 1 / 2 / 3 and Qwen3 ones with the first norm, the weight offset, the
# q / k gammas and head size 256 taken away; each keeps its own C entry and its own counter.
# launches of bf_add_rmsnorm / bf_rope_qk / bf_swiglu from this process (tests, diagnostics)
BLOCK_CALLS = {"rmsnorm": 0, "rope": 0, "swiglu": 0}


def rmsnorm_supported(x: Tensor, residual: Optional[Tensor], norm) -> bool:
    """Does bf_add_rmsnorm take x (and the residual) under `norm` (a module with `weight` [N])?"""
    return norm_add_rmsnorm_supported(x, None, residual, norm)


def _rows_of(t: Tensor, n: int) -> Tensor:
    t2 = t.reshape(-1, n)
    return t2 if t2.is_contiguous() and t2.data_ptr() % 16 == 0 else t2.clone(memory_format=torch.contiguous_format)


def _norm_forward(who: str, x: Tensor, gamma_pre: Optional[Tensor], residual: Optional[Tensor], gamma_out: Tensor,
                  eps_pre: float, eps_out: float, weight_offset: Optional[int], want_sum: bool):
    """The body of add_rmsnorm (weight_offset None: bf_add_rmsnorm, which has neither an offset nor a first norm) and of
    norm_add_rmsnorm (bf_norm_add_rmsnorm)."""
    _require_device(x, who + " input")
    N = x.shape[-1]
    x2 = _rows_of(x, N)
    r2 = None
    if residual is not None:
        if residual.shape != x.shape or residual.dtype != x.dtype:
            raise _C.BayeFormersAMDError(f"{who}: residual must match the input's shape and dtype")
        r2 = _rows_of(residual, N)
    if weight_offset is None:
        if gamma_out.dtype not in (torch.float32, x.dtype):
            raise _C.BayeFormersAMDError(f"{who}: gamma must be float32 or have the input's dtype")
    else:
        for g in (gamma_pre, gamma_out):
            if g is not None and (g.dtype != gamma_out.dtype or g.dtype not in (torch.float32, x.dtype) or g.numel() != N):
                raise _C.BayeFormersAMDError(f"{who}: the gammas must be [N], of one dtype: float32 or the input's")
    out = torch.empty_like(x2)
    changed = r2 is not None or gamma_pre is not None
    z = torch.empty_like(x2) if (want_sum and changed) else None
    if weight_offset is None:
        _C.check(_C.lib().bf_add_rmsnorm(x2.data_ptr(), r2.data_ptr() if r2 is not None else None, gamma_out.data_ptr(),
                                         _TORCH2BF[gamma_out.dtype], z.data_ptr() if z is not None else None, out.data_ptr(),
                                         _TORCH2BF[x.dtype], x2.shape[0], N, float(eps_out), _stream_ptr()), "bf_add_rmsnorm")
    else:
        _C.check(_C.lib().bf_norm_add_rmsnorm(
            x2.data_ptr(), gamma_pre.data_ptr() if gamma_pre is not None else None, r2.data_ptr() if r2 is not None else None,
            gamma_out.data_ptr(), _TORCH2BF[gamma_out.dtype], int(weight_offset), z.data_ptr() if z is not None else None,
            out.data_ptr(), _TORCH2BF[x.dtype], x2.shape[0], N, float(eps_pre), float(eps_out), _stream_ptr()),
            "bf_norm_add_rmsnorm")
    if z is not None:
        z = z.view(x.shape)
    elif want_sum and not changed:
        z = x
    return z, out.view(x.shape)


def add_rmsnorm(x: Tensor, residual: Optional[Tensor], gamma: Tensor, eps: float, want_sum: bool = True):
    """(z, y) with z = x + residual and y = z * rsqrt(mean(z^2) + eps) * gamma over the last axis, one pass
    (bf_add_rmsnorm).  z is bitwise torch's `residual + x`; residual None: z is x itself.  want_sum=False (or no
    residual): z is not written and None is returned in its place."""
    out = _norm_forward("add_rmsnorm", x, None, residual, gamma, eps, eps, None, want_sum)
    BLOCK_CALLS["rmsnorm"] += 1
    return out


def _rope_supported(q: Tensor, k: Tensor, cos: Tensor, sin: Tensor, gamma_q: Optional[Tensor], gamma_k: Optional[Tensor],
                    head_dims) -> bool:
    if not (q.is_cuda and q.dtype in _TORCH2BF and k.dtype == q.dtype and k.is_cuda and q.dim() == 4 and k.dim() == 4):
        return False
    B, H, T, D = q.shape
    if D not in head_dims or k.shape[0] != B or k.shape[2] != T or k.shape[3] != D or q.numel() == 0 or k.numel() == 0:
        return False
    if B * T * (H + k.shape[1]) * (D // 16) >= 2 ** 31:
        return False
    for c in (cos, sin):
        if not (c.is_cuda and c.dtype in (torch.float32, q.dtype) and c.dim() == 3 and c.shape[0] in (1, B)
                and tuple(c.shape[1:]) == (T, D) and c.is_contiguous() and c.data_ptr() % 16 == 0):
            return False
    if cos.shape != sin.shape or cos.dtype != sin.dtype:
        return False
    if gamma_q is not None or gamma_k is not None:
        gs = [g for g in (gamma_q, gamma_k) if g is not None]
        if not all(_gamma_ok(g, D, q.dtype) and g.dtype == gs[0].dtype for g in gs):
            return False
    return all(t.stride(3) == 1 and all(s >= 0 and s % 8 == 0 for s in t.stride()[:3]) and t.data_ptr() % 16 == 0
               for t in (q, k))


def rope_supported(q: Tensor, k: Tensor, cos: Tensor, sin: Tensor) -> bool:
    """q [B, H, T, D], k [B, Hkv, T, D] with a contiguous feature dimension of 64 or 128 and (batch, head, token) strides
    that are multiples of 8; cos / sin contiguous [1 or B, T, D] of q's dtype or fp32: what bf_rope_qk takes."""
    return _rope_supported(q, k, cos, sin, None, None, (64, 128))


def _rope(who: str, llama: bool, backward: bool, q: Tensor, k: Tensor, cos: Tensor, sin: Tensor, x_q: Optional[Tensor],
          x_k: Optional[Tensor], gamma_q: Optional[Tensor], gamma_k: Optional[Tensor], eps: float, weight_offset: int,
          inplace: bool):
    """The body of the four rotary ops: q / k are what is rotated (backward: the gradients of the rotated tensors), x_q / x_k
    the backward's forward inputs.  llama: bf_rope_qk[_bwd], else bf_qknorm_rope[_bwd].  Returns (q', k', dgamma_q,
    dgamma_k)."""
    _require_device(q, who + " input")
    if backward:
        q, k = _rope_grad(q, q), _rope_grad(k, q)
    if not _rope_supported(q, k, cos, sin, gamma_q, gamma_k, (64, 128) if llama else (64, 128, 256)):
        raise _C.BayeFormersAMDError(f"{who}: unsupported shapes, strides or dtypes "
                                     f"(see ops.{'rope_supported' if llama else 'qknorm_rope_supported'})")
    if backward:
        for g, x, like in ((gamma_q, x_q, q), (gamma_k, x_k, k)):
            if g is not None and (x is None or x.shape != like.shape or x.dtype != like.dtype or not x.is_cuda):
                raise _C.BayeFormersAMDError(f"{who}: a gamma needs the forward's input of the gradient's shape and dtype")
    B, H, T, D = q.shape
    Hkv = k.shape[1]
    if inplace:
        qo, ko = q, k
    else:
        qo = torch.empty((B, T, H, D), dtype=q.dtype, device=q.device).transpose(1, 2)
        ko = torch.empty((B, T, Hkv, D), dtype=k.dtype, device=k.device).transpose(1, 2)
    s = _C.bf_rope_t(B, T, H, Hkv, D, cos.shape[0])
    for name, t in (("q_stride", q), ("k_stride", k), ("q_out_stride", qo), ("k_out_stride", ko)):
        getattr(s, name)[:] = [t.stride(0), t.stride(1), t.stride(2)]
    lib = _C.lib()
    if llama:
        entry = "bf_rope_qk_bwd" if backward else "bf_rope_qk"
        _C.check(getattr(lib, entry)(q.data_ptr(), k.data_ptr(), cos.data_ptr(), sin.data_ptr(), _TORCH2BF[cos.dtype],
                                     qo.data_ptr(), ko.data_ptr(), _TORCH2BF[q.dtype], ctypes.byref(s), _stream_ptr()), entry)
        return qo, ko, None, None
    g = gamma_q if gamma_q is not None else gamma_k
    gdt = _TORCH2BF[g.dtype] if g is not None else _C.BF_DT_F32
    ptr = lambda t: t.data_ptr() if t is not None else None
    if not backward:
        _C.check(lib.bf_qknorm_rope(q.data_ptr(), k.data_ptr(), cos.data_ptr(), sin.data_ptr(), _TORCH2BF[cos.dtype],
                                    ptr(gamma_q), ptr(gamma_k), gdt, int(weight_offset), float(eps), qo.data_ptr(),
                                    ko.data_ptr(), _TORCH2BF[q.dtype], ctypes.byref(s), _stream_ptr()), "bf_qknorm_rope")
        return qo, ko, None, None
    xq = _bthd(x_q) if gamma_q is not None else None
    xk = _bthd(x_k) if gamma_k is not None else None
    dgq = torch.empty(D, dtype=torch.float32, device=q.device) if gamma_q is not None else None
    dgk = torch.empty(D, dtype=torch.float32, device=q.device) if gamma_k is not None else None
    nbytes = lib.bf_qknorm_rope_bwd_workspace_bytes(ctypes.byref(s), int(g is not None))
    ws = workspace(q.device, nbytes) if nbytes else None
    _C.check(lib.bf_qknorm_rope_bwd(q.data_ptr(), k.data_ptr(), ptr(xq), ptr(xk), cos.data_ptr(), sin.data_ptr(),
                                    _TORCH2BF[cos.dtype], ptr(gamma_q), ptr(gamma_k), gdt, int(weight_offset), float(eps),
                                    qo.data_ptr(), ko.data_ptr(), ptr(dgq), ptr(dgk), ptr(ws), ws.numel() if ws is not None else 0,
                                    _TORCH2BF[q.dtype], ctypes.byref(s), _stream_ptr()), "bf_qknorm_rope_bwd")
    return qo, ko, dgq, dgk


def rope_qk(q: Tensor, k: Tensor, cos: Tensor, sin: Tensor, inplace: bool = False):
    """(q', k') = (q cos + rotate_half(q) sin, k cos + rotate_half(k) sin), HF's apply_rotary_pos_emb, in one launch
    (bf_rope_qk).  Shapes as rope_supported describes.  inplace: q and k are overwritten and returned; else the results
    are new tensors laid out [B, T, heads, D] and returned as their [B, heads, T, D] views."""
    qo, ko, _, _ = _rope("rope_qk", True, False, q, k, cos, sin, None, None, None, None, 0.0, 0, inplace)
    BLOCK_CALLS["rope"] += 1
    return qo, ko


def swiglu_supported(gate: Tensor, up: Tensor) -> bool:
    """gate / up of one shape and dtype, [..., N] with N % 8 == 0, whose rows lie one fixed stride apart (a multiple of
    8 elements, 16-byte aligned): contiguous tensors and the two halves of a stacked [rows, 2N] buffer."""
    if not (gate.is_cuda and up.is_cuda and gate.dtype in _TORCH2BF and up.dtype == gate.dtype and gate.shape == up.shape
            and gate.dim() >= 1 and gate.shape[-1] % 8 == 0 and gate.numel() > 0):
        return False
    return all(_row_stride(t) is not None for t in (gate, up))


def _row_stride(t: Tensor) -> Optional[int]:
    """Element stride between the rows of t seen as [rows, N], None when the rows are not evenly spaced."""
    n = t.shape[-1]
    if t.stride(-1) != 1 or t.data_ptr() % 16:
        return None
    rs = want = None
    for size, stride in zip(reversed(t.shape[:-1]), reversed(t.stride()[:-1])):
        if size == 1:
            continue
        if rs is None:
            rs, want = stride, stride * size
        elif stride != want:
            return None
        else:
            want *= size
    if rs is None:  # a single row
        return n
    return rs if rs >= n and rs % 8 == 0 else None


def _glu_forward(who: str, gate: Tensor, up: Tensor) -> Tensor:
    """The body of swiglu and geglu: the entry is bf_<who>."""
    _require_device(gate, who + " input")
    if not swiglu_supported(gate, up):
        raise _C.BayeFormersAMDError(f"{who}: unsupported shapes, strides or dtypes (see ops.swiglu_supported)")
    N = gate.shape[-1]
    out = torch.empty(gate.shape, dtype=gate.dtype, device=gate.device)
    entry = "bf_" + who
    _C.check(getattr(_C.lib(), entry)(gate.data_ptr(), _row_stride(gate), up.data_ptr(), _row_stride(up), out.data_ptr(), N,
                                      _TORCH2BF[gate.dtype], gate.numel() // N, N, _stream_ptr()), entry)
    return out


def swiglu(gate: Tensor, up: Tensor) -> Tensor:
    """silu(gate) * up in one launch (bf_swiglu): one rounding, against the framework's two."""
    out = _glu_forward("swiglu", gate, up)
    BLOCK_CALLS["swiglu"] += 1
    return out


# ---- the Gemma 1 / 2 / 3 and Qwen3 siblings: norm -> add -> norm, q / k norm + RoPE, GeGLU
# launches of bf_norm_add_rmsnorm / bf_qknorm_rope / bf_geglu from this process (BLOCK_CALLS keeps its three keys)
FAMILY_BLOCK_CALLS = {"norm_add_norm": 0, "qknorm_rope": 0, "geglu": 0}


def _gamma_ok(w, n: int, dtype) -> bool:
    return (isinstance(w, Tensor) and w.is_cuda and w.dim() == 1 and w.shape[0] == n and w.dtype in (torch.float32, dtype)
            and w.is_contiguous() and w.data_ptr() % 16 == 0)


def norm_add_rmsnorm_supported(x: Tensor, pre, residual: Optional[Tensor], out_norm) -> bool:
    """Does bf_norm_add_rmsnorm take x (and the residual) under the norm modules `pre` (or None) and `out_norm` (modules
    with `weight` [N], of one dtype)?"""
    n = x.shape[-1]
    return (x.is_cuda and x.dtype in _TORCH2BF and x.dim() >= 1 and n % 8 == 0 and n <= 8192 and x.numel() > 0 and
            (residual is None or (residual.shape == x.shape and residual.dtype == x.dtype and residual.is_cuda)) and
            _gamma_ok(out_norm.weight, n, x.dtype) and
            (pre is None or (_gamma_ok(pre.weight, n, x.dtype) and pre.weight.dtype == out_norm.weight.dtype)))


def norm_add_rmsnorm(x: Tensor, gamma_pre: Optional[Tensor], residual: Optional[Tensor], gamma_out: Tensor,
                     eps_pre: float, eps_out: float, weight_offset: int = 1, want_sum: bool = True):
    """(z, y) of one pass (bf_norm_add_rmsnorm): u = x normalised under gamma_pre and rounded (x itself without one),
    z = residual + u rounded (u itself without a residual), y = z normalised under gamma_out; both norms multiply by
    (weight_offset + gamma): 1 for Gemma's modules, 0 for Llama's.  want_sum=False: z is not written and None is returned
    in its place; without gamma_pre and residual z is x itself."""
    out = _norm_forward("norm_add_rmsnorm", x, gamma_pre, residual, gamma_out, eps_pre, eps_out, int(weight_offset), want_sum)
    FAMILY_BLOCK_CALLS["norm_add_norm"] += 1
    return out


def qknorm_rope_supported(q: Tensor, k: Tensor, cos: Tensor, sin: Tensor, gamma_q: Optional[Tensor] = None,
                          gamma_k: Optional[Tensor] = None) -> bool:
    """rope_supported's layouts at head size 64, 128 or 256; the gammas (each may be None) [D] contiguous tensors of one
    dtype, q's or fp32: what bf_qknorm_rope takes."""
    return _rope_supported(q, k, cos, sin, gamma_q, gamma_k, (64, 128, 256))


def qknorm_rope(q: Tensor, k: Tensor, cos: Tensor, sin: Tensor, gamma_q: Optional[Tensor] = None,
                gamma_k: Optional[Tensor] = None, eps: float = 1e-6, weight_offset: int = 0, inplace: bool = False):
    """rope_qk at head size 64, 128 or 256 with an RMSNorm of every head in front of the rotation, in one launch
    (bf_qknorm_rope): n = x rsqrt(mean_D(x^2) + eps) (weight_offset + gamma) kept in fp32, then n cos + rotate_half(n) sin,
    rounded once.  A tensor whose gamma is None is only rotated.  Shapes as qknorm_rope_supported describes; inplace and
    the returned layouts as rope_qk's."""
    qo, ko, _, _ = _rope("qknorm_rope", False, False, q, k, cos, sin, None, None, gamma_q, gamma_k, eps, weight_offset, inplace)
    FAMILY_BLOCK_CALLS["qknorm_rope"] += 1
    return qo, ko


def geglu_supported(gate: Tensor, up: Tensor) -> bool:
    """What bf_geglu takes: what bf_swiglu takes (swiglu_supported)."""
    return swiglu_supported(gate, up)


def geglu(gate: Tensor, up: Tensor) -> Tensor:
    """gelu(gate, approximate="tanh") * up in one launch (bf_geglu): one rounding, against the framework's two."""
    out = _glu_forward("geglu", gate, up)
    FAMILY_BLOCK_CALLS["geglu"] += 1
    return out


# ---- their backward: bf_add_rmsnorm_bwd / bf_rope_qk_bwd / bf_swiglu_bwd, and the autograd functions over both directions
# launches of the three backward entries from this process (the forwards of a training step count in BLOCK_CALLS)
BLOCK_BWD_CALLS = {"rmsnorm": 0, "rope": 0, "swiglu": 0}


def rmsnorm_bwd_supported(x: Tensor, residual: Optional[Tensor], norm) -> bool:
    """Does bf_add_rmsnorm_bwd take what bf_add_rmsnorm took?  The same limits: N % 8 == 0, N <= 8192."""
    return rmsnorm_supported(x, residual, norm)


def _grad_rows(g: Tensor, like: Tensor, n: int) -> Tensor:
    return _rows_of(g if g.dtype == like.dtype else g.to(like.dtype), n)


def _norm_backward(who: str, x: Optional[Tensor], z: Tensor, gamma_pre: Optional[Tensor], gamma_out: Tensor,
                   grad_out: Optional[Tensor], eps_pre: float, eps_out: float, weight_offset: Optional[int],
                   grad_sum: Optional[Tensor], want_dz: bool):
    """The body of add_rmsnorm_backward (weight_offset None: bf_add_rmsnorm_bwd) and of norm_add_rmsnorm_backward
    (bf_norm_add_rmsnorm_bwd): (dx, dz, dgamma_pre, dgamma_out) as the latter describes them."""
    _require_device(z, who + " input")
    N = z.shape[-1]
    pre = gamma_pre is not None
    if weight_offset is None:
        if gamma_out.dtype not in (torch.float32, z.dtype):
            raise _C.BayeFormersAMDError(f"{who}: gamma must be float32 or have the input's dtype")
        if grad_out.shape != z.shape or (grad_sum is not None and grad_sum.shape != z.shape):
            raise _C.BayeFormersAMDError(f"{who}: the gradients must have the input's shape")
    else:
        if grad_out is None and grad_sum is None:
            raise _C.BayeFormersAMDError(f"{who}: no gradient")
        for g in (gamma_pre, gamma_out):
            if g is not None and (g.dtype != gamma_out.dtype or g.dtype not in (torch.float32, z.dtype) or g.numel() != N):
                raise _C.BayeFormersAMDError(f"{who}: the gammas must be [N], of one dtype: float32 or the input's")
        if any(t is not None and t.shape != z.shape for t in (grad_out, grad_sum, x if pre else None)):
            raise _C.BayeFormersAMDError(f"{who}: the gradients and x must have z's shape")
        if pre and (x is None or x.dtype != z.dtype):
            raise _C.BayeFormersAMDError(f"{who}: gamma_pre needs the forward's input x")
    z2 = _rows_of(z, N)
    g2 = _grad_rows(grad_out, z, N) if grad_out is not None else None
    h2 = _grad_rows(grad_sum, z, N) if grad_sum is not None else None
    dz = torch.empty_like(z2) if (want_dz or not pre) else None
    dg_out = torch.empty(N, dtype=torch.float32, device=z.device)
    lib = _C.lib()
    if weight_offset is None:
        ws = workspace(z.device, lib.bf_add_rmsnorm_bwd_workspace_bytes(z2.shape[0], N))
        _C.check(lib.bf_add_rmsnorm_bwd(z2.data_ptr(), gamma_out.data_ptr(), _TORCH2BF[gamma_out.dtype], g2.data_ptr(),
                                        h2.data_ptr() if h2 is not None else None, dz.data_ptr(), dg_out.data_ptr(),
                                        ws.data_ptr(), ws.numel(), _TORCH2BF[z.dtype], z2.shape[0], N, float(eps_out),
                                        _stream_ptr()), "bf_add_rmsnorm_bwd")
        dz = dz.view(z.shape)
        return dz, dz, None, dg_out
    x2 = _rows_of(x, N) if pre else None
    dx = torch.empty_like(z2) if pre else None
    dg_pre = torch.empty(N, dtype=torch.float32, device=z.device) if pre else None
    ptr = lambda t: t.data_ptr() if t is not None else None
    ws = workspace(z.device, lib.bf_norm_add_rmsnorm_bwd_workspace_bytes(z2.shape[0], N, int(pre)))
    _C.check(lib.bf_norm_add_rmsnorm_bwd(ptr(x2), z2.data_ptr(), ptr(gamma_pre), gamma_out.data_ptr(), _TORCH2BF[gamma_out.dtype],
                                         int(weight_offset), ptr(g2), ptr(h2), ptr(dz), ptr(dx), ptr(dg_pre), dg_out.data_ptr(),
                                         ws.data_ptr(), ws.numel(), _TORCH2BF[z.dtype], z2.shape[0], N, float(eps_pre),
                                         float(eps_out), _stream_ptr()), "bf_norm_add_rmsnorm_bwd")
    dz = dz.view(z.shape) if dz is not None else None
    return (dx.view(z.shape) if pre else dz), dz, dg_pre, dg_out


def add_rmsnorm_backward(z: Tensor, gamma: Tensor, grad_out: Tensor, eps: float, grad_sum: Optional[Tensor] = None):
    """Gradients of add_rmsnorm (bf_add_rmsnorm_bwd) from the sum z it returned (x itself without a residual): (dz,
    dgamma).  dz is the gradient of both x and the residual, dgamma is fp32.  grad_sum: the gradient that reached z
    through its other consumer, added to dz inside the kernel."""
    _, dz, _, dgamma = _norm_backward("add_rmsnorm_backward", None, z, None, gamma, grad_out, eps, eps, None, grad_sum, True)
    BLOCK_BWD_CALLS["rmsnorm"] += 1
    return dz, dgamma


class AddRMSNormFn(torch.autograd.Function):
    """add_rmsnorm with both directions in the HIP kernels.  With a residual it returns (z, y), the two outputs of one
    launch; backward receives their gradients separately and hands z's — the next residual add's, a returned hidden
    state's — to the kernel, which adds it on load.  Without a residual it returns y alone.  Saves z (an output, or x) and
    gamma, nothing else."""

    @staticmethod
    def forward(ctx, x, residual, gamma, eps):
        ctx.eps, ctx.has_res = eps, residual is not None
        z, y = add_rmsnorm(x, residual, gamma, eps)
        ctx.save_for_backward(z, gamma)
        ctx.set_materialize_grads(False)  # an output nobody used arrives as None, not as a tensor of zeros
        return (z, y) if ctx.has_res else y

    @staticmethod
    def backward(ctx, *grads):
        z, gamma = ctx.saved_tensors
        grad_z, grad_y = grads if ctx.has_res else (None, grads[0])
        need = ctx.needs_input_grad
        if grad_y is None:  # only the sum was used: the add's own backward
            return grad_z if need[0] else None, grad_z if need[1] else None, None, None
        dz, dgamma = add_rmsnorm_backward(z, gamma, grad_y, ctx.eps, grad_sum=grad_z)
        if need[2] and dgamma.dtype != gamma.dtype:
            dgamma = dgamma.to(gamma.dtype)  # the kernel emits fp32
        return dz if need[0] else None, dz if (ctx.has_res and need[1]) else None, dgamma if need[2] else None, None


def _rope_grad(g: Tensor, like: Tensor) -> Tensor:
    g = g if g.dtype == like.dtype else g.to(like.dtype)
    ok = g.stride(3) == 1 and all(s >= 0 and s % 8 == 0 for s in g.stride()[:3]) and g.data_ptr() % 16 == 0
    return g if ok else g.contiguous()


def rope_qk_backward(grad_q: Tensor, grad_k: Tensor, cos: Tensor, sin: Tensor):
    """Gradients of rope_qk (bf_rope_qk_bwd), its transpose: grad_q [B, H, T, D] / grad_k [B, Hkv, T, D] in any layout
    rope_supported takes (read where the attention backward left them) -> (dq, dk), new tensors laid out [B, T, heads, D]
    — what the backward of the projections reads — and returned as their [B, heads, T, D] views."""
    dq, dk, _, _ = _rope("rope_qk_backward", True, True, grad_q, grad_k, cos, sin, None, None, None, None, 0.0, 0, False)
    BLOCK_BWD_CALLS["rope"] += 1
    return dq, dk


class RopeQKFn(torch.autograd.Function):
    """rope_qk (out of place) with both directions in the HIP kernels; saves the two tables."""

    @staticmethod
    def forward(ctx, q, k, cos, sin):
        ctx.save_for_backward(cos, sin)
        return rope_qk(q, k, cos, sin)

    @staticmethod
    def backward(ctx, grad_q, grad_k):
        cos, sin = ctx.saved_tensors
        dq, dk = rope_qk_backward(grad_q, grad_k, cos, sin)
        return dq, dk, None, None


def swiglu_bwd_supported(gate: Tensor, up: Tensor) -> bool:
    """What bf_swiglu_bwd takes of the forward's inputs: what bf_swiglu took."""
    return swiglu_supported(gate, up)


def _glu_backward(who: str, gate: Tensor, up: Tensor, grad_out: Tensor, stacked: bool):
    """The body of swiglu_backward and geglu_backward: the entry is bf_<who>_bwd."""
    _require_device(gate, who + "_backward input")
    if not swiglu_supported(gate, up) or grad_out.shape != gate.shape:
        raise _C.BayeFormersAMDError(f"{who}_backward: unsupported shapes, strides or dtypes (see ops.swiglu_supported)")
    g = grad_out if grad_out.dtype == gate.dtype else grad_out.to(gate.dtype)
    if not g.is_cuda or _row_stride(g) is None:
        g = g.contiguous()
    N = gate.shape[-1]
    if stacked:
        both = torch.empty((*gate.shape[:-1], 2 * N), dtype=gate.dtype, device=gate.device)
        dgate, dup = both[..., :N], both[..., N:]
    else:
        dgate, dup = (torch.empty(gate.shape, dtype=gate.dtype, device=gate.device) for _ in range(2))
    entry = f"bf_{who}_bwd"
    _C.check(getattr(_C.lib(), entry)(gate.data_ptr(), _row_stride(gate), up.data_ptr(), _row_stride(up), g.data_ptr(),
                                      _row_stride(g), dgate.data_ptr(), 2 * N if stacked else N, dup.data_ptr(),
                                      2 * N if stacked else N, _TORCH2BF[gate.dtype], gate.numel() // N, N, _stream_ptr()),
             entry)
    return dgate, dup


def swiglu_backward(gate: Tensor, up: Tensor, grad_out: Tensor, stacked: bool = False):
    """Gradients of swiglu (bf_swiglu_bwd): (dgate, dup) from the forward's inputs.  stacked: the two are the halves of
    one [..., 2N] buffer (the layout a stacked gate / up projection's backward reads) instead of two tensors."""
    out = _glu_backward("swiglu", gate, up, grad_out, stacked)
    BLOCK_BWD_CALLS["swiglu"] += 1
    return out


class SwiGLUFn(torch.autograd.Function):
    """swiglu with both directions in the HIP kernels; saves gate and up (the projections' outputs), nothing new."""

    @staticmethod
    def forward(ctx, gate, up):
        ctx.save_for_backward(gate, up)
        return swiglu(gate, up)

    @staticmethod
    def backward(ctx, grad_out):
        gate, up = ctx.saved_tensors
        return swiglu_backward(gate, up, grad_out)


# ---- the backward of the Gemma / Qwen3 siblings: bf_norm_add_rmsnorm_bwd / bf_qknorm_rope_bwd / bf_geglu_bwd
# launches of the three backward entries from this process (the forwards of a training step count in FAMILY_BLOCK_CALLS)
FAMILY_BLOCK_BWD_CALLS = {"norm_add_norm": 0, "qknorm_rope": 0, "geglu": 0}


def norm_add_rmsnorm_backward(x: Optional[Tensor], z: Tensor, gamma_pre: Optional[Tensor], gamma_out: Tensor,
                              grad_out: Optional[Tensor], eps_pre: float, eps_out: float, weight_offset: int = 1,
                              grad_sum: Optional[Tensor] = None, want_dz: bool = True):
    """Gradients of norm_add_rmsnorm (bf_norm_add_rmsnorm_bwd) from the sum z it returned (x itself when nothing changed
    it) and, with gamma_pre, its input x: (dx, dz, dgamma_pre, dgamma_out).  dz is the gradient of the residual; without
    gamma_pre dx is dz and dgamma_pre None.  The dgammas are fp32.  grad_sum: the gradient that reached z through its
    other consumer, added inside the kernel; grad_out None: only the sum was consumed (dgamma_out is then zero).
    want_dz=False (with gamma_pre, no residual): dz is not written and None is returned in its place."""
    out = _norm_backward("norm_add_rmsnorm_backward", x, z, gamma_pre, gamma_out, grad_out, eps_pre, eps_out,
                         int(weight_offset), grad_sum, want_dz)
    FAMILY_BLOCK_BWD_CALLS["norm_add_norm"] += 1
    return out


class NormAddRMSNormFn(torch.autograd.Function):
    """norm_add_rmsnorm with both directions in the HIP kernels.  It returns (z, y), the two outputs of one launch, or y
    alone when z is x (no gamma_pre, no residual); backward receives their gradients separately and hands z's to the
    kernel, which adds it on load, as AddRMSNormFn does.  Saves x (only with gamma_pre), z (an output, or x) and the gammas."""

    @staticmethod
    def forward(ctx, x, gamma_pre, residual, gamma_out, eps_pre, eps_out, weight_offset):
        ctx.eps_pre, ctx.eps_out, ctx.woff = eps_pre, eps_out, weight_offset
        ctx.has_pre, ctx.has_res = gamma_pre is not None, residual is not None
        z, y = norm_add_rmsnorm(x, gamma_pre, residual, gamma_out, eps_pre, eps_out, weight_offset)
        ctx.save_for_backward(x if ctx.has_pre else None, z, gamma_pre, gamma_out)
        ctx.set_materialize_grads(False)  # an output nobody used arrives as None, not as a tensor of zeros
        return (z, y) if (ctx.has_pre or ctx.has_res) else y

    @staticmethod
    def backward(ctx, *grads):
        x, z, gamma_pre, gamma_out = ctx.saved_tensors
        grad_z, grad_y = grads if (ctx.has_pre or ctx.has_res) else (None, grads[0])
        need = ctx.needs_input_grad
        if grad_y is None and grad_z is None:
            return None, None, None, None, None, None, None
        if grad_y is None and not ctx.has_pre:  # only the sum was used: the add's own backward
            return grad_z if need[0] else None, None, grad_z if need[2] else None, None, None, None, None
        dx, dz, dg_pre, dg_out = norm_add_rmsnorm_backward(x, z, gamma_pre, gamma_out, grad_y, ctx.eps_pre, ctx.eps_out, ctx.woff,
                                                           grad_sum=grad_z, want_dz=ctx.has_res and need[2])
        if grad_y is None:
            dg_out = None  # the second norm's output was not used
        elif need[3] and dg_out.dtype != gamma_out.dtype:
            dg_out = dg_out.to(gamma_out.dtype)  # the kernel emits fp32
        if ctx.has_pre and need[1] and dg_pre.dtype != gamma_pre.dtype:
            dg_pre = dg_pre.to(gamma_pre.dtype)
        return (dx if need[0] else None, dg_pre if (ctx.has_pre and need[1]) else None,
                dz if (ctx.has_res and need[2]) else None, dg_out if need[3] else None, None, None, None)


def _bthd(t: Tensor) -> Tensor:
    """t [B, heads, T, D] laid out [B, T, heads, D] back to back (the projections' layout): t itself, or a copy."""
    if t.transpose(1, 2).is_contiguous() and t.data_ptr() % 16 == 0:
        return t
    return t.transpose(1, 2).contiguous().transpose(1, 2)


def qknorm_rope_backward(grad_q: Tensor, grad_k: Tensor, cos: Tensor, sin: Tensor, q: Optional[Tensor] = None,
                         k: Optional[Tensor] = None, gamma_q: Optional[Tensor] = None, gamma_k: Optional[Tensor] = None,
                         eps: float = 1e-6, weight_offset: int = 0):
    """Gradients of qknorm_rope (bf_qknorm_rope_bwd): grad_q [B, H, T, D] / grad_k [B, Hkv, T, D] in any layout
    qknorm_rope_supported takes (read where the attention backward left them) -> (dq, dk, dgamma_q, dgamma_k): dq / dk new
    tensors laid out [B, T, heads, D] — what the backward of the projections reads — returned as their [B, heads, T, D]
    views, the dgammas fp32 [D] (None for a tensor without a gamma).  q / k: the forward's inputs, needed for a tensor that
    has a gamma."""
    out = _rope("qknorm_rope_backward", False, True, grad_q, grad_k, cos, sin, q, k, gamma_q, gamma_k, eps, weight_offset, False)
    FAMILY_BLOCK_BWD_CALLS["qknorm_rope"] += 1
    return out


class QKNormRopeFn(torch.autograd.Function):
    """qknorm_rope (out of place) with both directions in the HIP kernels; saves the two tables, the gammas, and q / k only
    when a gamma is present."""

    @staticmethod
    def forward(ctx, q, k, cos, sin, gamma_q, gamma_k, eps, weight_offset):
        ctx.eps, ctx.woff = eps, weight_offset
        ctx.save_for_backward(cos, sin, gamma_q, gamma_k, q if gamma_q is not None else None, k if gamma_k is not None else None)
        return qknorm_rope(q, k, cos, sin, gamma_q, gamma_k, eps=eps, weight_offset=weight_offset)

    @staticmethod
    def backward(ctx, grad_q, grad_k):
        cos, sin, gamma_q, gamma_k, q, k = ctx.saved_tensors
        dq, dk, dgq, dgk = qknorm_rope_backward(grad_q, grad_k, cos, sin, q, k, gamma_q, gamma_k, ctx.eps, ctx.woff)
        need = ctx.needs_input_grad
        if dgq is not None and need[4] and dgq.dtype != gamma_q.dtype:
            dgq = dgq.to(gamma_q.dtype)  # the kernel emits fp32
        if dgk is not None and need[5] and dgk.dtype != gamma_k.dtype:
            dgk = dgk.to(gamma_k.dtype)
        return dq, dk, None, None, dgq if need[4] else None, dgk if need[5] else None, None, None


def geglu_backward(gate: Tensor, up: Tensor, grad_out: Tensor, stacked: bool = False):
    """Gradients of geglu (bf_geglu_bwd): (dgate, dup) from the forward's inputs; stacked as swiglu_backward's."""
    out = _glu_backward("geglu", gate, up, grad_out, stacked)
    FAMILY_BLOCK_BWD_CALLS["geglu"] += 1
    return out


class GeGLUFn(torch.autograd.Function):
    """geglu with both directions in the HIP kernels; saves gate and up (the projections' outputs), nothing new."""

    @staticmethod
    def forward(ctx, gate, up):
        ctx.save_for_backward(gate, up)
        return geglu(gate, up)

    @staticmethod
    def backward(ctx, grad_out):
        gate, up = ctx.saved_tensors
        return geglu_backward(gate, up, grad_out)


# ------------------------------------------------------------------------------------- Monte-Carlo predictive statistics
_PREDICTIVE_WS = {}


def predictive_layout(R: int, C: int, S_total: int, has_labels: bool):
    """(bytes, offsets) of the packed partials of bf_mc_predictive_partial: offsets = (sum_p, sum_h, sum_py, sum_logpy,
    counts, end) in bytes; sum_p / sum_h are fp32, the rest fp64 (starting at offsets[2], 8-byte aligned)."""
    offs = (ctypes.c_size_t * 6)()
    n = _C.lib().bf_mc_predictive_bytes(int(R), int(C), int(S_total), int(bool(has_labels)), offs)
    if n == 0:
        raise ValueError(f"predictive_layout: bad shape R={R} C={C} S_total={S_total}")
    return int(n), tuple(int(o) for o in offs)


def predictive_workspace(device: torch.device, S_total: int) -> Tensor:
    """Zero-filled workspace of the predictive kernels, one per (device, stream): the kernels leave it zeroed for the next
    launch (their tickets), so it is filled once, when it is allocated or grown.  It holds state between launches, so two
    launches must not use it at once.  Under a stream capture every call gets its own: every capture runs on the same
    capture stream, and two graphs replayed concurrently must not share tickets (the captured zero-fill then runs at the
    start of every replay)."""
    need = int(_C.lib().bf_mc_predictive_workspace_bytes(int(S_total)))
    if torch.cuda.is_current_stream_capturing():
        return torch.zeros(need, dtype=torch.uint8, device=device)
    key = (device.index if device.index is not None else torch.cuda.current_device(), _stream_ptr())
    ws = _PREDICTIVE_WS.get(key)
    if ws is None or ws.numel() < need:
        ws = torch.zeros(need, dtype=torch.uint8, device=device)
        _PREDICTIVE_WS[key] = ws
    return ws


def predictive_partial(logits: Tensor, labels: Optional[Tensor], ignore_index: int, sample_base: int, S_total: int,
                       partial: Tensor, ws: Tensor) -> Tensor:
    """bf_mc_predictive_partial of logits [S_local, R, C] (last dim contiguous) into the uint8 buffer `partial`."""
    _require_device(logits, "mc_predictive logits")
    S_local, R, C = logits.shape
    if logits.stride(2) != 1 and C > 1:
        raise ValueError("mc_predictive: the class dimension must be contiguous")
    _C.check(_C.lib().bf_mc_predictive_partial(
        logits.data_ptr(), _TORCH2BF[logits.dtype], logits.stride(0), logits.stride(1) if R > 1 else C, S_local, R, C,
        labels.data_ptr() if labels is not None else None, int(ignore_index), int(sample_base), int(S_total),
        partial.data_ptr(), ws.data_ptr(), ws.numel(), _stream_ptr()), "bf_mc_predictive_partial")
    return partial


def predictive_outputs(R: int, C: int, S_total: int, has_labels: bool, device) -> dict:
    """Fresh output tensors of bf_mc_predictive_finish."""
    f32 = dict(dtype=torch.float32, device=device)
    out = {"probs": torch.empty((R, C), **f32), "predictive_entropy": torch.empty(R, **f32),
           "expected_entropy": torch.empty(R, **f32), "mutual_information": torch.empty(R, **f32),
           "prediction": torch.empty(R, dtype=torch.int64, device=device)}
    if has_labels:
        out["log_likelihood"] = torch.empty(R, dtype=torch.float64, device=device)
        out["correct_per_sample"] = torch.empty(S_total, dtype=torch.int64, device=device)
        out["scalars"] = torch.empty(2, dtype=torch.float64, device=device)
        out["counts"] = torch.empty(2, dtype=torch.int64, device=device)
    return out


def predictive_finish(partial: Tensor, R: int, C: int, S_total: int, labels: Optional[Tensor], ignore_index: int,
                      out: dict, ws: Tensor) -> dict:
    """bf_mc_predictive_finish: complete partials -> the tensors of `out` (predictive_outputs)."""
    o = _C.bf_predictive_out_t()
    for name in ("probs", "predictive_entropy", "expected_entropy", "mutual_information", "prediction",
                 "log_likelihood", "correct_per_sample", "scalars", "counts"):
        t = out.get(name)
        setattr(o, "d_" + name, t.data_ptr() if t is not None else None)
    _C.check(_C.lib().bf_mc_predictive_finish(
        partial.data_ptr(), int(R), int(C), int(S_total), labels.data_ptr() if labels is not None else None,
        int(ignore_index), ctypes.byref(o), ws.data_ptr(), ws.numel(), _stream_ptr()), "bf_mc_predictive_finish")
    return out


# ------------------------------------------------------------------------------------------------- Bayesian LoRA
# bnn.LoRALinear (include/bayeformers_amd_lora.h): y[s] = x[s] W0^T + b0 + scale * (x[s] A_s^T) B^T on a frozen base.  The
# base products run on the GEMMs above with S = 1 — one stream over W0 for all samples — and bf_lora_fwd / bf_lora_bwd add the
# rank-r terms in place.  What lora_supported() refuses runs the same formula as framework ops on the same A_s.
LORA_MAX_RANK = 64
LORA_CALLS = {"fwd": 0, "bwd": 0, "composite_fwd": 0, "composite_bwd": 0, "base_skinny": 0, "base_gemm": 0}


def lora_kernel_wins(r: int, backward: bool) -> bool:
    """Where the kernels beat the framework composite on one MI355X (profiles/bayesian_lora.md; bf16, S 4, 4096 / 11008-wide
    layers, 8 .. 16384 rows, r 16 and 64): bf_lora_fwd at r = 16 (0.62-0.93x the composite's time from 4096 rows on, a tie
    within the spread below), not at r = 64 (1.3-2.0x from 4096 rows on); bf_lora_bwd nowhere yet (1.7-7.0x from 4096 rows on:
    its row contractions gather their operands element by element).  Ranks between the two measured ones go with the nearer."""
    return not backward and r <= 32


def lora_supported(dtype: torch.dtype, N: int, K: int, r: int, *tensors: Tensor, backward: Optional[bool] = None) -> bool:
    """Do bf_lora_fwd / bf_lora_bwd take this layer?  16-bit compute, K % 8 == 0, N % 8 == 0, r % 8 == 0 with
    8 <= r <= LORA_MAX_RANK; `tensors` (optional): the operands, each on a ROCm device, contiguous and 16-byte aligned.
    backward = False / True: also whether that direction's kernel is the faster route (lora_kernel_wins) — what
    lora_forward / lora_backward ask; None: the kernels' class alone.
    The one predicate that routes a call to the kernels or to the framework composite."""
    if dtype not in (torch.bfloat16, torch.float16) or K % 8 or N % 8 or r % 8 or not 8 <= r <= LORA_MAX_RANK:
        return False
    if backward is not None and not lora_kernel_wins(r, backward):
        return False
    return all(t is None or (t.is_cuda and t.is_contiguous() and t.data_ptr() % 16 == 0) for t in tensors)


def _lora_dims(x: Tensor, a_s: Tensor, b: Tensor, S: int):
    r, K = a_s.shape[-2], a_s.shape[-1]
    N = b.shape[0]
    rows = x.numel() // K
    if a_s.shape[0] != S or b.shape[1] != r or rows % S:
        raise _C.BayeFormersAMDError(f"lora: x {tuple(x.shape)}, A_s {tuple(a_s.shape)}, B {tuple(b.shape)} do not fit S={S}")
    return rows // S, N, K, r


def lora_fwd(x: Tensor, a_s: Tensor, b: Tensor, y: Optional[Tensor], scale: float, S: int) -> Tensor:
    """h = x A_s^T (returned, [S*M, r] of x's dtype) and y += scale * h B^T in place (bf_lora_fwd).  x: [S*M, K] 16-bit,
    a_s: [S, r, K] of the same dtype, b: [N, r] fp32, y: [S*M, N] of x's dtype or None.  Refusals raise."""
    _require_device(x, "x")
    M, N, K, r = _lora_dims(x, a_s, b, S)
    if a_s.dtype != x.dtype or b.dtype != torch.float32 or (y is not None and y.dtype != x.dtype):
        raise _C.BayeFormersAMDError("lora_fwd: A_s and y must have x's dtype, B must be fp32")
    if not all(t is None or t.is_contiguous() for t in (x, a_s, b, y)):
        raise _C.BayeFormersAMDError("lora_fwd: operands must be contiguous")
    h = torch.empty((S * M, r), dtype=x.dtype, device=x.device)
    _C.check(_C.lib().bf_lora_fwd(x.data_ptr(), a_s.data_ptr(), b.data_ptr(), y.data_ptr() if y is not None else None,
                                  h.data_ptr(), float(scale), _TORCH2BF.get(x.dtype, -1), S, M, N, K, r, None, 0, _stream_ptr()),
             "bf_lora_fwd")
    LORA_CALLS["fwd"] += 1
    return h


def lora_bwd(x: Tensor, dy: Tensor, a_s: Tensor, b: Tensor, h: Optional[Tensor], dx: Optional[Tensor], scale: float, S: int,
             need_db: bool = True):
    """(dA [S, r, K] fp32, dB [N, r] fp32 or None) and dx += scale * (dy B) A_s in place (bf_lora_bwd).  x: [S*M, K], dy: [S*M, N],
    h: what lora_fwd returned (needed for dB), dx: [S*M, K] holding dy W0, or None.  Refusals raise."""
    _require_device(x, "x")
    M, N, K, r = _lora_dims(x, a_s, b, S)
    if any(t is not None and t.dtype != x.dtype for t in (dy, a_s, h, dx)) or b.dtype != torch.float32:
        raise _C.BayeFormersAMDError("lora_bwd: dy, A_s, h and dx must have x's dtype, B must be fp32")
    if not all(t is None or t.is_contiguous() for t in (x, dy, a_s, b, h, dx)):
        raise _C.BayeFormersAMDError("lora_bwd: operands must be contiguous")
    if need_db and h is None:
        raise _C.BayeFormersAMDError("lora_bwd: dB needs the forward's h")
    lib = _C.lib()
    dt = _TORCH2BF.get(x.dtype, -1)
    da = torch.empty((S, r, K), dtype=torch.float32, device=x.device)
    db = torch.empty((N, r), dtype=torch.float32, device=x.device) if need_db else None
    need = lib.bf_lora_bwd_workspace_bytes(S, M, N, K, r, dt)
    ws = workspace(x.device, need)
    ptr = lambda t: t.data_ptr() if t is not None else None
    _C.check(lib.bf_lora_bwd(x.data_ptr(), dy.data_ptr(), a_s.data_ptr(), b.data_ptr(), ptr(h), ptr(dx), da.data_ptr(), ptr(db),
                             float(scale), dt, S, M, N, K, r, ws.data_ptr(), ws.numel(), _stream_ptr()), "bf_lora_bwd")
    LORA_CALLS["bwd"] += 1
    return da, db


def lora_reduce_da(da: Tensor, gaussian, stream_id: int, S: int, seed: int, sample_base: int, need_mu: bool = True):
    """(dmu_A or None, drho_A) from the per-sample gradients dA [S, r, K] fp32 (bf_lora_reduce_da): dmu = sum_s dA_s,
    drho = (sum_s dA_s o eps_s) o softplus'(rho), eps regenerated from the counter."""
    rho = gaussian.rho
    da = da.contiguous()
    dmu = torch.empty_like(rho, dtype=torch.float32) if need_mu else None
    drho = torch.empty_like(rho, dtype=torch.float32)
    _C.check(_C.lib().bf_lora_reduce_da(da.data_ptr(), rho.data_ptr(), rho.numel(), S, seed, sample_base & 0xFFFFFFFF,
                                        int(stream_id), dmu.data_ptr() if dmu is not None else None, drho.data_ptr(),
                                        _stream_ptr()), "bf_lora_reduce_da")
    return dmu, drho


def _gemm_nn_takes(dtype: torch.dtype, M: int, N: int, K: int) -> bool:
    # (bf_gemm_nn's own condition, restated: it fails rather than falls back)
    return dtype in (torch.bfloat16, torch.float16) and N % 64 == 0 and K % 8 == 0 and M * K >= 16384


def lora_base_forward(x: Tensor, w0: Tensor, bias32: Optional[Tensor]) -> Tensor:
    """x W0^T + b0 for ALL samples' rows as one product (S = 1): bf_gemm_nt_skinny up to SKINNY_ROWS rows (a decode step:
    W0 is streamed once whatever S is), the tiled GEMM otherwise.  x: [rows, K] 16-bit, w0: [N, K] of the same dtype,
    bias32: [1, N] fp32 or None."""
    rows, K = x.shape
    N = w0.shape[0]
    w = w0.view(1, N, K)
    if K % 32 == 0 and skinny_supported(x, w, 1, K):
        LORA_CALLS["base_skinny"] += 1
        return skinny_linear_forward(x, w, bias32, 1, N, K)
    LORA_CALLS["base_gemm"] += 1
    return gemm_nt(x, w, bias32, 1, rows, N, K, rows * K, x.dtype).view(rows, N)


def lora_forward(x: Tensor, a_s: Tensor, b: Tensor, w0: Tensor, b0: Optional[Tensor], scale: float, S: int,
                 bias32: Optional[Tensor] = None):
    """(y, h) of bnn.LoRALinear for S samples: y[s] = x[s] W0^T + b0 + scale * h[s] B^T, h[s] = x[s] A_s^T.  x: [S*M, K];
    a_s: [S, r, K] as ops.sample_logprob drew it; b: [N, r] fp32; w0: [N, K]; b0: [N] or None (bias32: its fp32 [1, N]
    copy, when the caller keeps one).  Kernels where lora_supported(), else the same formula as framework ops."""
    _require_device(x, "input")
    N, K, r = w0.shape[0], w0.shape[1], a_s.shape[1]
    x = x if x.is_contiguous() else x.contiguous()
    if a_s.dtype == x.dtype and w0.dtype == x.dtype and lora_supported(x.dtype, N, K, r, x, a_s, b, w0, backward=False):
        if b0 is not None and bias32 is None:
            bias32 = b0.detach().float().view(1, N)
        y = lora_base_forward(x, w0, bias32)
        h = lora_fwd(x, a_s, b, y, scale, S)
        return y, h
    LORA_CALLS["composite_fwd"] += 1
    M = x.shape[0] // S
    xd = x.dtype
    h = torch.bmm(x.view(S, M, K), a_s.to(xd).transpose(1, 2))
    y = torch.nn.functional.linear(x, w0.to(xd), b0.to(xd) if b0 is not None else None)
    y = torch.baddbmm(y.view(S, M, N), h, b.to(xd).t().expand(S, r, N), alpha=float(scale))
    return y.view(S * M, N), h.view(S * M, r)


def lora_backward(x: Tensor, dy: Tensor, a_s: Tensor, b: Tensor, h: Tensor, w0: Tensor, scale: float, S: int,
                  need_x: bool = True, need_b: bool = True):
    """(dx or None, dA [S, r, K] fp32, dB [N, r] fp32 or None) of lora_forward: g = dy B, dx = dy W0 + scale * g A_s,
    dA_s = scale * g[s]^T x[s], dB = scale * sum_s dy[s]^T h[s].  No gradient reaches W0."""
    N, K, r = w0.shape[0], w0.shape[1], a_s.shape[1]
    M = x.shape[0] // S
    dy = dy.reshape(S * M, N)
    dy = (dy if dy.dtype == x.dtype else dy.to(x.dtype)).contiguous()
    if a_s.dtype == x.dtype and w0.dtype == x.dtype and lora_supported(x.dtype, N, K, r, x, dy, a_s, b, h, w0, backward=True):
        dx = None
        if need_x:
            if _gemm_nn_takes(x.dtype, S * M, N, K):
                dx = gemm_nn(dy.view(1, S * M, N), w0.view(1, N, K)).view(S * M, K)
            else:
                dx = torch.matmul(dy, w0)
        da, db = lora_bwd(x, dy, a_s, b, h, dx, scale, S, need_b)
        return dx, da, db
    LORA_CALLS["composite_bwd"] += 1
    xd = x.dtype
    g = torch.matmul(dy.view(S, M, N), b.to(xd))
    dx = None
    if need_x:
        dx = torch.baddbmm(torch.matmul(dy, w0.to(xd)).view(S, M, K), g, a_s.to(xd), alpha=float(scale)).view(S * M, K)
    da = (float(scale) * torch.bmm(g.transpose(1, 2), x.view(S, M, K))).float()
    db = (float(scale) * torch.matmul(dy.t(), h.reshape(S * M, r))).float() if need_b else None
    return dx, da, db


# bnn.Linear with local = True (include/bayeformers_amd_lrt.h): the layer samples its pre-activations,
# y = act(m + sqrt(v) * zeta) with m = x mu^T + mu_b and v = x^2 (sigma^2)^T + sigma_b^2, instead of its weights.  The two
# products run on the GEMMs above with the sample axis used as the pair axis; the bf_lrt_* passes form their operands and
# combine their results.  What lrt_supported() refuses runs the same formula as framework ops on the same zeta.
LRT_CALLS = {"fwd": 0, "bwd": 0, "composite_fwd": 0, "composite_bwd": 0, "gemm_nn": 0, "gemm_tn": 0, "matmul": 0,
             "operands": 0, "kl": 0}
LRT_ONE_LAUNCH = True  # [m; v] as ONE bf_gemm_nt_act launch (S = 2, M = R) rather than two S = 1 launches (tools/lrt_bench.py)


def lrt_kernel_wins(N: int, K: int, rows: int, backward: bool) -> bool:
    """Where the kernel route beats the framework composite on one MI355X (profiles/local_reparameterization.md): every
    measured class, forward and backward — the composite runs the same two products and a chain of a dozen elementwise
    passes over the [rows, N] activations around them."""
    return True


def lrt_supported(dtype: torch.dtype, N: int, K: int, *tensors: Tensor, rows: int = 0, backward: Optional[bool] = None) -> bool:
    """Do the bf_lrt_* entries take this layer?  bf16 compute (in fp16 x^2 overflows above |x| = 256 and a MOPED sigma^2
    underflows), K % 8 == 0, N % 8 == 0; `tensors` (optional): the operands, each on a ROCm device, contiguous and 16-byte
    aligned.  backward = False / True: also whether that direction's kernels are the faster route (lrt_kernel_wins).
    The one predicate that routes a call to the kernels or to the framework composite."""
    if dtype != torch.bfloat16 or K % 8 or N % 8:
        return False
    if backward is not None and not lrt_kernel_wins(N, K, rows, backward):
        return False
    return all(t is None or (t.is_cuda and t.is_contiguous() and t.data_ptr() % 16 == 0) for t in tensors)


def _lrt_has_bias(layer) -> bool:
    from .nn.parameters.base import NoneParameter

    return not isinstance(layer.bias, NoneParameter)


def lrt_operands(layer, keep: bool = False):
    """(w2 [2, N, K] bf16 = [mu; sigma^2], b2 [2, N] fp32 = [mu_b; sigma_b^2] or None) of a layer (bf_lrt_operands).  Without
    gradients (keep) the pair is made once and kept on the layer, exactly as Linear.mean_weights keeps its copy (a new mu or
    rho — another address or version counter —, a later stale epoch or ops.invalidate_caches makes it again); a step that
    records gradients redoes it in its forward and in its backward: the optimizer moves the masters every step, and 2 N K
    16-bit values per layer are not held from one to the other."""
    mu, rho = layer.weight.mu, layer.weight.rho
    _require_device(mu, "mu")
    N, K = layer.out_features, layer.in_features
    has_bias = _lrt_has_bias(layer)
    key = None
    # (a forward being captured into a HIP graph makes the pair inside the graph: a replay after an optimizer step must read
    # the masters again, and a kept pair would be baked in by address)
    keep = keep and not torch.cuda.is_current_stream_capturing()
    if keep:
        key = (mu.device, mu.data_ptr(), mu._version, rho.data_ptr(), rho._version, bfr.STATE.stale_epoch)
        if has_bias:
            key += (layer.bias.mu.data_ptr(), layer.bias.mu._version, layer.bias.rho.data_ptr(), layer.bias.rho._version)
        hit = layer.__dict__.get("_mean_cache_lrt")
        if hit is not None and hit[0] == key:
            return hit[1], hit[2]
    with torch.inference_mode(False), torch.no_grad():
        w2 = torch.empty((2, N, K), dtype=torch.bfloat16, device=mu.device)
        b2 = torch.empty((2, N), dtype=torch.float32, device=mu.device) if has_bias else None
    if not (mu.is_contiguous() and rho.is_contiguous() and mu.dtype == torch.float32 and rho.dtype == torch.float32):
        raise _C.BayeFormersAMDError("mu/rho must be contiguous fp32 tensors")
    _C.check(_C.lib().bf_lrt_operands(mu.data_ptr(), rho.data_ptr(), layer.bias.mu.data_ptr() if has_bias else None,
                                      layer.bias.rho.data_ptr() if has_bias else None, w2.data_ptr(),
                                      b2.data_ptr() if has_bias else None, _C.BF_DT_BF16, N, K, _stream_ptr()), "bf_lrt_operands")
    LRT_CALLS["operands"] += 1
    if keep:
        layer.__dict__["_mean_cache_lrt"] = (key, w2, b2)
    return w2, b2


def lrt_square(x: Tensor, R_pad: int, pair: bool = True) -> Tensor:
    """xx [2, R_pad, K] bf16 with xx[1] = x^2 and (pair) xx[0] = x, rows past x's written as zeros (bf_lrt_square)."""
    R, K = x.shape
    xx = torch.empty((2, R_pad, K), dtype=x.dtype, device=x.device)
    _C.check(_C.lib().bf_lrt_square(x.data_ptr(), xx.data_ptr(), _TORCH2BF.get(x.dtype, -1), R, R_pad, K, int(pair), _stream_ptr()),
             "bf_lrt_square")
    return xx


def lrt_combine(m: Tensor, v: Tensor, S: int, seed: int, sample_base: int, layer_id: int, act: int = 0,
                want_pre: bool = False, want_sd: bool = False):
    """(y, pre or None, sqrt(v) or None), all [S*M, N] bf16, from the fp32 moments m, v [S*M, N] (bf_lrt_combine)."""
    R, N = m.shape
    y = torch.empty((R, N), dtype=torch.bfloat16, device=m.device)
    pre = torch.empty_like(y) if want_pre else None
    sd = torch.empty_like(y) if want_sd else None
    _C.check(_C.lib().bf_lrt_combine(m.data_ptr(), v.data_ptr(), y.data_ptr(), pre.data_ptr() if want_pre else None,
                                     sd.data_ptr() if want_sd else None, _C.BF_DT_BF16, S, R // S, N, int(act), seed,
                                     sample_base & 0xFFFFFFFF, int(layer_id), _stream_ptr()), "bf_lrt_combine")
    return y, pre, sd


def lrt_zeta(S: int, M: int, N: int, seed: int, sample_base: int, layer_id: int, device="cuda") -> Tensor:
    """zeta [S*M, N] fp32 of a local layer (bf_lrt_zeta): ops.philox_normal(M*N, S, seed, sample_base, BF_LRT_STREAM |
    layer_id) plus the device sample counter when one is set."""
    out = torch.empty((S * M, N), dtype=torch.float32, device=device)
    _C.check(_C.lib().bf_lrt_zeta(out.data_ptr(), S, M, N, seed, sample_base & 0xFFFFFFFF, int(layer_id), _stream_ptr()),
             "bf_lrt_zeta")
    return out


def lrt_grad_prepare(dy: Tensor, pre: Optional[Tensor], sd: Tensor, S: int, R_pad: int, seed: int, sample_base: int,
                     layer_id: int):
    """(dmdv [2, R_pad, N] bf16, colsum [2, N] fp32) from dy, sqrt(v) (and the pre-activation of a fused GELU), zeta
    regenerated (bf_lrt_grad_prepare)."""
    R, N = dy.shape
    lib = _C.lib()
    dmdv = torch.empty((2, R_pad, N), dtype=dy.dtype, device=dy.device)
    colsum = torch.empty((2, N), dtype=torch.float32, device=dy.device)
    need = lib.bf_lrt_grad_prepare_workspace_bytes(R_pad, N)
    ws = workspace(dy.device, need)
    _C.check(lib.bf_lrt_grad_prepare(dy.data_ptr(), pre.data_ptr() if pre is not None else None, sd.data_ptr(), dmdv.data_ptr(),
                                     colsum.data_ptr(), _TORCH2BF.get(dy.dtype, -1), S, R // S, R_pad, N,
                                     1 if pre is not None else 0, seed, sample_base & 0xFFFFFFFF, int(layer_id), ws.data_ptr(),
                                     ws.numel(), _stream_ptr()), "bf_lrt_grad_prepare")
    return dmdv, colsum


def lrt_dx(ab: Tensor, x: Tensor) -> Tensor:
    """dx = a + 2 x o b from ab [2, R_pad, K] and x [R, K] (bf_lrt_dx)."""
    R, K = x.shape
    dx = torch.empty_like(x)
    _C.check(_C.lib().bf_lrt_dx(ab.data_ptr(), ab.shape[1] * K, x.data_ptr(), dx.data_ptr(), _TORCH2BF.get(x.dtype, -1), R, K,
                                _stream_ptr()), "bf_lrt_dx")
    return dx


def lrt_drho(dsig2: Tensor, rho: Tensor) -> Tensor:
    """drho = dsigma^2 * 2 sigma sigmoid(rho) (bf_lrt_drho); fp32, any shape with a multiple of 4 elements."""
    drho = torch.empty_like(rho, dtype=torch.float32)
    _C.check(_C.lib().bf_lrt_drho(dsig2.data_ptr(), rho.data_ptr(), drho.data_ptr(), rho.numel(), _stream_ptr()), "bf_lrt_drho")
    return drho


def kl_gaussian(gaussian, prior) -> Tensor:
    """[2] float64 {E_q log p, E_q log q} of one Gaussian tensor under a Gaussian prior, in closed form (bf_kl_gaussian)."""
    mu, rho, pmu, prho = gaussian.mu, gaussian.rho, prior.mu, prior.rho
    _require_device(mu, "mu")
    if not all(t.is_cuda and t.is_contiguous() and t.dtype == torch.float32 and t.numel() == mu.numel() for t in (mu, rho, pmu, prho)):
        raise _C.BayeFormersAMDError("kl_gaussian: mu, rho and the prior's mu, rho must be contiguous fp32 tensors of one size "
                                     "on a ROCm device")
    lib = _C.lib()
    out = torch.empty(2, dtype=torch.float64, device=mu.device)
    ws = workspace(mu.device, lib.bf_kl_gaussian_workspace_bytes())
    _C.check(lib.bf_kl_gaussian(mu.data_ptr(), rho.data_ptr(), pmu.data_ptr(), prho.data_ptr(), mu.numel(), out.data_ptr(),
                                ws.data_ptr(), ws.numel(), _stream_ptr()), "bf_kl_gaussian")
    LRT_CALLS["kl"] += 1
    return out


def _lrt_pad(rows: int) -> int:
    return (rows + 63) // 64 * 64  # (bf_gemm_tn's contraction runs in steps of 64 rows)


def lrt_forward(layer, x: Tensor, S: int, seed: int, sample_base: int, act: int = 0, need_grad: bool = False):
    """(y, saved) of a local bnn.Linear for S samples: y[s] = act(m + sqrt(v) * zeta), x: [S*M, K].  `saved` is what
    lrt_backward needs (None unless need_grad): on the kernel route (xx [2, R_pad, K] = [x; x^2], sqrt(v), pre or None), on
    the composite route (x, sqrt(v), pre or None, zeta).  Kernels where lrt_supported(), else the same formula as framework
    ops — in x's dtype for bf16, in fp32 for fp16 and fp32 inputs."""
    _require_device(x, "input")
    N, K = layer.out_features, layer.in_features
    x = x if x.is_contiguous() else x.contiguous()
    R = x.shape[0]
    if R % S:
        raise _C.BayeFormersAMDError(f"input rows ({R}) are not a multiple of the sample count S={S}")
    M = R // S
    if lrt_supported(x.dtype, N, K, x, rows=R, backward=False) and layer.weight.mu.dtype == torch.float32:
        w2, b2 = lrt_operands(layer, keep=not need_grad)
        R_pad = _lrt_pad(R) if need_grad else R
        one = LRT_ONE_LAUNCH or need_grad
        xx = lrt_square(x, R_pad, pair=one)
        mv = torch.empty((2, R, N), dtype=torch.float32, device=x.device)
        if one:
            gemm_nt(xx, w2, b2, 2, R, N, K, R_pad * K, torch.float32, out=mv)
        else:
            gemm_nt(x, w2[0:1], b2[0:1] if b2 is not None else None, 1, R, N, K, R * K, torch.float32, out=mv[0:1])
            gemm_nt(xx[1], w2[1:2], b2[1:2] if b2 is not None else None, 1, R, N, K, R * K, torch.float32, out=mv[1:2])
        y, pre, sd = lrt_combine(mv[0], mv[1], S, seed, sample_base, layer.layer_id, act, want_pre=bool(act) and need_grad,
                                 want_sd=need_grad)
        LRT_CALLS["fwd"] += 1
        return y, ((xx, sd, pre) if need_grad else None)
    LRT_CALLS["composite_fwd"] += 1
    cd = x.dtype if x.dtype == torch.bfloat16 else torch.float32
    has_bias = _lrt_has_bias(layer)
    sig2 = torch.nn.functional.softplus(layer.weight.rho.detach().float()).square()
    xc = x.to(cd)
    m = torch.nn.functional.linear(xc, layer.weight.mu.detach().to(cd), layer.bias.mu.detach().to(cd) if has_bias else None)
    v = torch.nn.functional.linear(xc * xc, sig2.to(cd),
                                   torch.nn.functional.softplus(layer.bias.rho.detach().float()).square().to(cd) if has_bias else None)
    zeta = lrt_zeta(S, M, N, seed, sample_base, layer.layer_id, x.device)
    sd = torch.sqrt(torch.clamp_min(v, 0))
    pre = m + sd * zeta.to(cd)
    y = torch.nn.functional.gelu(pre) if act else pre
    return y.to(x.dtype), ((x, sd, pre if act else None, zeta) if need_grad else None)


def lrt_backward(layer, saved, dy: Tensor, S: int, seed: int, sample_base: int, need_x: bool = True, need_mu: bool = True,
                 need_mu_b: bool = True):
    """(dx, dmu, drho, dmu_b, drho_b) of lrt_forward, zeta a constant: dm = g, dv = g zeta / (2 sqrt(v)) (0 where v == 0),
    dx = dm mu + 2 x o (dv sigma^2), dmu = dm^T x, dsigma^2 = dv^T x^2, drho = dsigma^2 * 2 sigma sigmoid(rho) and the column
    sums for the bias.  Run it under the forward's counter (bfr.counter_override)."""
    N, K = layer.out_features, layer.in_features
    has_bias = _lrt_has_bias(layer)
    if len(saved) == 3:
        xx, sd, pre = saved
        R_pad = xx.shape[1]
        R = sd.shape[0]
        x = xx[0, :R]
        dy = dy.reshape(R, N)
        dy = (dy if dy.dtype == x.dtype else dy.to(x.dtype)).contiguous()
        dmdv, colsum = lrt_grad_prepare(dy, pre, sd, S, R_pad, seed, sample_base, layer.layer_id)
        w2, _ = lrt_operands(layer)
        dx = None
        if need_x:
            if _gemm_nn_takes(x.dtype, R_pad, N, K):
                ab = gemm_nn(dmdv, w2)
                LRT_CALLS["gemm_nn"] += 1
            else:
                ab = torch.bmm(dmdv, w2)
                LRT_CALLS["matmul"] += 1
            dx = lrt_dx(ab, x)
        dw = gemm_tn(dmdv, xx)  # [2, N, K] fp32: dmu, dsigma^2
        LRT_CALLS["gemm_tn"] += 1
        LRT_CALLS["bwd"] += 1
        dmu = dw[0] if need_mu else None
        drho = lrt_drho(dw[1], layer.weight.rho)
        dmu_b = drho_b = None
        if has_bias:
            dmu_b = colsum[0] if need_mu_b else None
            drho_b = lrt_drho(colsum[1], layer.bias.rho)
        return dx, dmu, drho, dmu_b, drho_b
    LRT_CALLS["composite_bwd"] += 1
    x, sd, pre, zeta = saved
    cd = sd.dtype
    R = x.shape[0]
    g = dy.reshape(R, N).to(cd)
    if pre is not None:
        pf = pre.float()
        g = (g.float() * (0.5 * torch.erfc(-pf * 0.7071067811865476) + pf * torch.exp(-0.5 * pf * pf) * 0.3989422804014327)).to(cd)
    dv = torch.where(sd > 0, g * zeta.to(cd) / (2 * sd), torch.zeros_like(g))
    xc = x.to(cd)
    rho = layer.weight.rho.detach().float()
    sigma = torch.nn.functional.softplus(rho)
    dx = None
    if need_x:
        dx = (torch.matmul(g, layer.weight.mu.detach().to(cd)) + 2 * xc * torch.matmul(dv, sigma.square().to(cd))).to(x.dtype)
    dmu = torch.matmul(g.t(), xc).float() if need_mu else None
    drho = torch.matmul(dv.t(), xc * xc).float() * (2 * sigma * torch.sigmoid(rho))
    dmu_b = drho_b = None
    if has_bias:
        rho_b = layer.bias.rho.detach().float()
        dmu_b = g.float().sum(0) if need_mu_b else None
        drho_b = dv.float().sum(0) * (2 * torch.nn.functional.softplus(rho_b) * torch.sigmoid(rho_b))
    return dx, dmu, drho, dmu_b, drho_b


# ------------------------------------------------------------------------------------------- Bayesian mixture of experts
# bnn.Experts (include/bayeformers_amd_moe.h): every (sample, expert) pair has weight matrices of its own, so the layer is a
# grouped GEMM over S * E groups whose sizes the router decides.  bf_moe_route lays the slots out by group on the device (no
# host round trip: the launches have a fixed grid, so a decode step with such a layer can be graph-captured), bf_moe_gate_up
# and bf_moe_down run the two products over the tile table, bf_moe_combine adds a row's k results.  What moe_supported()
# refuses runs moe_composite, the framework's loop per (sample, expert) on the same sampled weights — it waits for the
# device, so such a call cannot be captured.
MOE_TILE_ROWS, MOE_MAX_TOPK, MOE_MAX_GROUPS = _C.BF_MOE_TILE_ROWS, _C.BF_MOE_MAX_TOPK, _C.BF_MOE_MAX_GROUPS
MOE_CALLS = {"route": 0, "gate_up": 0, "down": 0, "combine": 0, "composite_fwd": 0, "composite_bwd": 0, "sample": 0}


def moe_is_silu(act) -> bool:
    """Is `act` (an experts module's act_fn, or a name) SiLU — the one activation bf_moe_gate_up applies?"""
    if isinstance(act, str):
        return act in ("silu", "swish")
    return (act is torch.nn.functional.silu or isinstance(act, torch.nn.SiLU)
            or (act.__class__.__name__ == "SiLUActivation" and not list(act.parameters())))


MOE_KERNEL_ROWS_PER_GROUP = 128


def moe_kernel_wins(S: int, E: int, k: int, rows: int) -> bool:
    """Where the kernel route beats the framework loop on one MI355X, eager (profiles/bayesian_moe.md; bf16, S 4): by the rows
    a (sample, expert) group holds on average, rows * k / (S * E).  Measured wins: decode steps (at most one row per group:
    0.33x the loop's time on a Mixtral-shaped layer, 0.02x on a Qwen3-MoE-shaped one) and 64 rows per group (Qwen3-MoE-shaped
    prefill, 0.07x: the loop is bound by its 7717 launches).  Measured loss: 256 rows per group (Mixtral-shaped prefill, 4.3x):
    every 16-row tile streams its group's weights again, where the loop's per-expert GEMMs are tiled.  Sizes between the two go
    with the nearer in ratio: up to MOE_KERNEL_ROWS_PER_GROUP rows per group the kernels.  A capturing stream never asks:
    the loop cannot be captured."""
    return rows * k <= MOE_KERNEL_ROWS_PER_GROUP * S * E


def moe_supported(dtype: torch.dtype, H: int, I: int, E: int, k: int, act, *tensors: Tensor, S: int = 1,
                  rows: Optional[int] = None) -> bool:
    """Do the bf_moe_* entries take this layer?  16-bit compute, H % 8 == 0, I % 8 == 0, SiLU, 1 <= k <= MOE_MAX_TOPK,
    S * E <= MOE_MAX_GROUPS; `tensors` (optional): the operands, each on a ROCm device, contiguous and 16-byte aligned.
    rows (optional): also whether the kernels are the faster route for that many rows (moe_kernel_wins) — what moe_forward
    asks outside a graph capture; None: the kernels' class alone.
    The one predicate that routes a call to the kernels or to the framework composite."""
    if dtype not in (torch.bfloat16, torch.float16) or H < 8 or I < 8 or H % 8 or I % 8 or not moe_is_silu(act):
        return False
    if not 1 <= k <= MOE_MAX_TOPK or E < 1 or S < 1 or S * E > MOE_MAX_GROUPS:
        return False
    if rows is not None and not moe_kernel_wins(S, E, k, rows) and not (
            torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()):
        return False
    return all(t is None or (t.is_cuda and t.is_contiguous() and t.data_ptr() % 16 == 0) for t in tensors)


def moe_max_tiles(S: int, E: int, R: int, k: int) -> int:
    """Tiles the grouped GEMMs are launched with: R*k / MOE_TILE_ROWS + min(S*E, R*k), known without the routing."""
    return (R * k) // MOE_TILE_ROWS + min(S * E, R * k)


def moe_route(top_k_index: Tensor, S: int, E: int):
    """(offsets [S*E + 1], slots [R*k], tiles [max_tiles, 3]) int32 of bf_moe_route for top_k_index [R, k] int64: the slots
    (row * k + j) sorted by group s * E + index, stable; an index equal to E is dropped.  slots past offsets[-1] and nothing
    else are left unwritten.  Nothing is read back to the host."""
    _require_device(top_k_index, "top_k_index")
    if top_k_index.dim() != 2 or top_k_index.dtype != torch.int64 or not top_k_index.is_contiguous():
        raise _C.BayeFormersAMDError("moe_route: top_k_index must be a contiguous [R, k] int64 tensor")
    R, k = top_k_index.shape
    dev = top_k_index.device
    lib = _C.lib()
    offsets = torch.empty(max(S * E, 0) + 1, dtype=torch.int32, device=dev)
    slots = torch.empty(R * k, dtype=torch.int32, device=dev)
    tiles = torch.empty((moe_max_tiles(S, E, R, k), 3), dtype=torch.int32, device=dev)
    need = lib.bf_moe_route_workspace_bytes(S, E, R, k)
    ws = workspace(dev, need)
    _C.check(lib.bf_moe_route(top_k_index.data_ptr(), offsets.data_ptr(), slots.data_ptr(), tiles.data_ptr(), S, E, R, k,
                              ws.data_ptr(), ws.numel(), _stream_ptr()), "bf_moe_route")
    MOE_CALLS["route"] += 1
    return offsets, slots, tiles


def _moe_dims(w_gu: Tensor, w_d: Optional[Tensor] = None):
    if w_gu.dim() != 4 or w_gu.shape[2] % 2 or (w_d is not None and (
            w_d.dim() != 4 or w_d.shape[:2] != w_gu.shape[:2] or w_d.shape[2] != w_gu.shape[3]
            or 2 * w_d.shape[3] != w_gu.shape[2])):
        raise _C.BayeFormersAMDError(f"moe: w_gu {tuple(w_gu.shape)} must be [S, E, 2I, H]"
                                     + (f" and w_d {tuple(w_d.shape)} [S, E, H, I]" if w_d is not None else ""))
    S, E, I2, H = w_gu.shape
    return S, E, H, I2 // 2


def moe_gate_up(x: Tensor, w_gu: Tensor, route, k: int) -> Tensor:
    """h [R*k, I] of x's dtype: h[slot] = silu(gate) * up with [gate | up] = x[slot // k] w_gu[s, e]^T (bf_moe_gate_up).
    x: [R, H] 16-bit, w_gu: [S, E, 2I, H] of the same dtype, route: what moe_route returned.  Rows of dropped slots are not
    written.  Refusals raise."""
    _require_device(x, "x")
    S, E, H, I = _moe_dims(w_gu)
    _, slots, tiles = route
    if x.dim() != 2 or x.shape[1] != H or w_gu.dtype != x.dtype:
        raise _C.BayeFormersAMDError(f"bf_moe_gate_up: x {tuple(x.shape)} {x.dtype} must be [R, H={H}] of w_gu's dtype "
                                     f"{w_gu.dtype} (16-bit compute)")
    if not (x.is_contiguous() and w_gu.is_contiguous()):
        raise _C.BayeFormersAMDError("bf_moe_gate_up: operands must be contiguous")
    R = x.shape[0]
    if slots.numel() != R * k or tiles.shape[0] != moe_max_tiles(S, E, R, k):
        raise _C.BayeFormersAMDError("bf_moe_gate_up: the route was made for another problem")
    h = torch.empty((R * k, I), dtype=x.dtype, device=x.device)
    _C.check(_C.lib().bf_moe_gate_up(x.data_ptr(), w_gu.data_ptr(), slots.data_ptr(), tiles.data_ptr(), h.data_ptr(),
                                     _TORCH2BF.get(x.dtype, -1), S, E, R, k, H, I, None, 0, _stream_ptr()), "bf_moe_gate_up")
    MOE_CALLS["gate_up"] += 1
    return h


def moe_down(h: Tensor, w_d: Tensor, route, k: int) -> Tensor:
    """y [R, k, H] fp32: y[r, j] = h[r * k + j] w_d[s, e]^T (bf_moe_down).  h: [R*k, I] 16-bit, w_d: [S, E, H, I] of the same
    dtype.  Rows of dropped slots are not written.  Refusals raise."""
    _require_device(h, "h")
    if w_d.dim() != 4:
        raise _C.BayeFormersAMDError(f"bf_moe_down: w_d {tuple(w_d.shape)} must be [S, E, H, I]")
    S, E, H, I = w_d.shape
    _, slots, tiles = route
    if h.dim() != 2 or h.shape[1] != I or h.shape[0] % k or w_d.dtype != h.dtype:
        raise _C.BayeFormersAMDError(f"bf_moe_down: h {tuple(h.shape)} {h.dtype} must be [R*k, I={I}] of w_d's dtype "
                                     f"{w_d.dtype} (16-bit compute)")
    if not (h.is_contiguous() and w_d.is_contiguous()):
        raise _C.BayeFormersAMDError("bf_moe_down: operands must be contiguous")
    R = h.shape[0] // k
    if slots.numel() != R * k or tiles.shape[0] != moe_max_tiles(S, E, R, k):
        raise _C.BayeFormersAMDError("bf_moe_down: the route was made for another problem")
    y = torch.empty((R, k, H), dtype=torch.float32, device=h.device)
    _C.check(_C.lib().bf_moe_down(h.data_ptr(), w_d.data_ptr(), slots.data_ptr(), tiles.data_ptr(), y.data_ptr(),
                                  _TORCH2BF.get(h.dtype, -1), S, E, R, k, H, I, None, 0, _stream_ptr()), "bf_moe_down")
    MOE_CALLS["down"] += 1
    return y


def moe_combine(y: Tensor, top_k_index: Tensor, top_k_weights: Tensor, E: int, dtype: torch.dtype) -> Tensor:
    """out [R, H] of `dtype`: out[r] = sum_j top_k_weights[r, j] * y[r, j] in j order, in fp32, rounded once; slots whose
    index is not an expert (E: dropped) count as zero (bf_moe_combine).  top_k_weights: fp32 or `dtype`."""
    _require_device(y, "y")
    if y.dim() != 3 or y.dtype != torch.float32 or top_k_index.shape != y.shape[:2] or top_k_weights.shape != y.shape[:2]:
        raise _C.BayeFormersAMDError("bf_moe_combine: y must be [R, k, H] fp32, top_k_index and top_k_weights [R, k]")
    if top_k_index.dtype != torch.int64:
        raise _C.BayeFormersAMDError("bf_moe_combine: top_k_index must be int64")
    if not (y.is_contiguous() and top_k_index.is_contiguous() and top_k_weights.is_contiguous()):
        raise _C.BayeFormersAMDError("bf_moe_combine: operands must be contiguous")
    R, k, H = y.shape
    out = torch.empty((R, H), dtype=dtype, device=y.device)
    _C.check(_C.lib().bf_moe_combine(y.data_ptr(), top_k_index.data_ptr(), top_k_weights.data_ptr(),
                                     _TORCH2BF.get(top_k_weights.dtype, -1), out.data_ptr(), _TORCH2BF.get(dtype, -1), E, R, k, H,
                                     None, 0, _stream_ptr()), "bf_moe_combine")
    MOE_CALLS["combine"] += 1
    return out


def moe_composite(x: Tensor, top_k_index: Tensor, top_k_weights: Tensor, w_gu: Tensor, w_d: Tensor, S: int, act) -> Tensor:
    """The framework's expert loop (transformers' `*Experts.forward`) once per sample on that sample's weights: for every
    expert that was hit, gather its rows, two F.linear calls around act(gate) * up, scale by the routing weight, index_add.
    Differentiable in x, top_k_weights, w_gu and w_d — the backward of bnn.Experts runs it under autograd — and the route of
    every call the kernels do not take.  It reads the hit experts back to the host: it cannot be graph-captured."""
    R, H = x.shape
    M = R // S
    E = w_gu.shape[1]
    if w_gu.dtype != x.dtype:
        w_gu, w_d = w_gu.to(x.dtype), w_d.to(x.dtype)
    outs = []
    for s in range(S):
        xs, ids, ws = x[s * M:(s + 1) * M], top_k_index[s * M:(s + 1) * M], top_k_weights[s * M:(s + 1) * M]
        out = torch.zeros_like(xs)
        for e in torch.unique(ids).tolist():
            if not 0 <= e < E:
                continue  # (E: the dropped-slot sentinel)
            tok, pos = torch.where(ids == e)
            gate, up = torch.nn.functional.linear(xs[tok], w_gu[s, e]).chunk(2, dim=-1)
            cur = torch.nn.functional.linear(act(gate) * up, w_d[s, e]) * ws[tok, pos, None]
            out = out.index_add(0, tok, cur.to(out.dtype))
        outs.append(out)
    return torch.cat(outs) if S > 1 else outs[0]


def moe_forward(x: Tensor, top_k_index: Tensor, top_k_weights: Tensor, w_gu: Tensor, w_d: Tensor, S: int, act) -> Tensor:
    """out [R, H] of bnn.Experts for S samples on the sampled weights w_gu [S, E, 2I, H] and w_d [S, E, H, I] (as
    ops.sample_logprob drew them): four entries — route, gate_up, down, combine — where moe_supported(), else moe_composite.
    While a graph is being captured an unsupported call raises: the composite waits for the device."""
    _require_device(x, "hidden_states")
    _, E, H, I = _moe_dims(w_gu, w_d)
    R, k = top_k_index.shape
    x = x if x.is_contiguous() else x.contiguous()
    idx = top_k_index if top_k_index.is_contiguous() else top_k_index.contiguous()
    wts = top_k_weights if top_k_weights.is_contiguous() else top_k_weights.contiguous()
    if (w_gu.dtype == x.dtype and w_d.dtype == x.dtype and idx.dtype == torch.int64 and wts.dtype in (torch.float32, x.dtype)
            and moe_supported(x.dtype, H, I, E, k, act, x, w_gu, w_d, S=S, rows=R)):
        route = moe_route(idx, S, E)
        h = moe_gate_up(x, w_gu, route, k)
        y = moe_down(h, w_d, route, k)
        return moe_combine(y, idx, wts, E, x.dtype)
    if torch.cuda.is_current_stream_capturing():
        raise _C.BayeFormersAMDError(
            f"moe_forward: this call is outside the bf_moe_* kernels' class (dtype {x.dtype}, H={H}, I={I}, E={E}, k={k}, S={S}, "
            f"act {act.__class__.__name__}) and the framework loop that serves it waits for the device: it cannot be captured")
    MOE_CALLS["composite_fwd"] += 1
    return moe_composite(x, idx, wts, w_gu, w_d, S, act)


def moe_backward(x: Tensor, dy: Tensor, top_k_index: Tensor, top_k_weights: Tensor, w_gu: Tensor, w_d: Tensor, S: int, act,
                 need_x: bool = True, need_wts: bool = True, need_w: bool = True):
    """(dx, d top_k_weights, dW_gu [S, E, 2I, H] fp32, dW_d [S, E, H, I] fp32) of moe_forward — each None when not needed — by
    autograd through moe_composite on the saved x, the sampled weights and the routing.  (Backward kernels: not yet.)"""
    MOE_CALLS["composite_bwd"] += 1
    with torch.enable_grad():
        xd = x.detach().requires_grad_(need_x)
        wt = top_k_weights.detach().requires_grad_(need_wts)
        gu = w_gu.detach().requires_grad_(need_w)
        dn = w_d.detach().requires_grad_(need_w)
        out = moe_composite(xd, top_k_index, wt, gu, dn, S, act)
        wanted = [t for t, need in ((xd, need_x), (wt, need_wts), (gu, need_w), (dn, need_w)) if need]
        grads = list(torch.autograd.grad(out, wanted, dy.reshape(out.shape).to(out.dtype), allow_unused=True))
    res = []
    for t, need in ((xd, need_x), (wt, need_wts), (gu, need_w), (dn, need_w)):
        g = grads.pop(0) if need else None
        res.append(torch.zeros_like(t) if need and g is None else g)
    dx, dwt, dgu, ddn = res
    return dx, dwt, dgu.float() if dgu is not None else None, ddn.float() if ddn is not None else None


def reduce_param_grad(dw: Tensor, gaussian, stream_id: int, S: int, seed: int, sample_base: int, need_mu: bool = True):
    """(dmu or None, drho) of one Gaussian from its per-sample weight gradients dw [S, *shape] fp32: dmu = sum_s dw_s,
    drho = (sum_s dw_s o eps_s) o softplus'(rho), eps regenerated from the counter (bf_launch_param_grad — what
    lora_reduce_da does for LoRA's dA, here for any sampled tensor: the two expert tensors of bnn.Experts)."""
    return lora_reduce_da(dw.reshape(S, -1), gaussian, stream_id, S, seed, sample_base, need_mu)
