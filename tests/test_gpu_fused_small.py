"""The single-kernel small-M linear path (csrc/bf_fused_small.hip) against the fp64 oracle.

One launch draws epsilon, forms W = mu + softplus(rho) * eps in registers, feeds the MFMA, samples the bias and sums both
log-probs: no other kernel produces y AND the log-probs from nothing but parameters.  Every case here proves which kernel it
launched with the library's own launch counters (bf_profile_*), never by mirroring the dispatch rule; the references are the
oracle's fp64 restatements (bo.eps_tensor, bo.gaussian_sample, bo.linear_logprobs_f64, bo.linear_logprob_magnitudes), computed
on the device in torch double.  No tolerance is new:

  * y, EVERY element      tol[y dtype] * max|ref| + 1e-5 sqrt(K), tol = 1e-5 / 2^-8 / 2^-11 (test_gemm_nt_against_torch), against
                          x_q W_s^T + b_s in fp64 with the device's own W_s (ops.sample_logprob) and x_q = x rounded to the
                          compute dtype — sharp enough for one dropped or duplicated product, a permuted k, a clamped row
                          written to the wrong m;
  * log_prior, log_q      LOGPROB_RTOL = 2e-6 of the oracle's sum of |terms| (test_fp32_path_matches_reference);
  * W_s (fp32)            4e-6 sigma + 1e-7 |W| against bo.gaussian_sample (test_sampled_weights_match_oracle) — ties the y
                          check to the oracle and not to another kernel of ours.

The grid walks the kernel's dispatch: templates MB = 1, 2, 3, 4, 6, 8 (M = 1 .. 128, with the 5 -> 6 and 7 -> 8 roundings and
a ragged last row block in each), the 4- and 8-wave K split (idle waves at K = 32 / 64 / 96, 5 slices on 4 waves at K = 160,
17 slices on 8 waves at K = 544), the scalar store and bias tail (N % 4 != 0), the partial last feature block (N % 16 != 0),
16-bit and fp32 inputs, every built-in prior kind, S = 1 .. 64, the sample counter's wrap and its device-resident mode.
"""
import contextlib
import ctypes
import functools

import numpy as np
import pytest
import torch

import bayeformers_amd as bf
import bayeformers_amd.nn as bnn
from bayeformers_amd import _C, ops
from bayeformers_amd import random as bfr
from oracle import bayes_oracle as bo
from util import SEED, run_layer

pytestmark = pytest.mark.gpu

LOGPROB_RTOL = 2e-6      # relative to sum|terms| (tests/test_gpu_linear.py)
Y_TOL = {torch.float32: 1e-5, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
CDT = {"bf16": torch.bfloat16, "fp16": torch.float16}
SMALL_M = [1, 6, 16, 17, 32, 33, 48, 49, 64]
WIDE_M = [65, 80, 81, 96, 97, 112, 113, 128]        # only layers of at most 512 x 512 weights run these fused
# (compute dtype, x is 16-bit): with a 16-bit x the output is 16-bit too
COMBOS = [("bf16", False), ("fp16", True), ("bf16", True), ("fp16", False)]


def template_of(M):
    """Label of the printed ratios only (the witness is the launch counter): the MB the kernel is instantiated with."""
    mb = (M + 15) // 16
    return {5: 6, 7: 8}.get(mb, mb)


def _process_state():
    lib = _C.lib()
    return (lib.bf_fused_small_max_rows(), bfr.STATE.device_counter is None, lib.bf_get_sample_counter(),
            bfr.get_compute_dtype())


@pytest.fixture(scope="module", autouse=True)
def process_state_left_as_found():
    """The row cap, the device-counter mode and the compute dtype are process-global: as found, after the whole file.
    (Profiling has no getter: every `launches()` block switches it off in its `finally`.)"""
    before = _process_state()
    yield
    assert _process_state() == before


# ------------------------------------------------------------------------------------------------ the witness
def _launch_counts():
    lib, n, out = _C.lib(), ctypes.c_uint64(0), {}
    for name, kind in (("fused", _C.BF_PROF_FUSED_SMALL), ("sample", _C.BF_PROF_SAMPLE), ("gemm", _C.BF_PROF_GEMM)):
        _C.check(lib.bf_profile_read(kind, ctypes.byref(n), None, None), "bf_profile_read")
        out[name] = int(n.value)
    return out


@contextlib.contextmanager
def launches():
    """Counts the library's launches inside the block into the dict it yields (filled when the block ends)."""
    lib = _C.lib()
    counts = {}
    _C.check(lib.bf_profile_enable(1), "bf_profile_enable")
    try:
        _C.check(lib.bf_profile_reset(), "bf_profile_reset")
        yield counts
        counts.update(_launch_counts())
    finally:
        lib.bf_profile_reset()
        lib.bf_profile_enable(0)


def assert_fused(counts, what=""):
    assert counts == {"fused": 1, "sample": 0, "gemm": 0}, (what, counts)


def assert_two_launch(counts, what=""):
    assert counts["fused"] == 0 and counts["sample"] >= 1 and counts["gemm"] >= 1, (what, counts)


def fused_run(layer, x, S, base, what=""):
    with launches() as c:
        y, lp = run_layer(layer, x, S, base)
    assert_fused(c, what)
    return y, lp


@contextlib.contextmanager
def compute_dtype(name):
    prev = bfr.get_compute_dtype()
    bf.set_compute_dtype(name)
    try:
        yield CDT[name]
    finally:
        bf.set_compute_dtype(prev)


@contextlib.contextmanager
def fused_rows_capped(rows):
    """bf_set_fused_small_max_rows is process-global: read first, restore, check that it is back."""
    lib = _C.lib()
    prev = lib.bf_fused_small_max_rows()
    _C.check(lib.bf_set_fused_small_max_rows(rows), "bf_set_fused_small_max_rows")
    try:
        yield
    finally:
        _C.check(lib.bf_set_fused_small_max_rows(prev), "bf_set_fused_small_max_rows")
        assert lib.bf_fused_small_max_rows() == prev


# ------------------------------------------------------------------------------------------------ layers from seeds
@functools.lru_cache(maxsize=8)
def layer_of(N, K, bias, prior):
    """mixture: the default scale mixture; custom: another mixture; gaussian: a general Gaussian prior next to a trainable
    mean (never aliased); moped / moped_trainable: from_frequentist(delta=0.05) with a frozen / a trainable mean."""
    torch.manual_seed(N * 10007 + K * 13 + 7)
    if prior == "mixture":
        layer = bnn.Linear(K, N, bias=bias)
    elif prior == "custom":
        layer = bnn.Linear(K, N, bias=bias, prior=bnn.ScaledGaussianMixture(0.25, 0.75, 0.1))
    elif prior == "gaussian":
        layer = bnn.Linear(K, N, bias=bias)
        priors = []
        for shape in ((N, K), (N,)):
            p = bnn.Gaussian(torch.Size(shape))
            with torch.no_grad():
                p.mu.uniform_(-0.3, 0.3)
                p.rho.uniform_(-2.0, 1.0)
            priors.append(p)
        layer.weight_prior = priors[0]
        if bias:
            layer.bias_prior = priors[1]
    else:
        freq = torch.nn.Linear(K, N, bias=bias)
        with torch.no_grad():
            freq.weight.normal_(0.0, 0.05)
            if bias:
                freq.bias.normal_(0.0, 0.05)
        layer = bnn.Linear.from_frequentist(freq, delta=0.05, freeze=prior == "moped")
    layer.layer_id = 0
    layer = layer.cuda()
    if prior == "moped":          # the frozen mean under its own MOPED prior
        assert ops.prior_alias(layer.weight, layer.weight_prior) is not None
    elif prior in ("gaussian", "moped_trainable"):
        assert ops.prior_alias(layer.weight, layer.weight_prior) is None
    return layer


def has_bias(layer):
    return isinstance(layer.bias, bnn.Gaussian)


def oracle_prior(prior):
    if isinstance(prior, bnn.ScaledGaussianMixture):
        return ("mixture", float(prior.pi), float(prior.sigma1), float(prior.sigma2))
    if isinstance(prior, bnn.Gaussian):
        return ("gaussian", prior.mu.detach(), prior.rho.detach())
    return None


def make_input(M, K, cdt=None):
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(1000 + M)).cuda()
    return x if cdt is None else x.to(cdt)


# ------------------------------------------------------------------------------------------------ the references
class Reference:
    """What the checks need of one (layer, S, base) and that depends neither on M nor on the dtypes: the device's own sampled
    weights and bias, and per sample the oracle's fp64 log-probs with their magnitudes.  Building it IS check C: every
    sample's fp32 W_s (and b_s) against bo.gaussian_sample of the oracle's epsilon in fp64, every element."""

    def __init__(self, layer, S, base):
        self.layer, self.S, self.base = layer, S, base
        N, K = layer.weight.mu.shape
        t = lambda p: p.detach()
        params = [(layer.weight, layer.weight_prior, 0, (N, K))]
        if has_bias(layer):
            params.append((layer.bias, layer.bias_prior, 1, (N,)))
        outs, _ = ops.sample_logprob([p[0] for p in params], [p[1] for p in params], [p[2] for p in params], S, SEED, base,
                                     out_dtype=torch.float32)
        self.b = outs[1].double() if has_bias(layer) else None
        self._w16 = {}
        pw, pb = oracle_prior(layer.weight_prior), oracle_prior(layer.bias_prior)
        self.lp64, self.mags, self.w_ratio = [], [], 0.0
        for s in range(S):
            idx = (base + s) & 0xFFFFFFFF
            eps = [bo.eps_tensor(shape, SEED, idx, 0, tid).cuda() for _, _, tid, shape in params] + [None]
            mu_b, rho_b = (t(layer.bias.mu), t(layer.bias.rho)) if has_bias(layer) else (None, None)
            args = (t(layer.weight.mu), t(layer.weight.rho), mu_b, rho_b, eps[0], eps[1], pw, pb)
            self.lp64.append(bo.linear_logprobs_f64(*args))
            self.mags.append(bo.linear_logprob_magnitudes(*args))
            for (g, _, tid, _), e in zip(params, eps):
                mu, rho = t(g.mu).double(), t(g.rho).double()
                want = bo.gaussian_sample(mu, rho, e.double())
                ratio = ((outs[tid][s].double() - want).abs() / (4e-6 * bo.sigma(rho) + 1e-7 * want.abs())).max().item()
                assert ratio <= 1.0, ("sampled values against the oracle: max err / bound", N, K, "bias" if tid else "weight", s, ratio)
                self.w_ratio = max(self.w_ratio, ratio)

    def w16(self, cdt):
        """[S, N, K] fp64 copy of the sampling kernel's weights in the compute dtype: the operand the MFMA must have seen."""
        if cdt not in self._w16:
            lw = self.layer
            w = ops.sample_logprob([lw.weight], [lw.weight_prior], [0], self.S, SEED, self.base, out_dtype=cdt)[0][0]
            self._w16[cdt] = w.double()
        return self._w16[cdt]

    def y(self, x, cdt):
        ref = torch.einsum("mk,snk->smn", x.to(cdt).double(), self.w16(cdt))
        return ref + self.b[:, None, :] if self.b is not None else ref

    def check_logprobs(self, lp, what):
        """Worst |got - fp64| / (LOGPROB_RTOL * magnitude) over the samples and both columns; asserts it is <= 1."""
        lp = lp.cpu().numpy()
        assert lp.shape == (self.S, 2)
        worst = 0.0
        for s in range(self.S):
            for col in (0, 1):
                want, mag = self.lp64[s][col], self.mags[s][col]
                assert np.isfinite(want) and np.isfinite(lp[s, col]), (what, s, col, want, lp[s, col])
                ratio = abs(lp[s, col] - want) / (LOGPROB_RTOL * mag)
                assert ratio <= 1.0, (what, "sample", s, "log_prior" if col == 0 else "log_q", lp[s, col], want, mag, ratio)
                worst = max(worst, ratio)
        return worst


@functools.lru_cache(maxsize=2)
def reference_of(N, K, bias, prior, S, base):
    return Reference(layer_of(N, K, bias, prior), S, base)


def y_ratio(y, ref, K):
    """max |y - ref| / bound over EVERY output, bound = tol[y dtype] * max|ref| + 1e-5 sqrt(K)."""
    bound = Y_TOL[y.dtype] * ref.abs().max().item() + 1e-5 * np.sqrt(K)
    assert y.shape == ref.shape and bool(torch.isfinite(y).all())
    return (y.double() - ref).abs().max().item() / bound


def check_case(ref, M, cdt_name, x16, what):
    """Checks A and B of one grid point through run_layer; returns (y ratio, log-prob ratio)."""
    layer, S, base = ref.layer, ref.S, ref.base
    N, K = layer.weight.mu.shape
    with compute_dtype(cdt_name) as cdt:
        x = make_input(M, K, cdt if x16 else None)
        y, lp = fused_run(layer, x, S, base, what)
        assert y.dtype == x.dtype and y.shape == (S, M, N)
        ry = y_ratio(y, ref.y(x, cdt), K)
        assert ry <= 1.0, (what, "y: max err / bound", ry)
        rl = ref.check_logprobs(lp, what)
    return ry, rl


# ------------------------------------------------------------------------------------------------ 2. the dispatch grid
# (N, K, bias, prior, S, base): every K of {32, 64, 96, 160, 512, 544, 768, 3072}, every N of {1, 2, 7, 33, 24, 200, 64, 512,
# 768, 3072}, each prior kind with and without bias, S = 1, 3, 64 and the wave splits:
#   4 waves — K < 512, and K >= 512 with ceil(N/16) * S >= 2048: 512 x 512 at S = 64 (32 * 64), 3072 x 768 at S = 11 (192 * 11);
#   8 waves — K >= 512 otherwise; 512 x 512 at S = 3 and M = 128 is MB = 8 on 8 waves, the largest LDS footprint.
GRID = [
    (1, 32, True, "mixture", 3, 10),
    (33, 32, False, "gaussian", 3, 11),
    (7, 64, True, "gaussian", 64, 500),
    (24, 96, False, "mixture", 3, 12),
    (33, 160, True, "custom", 3, 13),
    (200, 160, True, "moped", 1, 14),
    (512, 512, True, "mixture", 3, 15),
    (512, 512, True, "mixture", 64, 2000),
    (200, 544, True, "gaussian", 1, 16),
    (7, 544, False, "custom", 3, 17),
    (2, 768, True, "moped", 3, 18),
    (768, 768, True, "custom", 3, 19),
    (3072, 768, False, "mixture", 1, 20),
    (3072, 768, True, "moped", 11, 21),
    (64, 3072, False, "moped_trainable", 3, 22),
    (768, 3072, True, "gaussian", 3, 23),
    (3072, 3072, True, "mixture", 1, 24),
    (24, 64, True, "custom", 3, 2 ** 32 - 2),      # the sample counter wraps inside the call: 2^32 - 2, 2^32 - 1, 0
]


@pytest.mark.parametrize("N,K,bias,prior,S,base", GRID)
def test_all_outputs_against_fp64_over_the_dispatch_grid(N, K, bias, prior, S, base):
    ref = reference_of(N, K, bias, prior, S, base)
    Ms = SMALL_M + (WIDE_M if N * K <= 512 * 512 else [])
    worst, cases = {}, 0
    for i, M in enumerate(Ms):
        for cdt_name, x16 in (COMBOS[i % 4], COMBOS[(i + 1) % 4]):
            what = f"N={N} K={K} bias={bias} {prior} S={S} base={base} M={M} {cdt_name} x={'16-bit' if x16 else 'fp32'}"
            ry, rl = check_case(ref, M, cdt_name, x16, what)
            w = worst.setdefault(template_of(M), [0.0, 0.0])
            w[0], w[1] = max(w[0], ry), max(w[1], rl)
            cases += 1
    for mb in sorted(worst):
        print(f"[fused_small grid] N={N} K={K} bias={int(bias)} {prior} S={S} MB={mb}: y max err / bound = {worst[mb][0]:.3f}, "
              f"log-prob max err / bound = {worst[mb][1]:.3f}")
    print(f"[fused_small grid] N={N} K={K} {prior} S={S}: {cases} cases, one fused launch each; "
          f"W_s max err / bound = {ref.w_ratio:.3f}")


# one ragged M per template (1, 2, 3, 4, 6 by 5 -> 6, 6, 8 by 7 -> 8, 8) on a 4-wave and an 8-wave layer with ragged N
@pytest.mark.parametrize("N,K,bias,prior", [(33, 160, True, "custom"), (200, 544, True, "gaussian")])
@pytest.mark.parametrize("M", [6, 17, 33, 49, 65, 81, 97, 113])
def test_batched_equals_serial_and_repeats_bit_for_bit(N, K, bias, prior, M):
    """Sample s of an S-batched call == the single-sample call at base + s; two identical calls are bit-equal."""
    layer = layer_of(N, K, bias, prior)
    S, base = 4, 300
    for cdt_name, x16 in COMBOS[(M // 16) % 2::2]:
        with compute_dtype(cdt_name) as cdt:
            x = make_input(M, K, cdt if x16 else None)
            what = f"N={N} K={K} M={M} {cdt_name}"
            y, lp = fused_run(layer, x, S, base, what)
            y2, lp2 = fused_run(layer, x, S, base, what)
            assert torch.equal(y, y2) and torch.equal(lp, lp2)
            for s in range(S):
                ys, lps = fused_run(layer, x, 1, base + s, what)
                assert torch.equal(ys[0], y[s]) and torch.equal(lps[0], lp[s]), (what, s)
    print(f"[fused_small repeat] N={N} K={K} M={M} MB={template_of(M)}: batched == serial == repeated, one fused launch each")


@pytest.mark.parametrize("N,K,bias,prior,M", [(33, 160, True, "custom", 49), (200, 544, True, "gaussian", 97)])
def test_device_counter_mode_equals_host_counter_bit_for_bit(N, K, bias, prior, M):
    """`sample_base + *counter`: with the counter in device memory, a forward after three others have moved it draws what
    the host-counter forward at the same index draws."""
    layer = layer_of(N, K, bias, prior)
    x = make_input(M, K)
    base, S = 700, 3
    y_host, lp_host = fused_run(layer, x, S, base + 6)
    assert bfr.STATE.device_counter is None and _C.lib().bf_get_sample_counter() is None
    bf.use_device_counter(True)
    try:
        model = bnn.Model(layer)
        bf.manual_seed(SEED, next_sample=base)
        with torch.no_grad():
            with model.monte_carlo(2):
                for _ in range(3):
                    model(x.repeat(2, 1))
            with launches() as c, model.monte_carlo(S):
                y = model(x.repeat(S, 1)).view(S, M, N)
            lp = model.log_prob_samples().clone()
        assert int(bfr.STATE.device_counter.item()) == base + 6 + S
    finally:
        bf.use_device_counter(False)
    assert_fused(c)
    assert bfr.STATE.device_counter is None and _C.lib().bf_get_sample_counter() is None
    assert torch.equal(y, y_host) and torch.equal(lp, lp_host)


# ------------------------------------------------------------------------------------------------ 3. the hard values
def _edit_edges(g, rows):
    """The regimes of the `edge` / `edge_inf` fixtures on parameter `g` ([N, K] weight: a few columns per row; [N] bias: one
    entry per row): rho = 25 and rho = 20 with its two fp32 neighbours (the softplus threshold, both sides), rho = -30 (tiny
    sigma), rho = -12 next to means deep in the mixture's tail (15: where the reference's fp32 expression gives -inf)."""
    tail = torch.tensor([14.0, -14.2, 5.0, -9.0, 15.0])
    twenty = torch.tensor(20.0)
    above, below = torch.nextafter(twenty, torch.tensor(30.0)), torch.nextafter(twenty, torch.tensor(0.0))
    with torch.no_grad():
        if g.mu.dim() == 2:
            g.rho[rows[0], :4] = 25.0
            g.rho[rows[1], :4] = torch.stack([twenty, above, below, twenty])
            g.rho[rows[2], :4] = -30.0
            g.mu[rows[3], 8:13] = tail
            g.rho[rows[3], 8:13] = -12.0
            g.mu[rows[3], 13] = -14.2       # ... and both at once
            g.rho[rows[3], 13] = -30.0
        else:
            g.rho[rows[0]] = 25.0
            g.rho[rows[1]] = 20.0
            g.rho[rows[1] + 1] = above
            g.rho[rows[2]] = -30.0
            n = min(5, g.mu.numel() - rows[3])
            g.mu[rows[3]:rows[3] + n] = tail[:n]
            g.rho[rows[3]:rows[3] + n] = -12.0


def _hard_layer(kind, N, K):
    torch.manual_seed(31 * N + K)
    if kind in ("mixture", "custom"):       # the default mixture has sigma2 = e^-6
        prior = bnn.DEFAULT_SCALED_GAUSSIAN_MIXTURE if kind == "mixture" else bnn.ScaledGaussianMixture(0.3, 2.0, 0.05)
        layer = bnn.Linear(K, N, prior=prior)
        _edit_edges(layer.weight, [0, 1, 2, 3])
        _edit_edges(layer.weight, [N - 1, N - 2, N - 3, N - 4])    # the last, partial feature block carries them too
        _edit_edges(layer.bias, [0, 1, 3, 4])
    else:                                   # MOPED: zero weights (rho := 0), a weight below the resolution of exp(x) - 1
        freq = torch.nn.Linear(K, N)
        with torch.no_grad():
            freq.weight.mul_(0.2)
            freq.weight[0, :5] = 0.0
            freq.weight[1, 0] = 1e-7
            freq.weight[N - 1, K - 3:] = 0.0
            freq.weight[N - 1, 0] = -1e-7
            freq.bias[3] = 0.0
            freq.bias[N - 1] = 1e-7
        layer = bnn.Linear.from_frequentist(freq, delta=0.05, freeze=kind == "moped")
        rho_w, rho_b = layer.weight.rho.detach(), layer.bias.rho.detach()
        assert float(rho_w[0, 0]) == 0.0 and float(rho_w[1, 0]) == 0.0
        assert float(rho_b[3]) == 0.0 and float(rho_b[N - 1]) == 0.0
    layer.layer_id = 0
    return layer.cuda()


@pytest.mark.parametrize("K", [32, 64])
@pytest.mark.parametrize("kind,N", [("mixture", 24), ("custom", 9), ("moped", 33), ("moped_trainable", 18)])
def test_hard_parameter_values_through_the_fused_kernel(kind, N, K):
    """The fixtures that carry these values have K = 24 and K = 8 and never reach this kernel: its own softplus_fast /
    log_fast / prior_term calls see them here.  Against the oracle's fp64 closed forms (the reference's fp32 values are -inf
    or cancel there, tests/test_gpu_linear.py NO_REF_LOGPROB); finite wherever the fp64 value is."""
    S, base = 3, 40
    ref = Reference(_hard_layer(kind, N, K), S, base)
    worst = 0.0
    for M, (cdt_name, x16) in zip((6, 17, 64, 49), COMBOS):
        what = f"hard values {kind} N={N} K={K} M={M} {cdt_name}"
        with compute_dtype(cdt_name) as cdt:
            x = make_input(M, K, cdt if x16 else None)
            y, lp = fused_run(ref.layer, x, S, base, what)
            assert bool(torch.isfinite(lp).all()) and bool(torch.isfinite(y).all())
            worst = max(worst, ref.check_logprobs(lp, what))
            ry = y_ratio(y, ref.y(x, cdt), K)
            assert ry <= 1.0, (what, ry)
    print(f"[fused_small hard values] {kind} N={N} K={K}: log-prob max err / bound = {worst:.3f}; "
          f"sampled values max err / bound = {ref.w_ratio:.3f}")


# ------------------------------------------------------------------------------------------------ 4. the two paths agree
# at least one shape per template, ragged N, each prior kind: (N, K, bias, prior, S, base, Ms)
CROSS = [
    (1, 32, True, "mixture", 3, 10, [1, 17, 128]),
    (33, 160, True, "custom", 3, 13, [6, 33, 81]),
    (200, 544, True, "gaussian", 1, 16, [49, 65, 97, 113]),
    (2, 768, True, "moped", 3, 18, [16, 48, 96]),
    (512, 512, True, "mixture", 3, 15, [64, 128]),
    (64, 3072, False, "moped_trainable", 3, 22, [17, 112]),
    (3072, 768, False, "mixture", 1, 20, [33, 64]),
]


@pytest.mark.parametrize("N,K,bias,prior,S,base,Ms", CROSS)
def test_fused_and_two_launch_paths_agree(N, K, bias, prior, S, base, Ms):
    """bf_set_fused_small_max_rows(0) sends the same layer through the sampling launch + tiled GEMM: the same products in
    another fp32 summation order (twice the y bound), the same log-prob terms summed by another kernel."""
    ref = reference_of(N, K, bias, prior, S, base)
    layer = ref.layer
    worst = {}
    for i, M in enumerate(Ms):
        cdt_name, x16 = COMBOS[i % 4]
        what = f"N={N} K={K} {prior} S={S} M={M} {cdt_name} x={'16-bit' if x16 else 'fp32'}"
        with compute_dtype(cdt_name) as cdt:
            x = make_input(M, K, cdt if x16 else None)
            y, lp = fused_run(layer, x, S, base, what)
            with fused_rows_capped(0):
                with launches() as c:
                    y2, lp2 = run_layer(layer, x, S, base)
            assert_two_launch(c, what)
            y64 = ref.y(x, cdt)
            bound = Y_TOL[y.dtype] * y64.abs().max().item() + 1e-5 * np.sqrt(K)
            ry = (y.double() - y2.double()).abs().max().item() / (2 * bound)
            assert ry <= 1.0, (what, ry)
            assert y_ratio(y2, y64, K) <= 1.0, what     # (and the tiled path meets the fp64 bound itself)
            rl = 0.0
            for s in range(S):
                for col in (0, 1):
                    r = abs(float(lp[s, col]) - float(lp2[s, col])) / (LOGPROB_RTOL * ref.mags[s][col])
                    assert r <= 1.0, (what, s, col, float(lp[s, col]), float(lp2[s, col]))
                    rl = max(rl, r)
            w = worst.setdefault(template_of(M), [0.0, 0.0])
            w[0], w[1] = max(w[0], ry), max(w[1], rl)
    for mb in sorted(worst):
        print(f"[fused_small two paths] N={N} K={K} {prior} S={S} MB={mb}: |y - y'| / (2 bound) = {worst[mb][0]:.3f}, "
              f"log-probs / bound = {worst[mb][1]:.3f}; zero fused launches in the forced runs")


# ------------------------------------------------------------------------------------------------ 5. nothing else written
@pytest.mark.parametrize("N,K,bias,prior,M", [(7, 544, False, "custom", 17), (33, 160, True, "custom", 49),
                                              (2, 768, True, "moped", 97), (1, 32, True, "mixture", 113),
                                              (33, 32, False, "gaussian", 6)])
@pytest.mark.parametrize("cdt_name,x16", COMBOS)
def test_nothing_outside_the_output_is_written(N, K, bias, prior, M, cdt_name, x16):
    """bf_linear_fwd called as ops.linear_forward calls it, with y inside a buffer filled with a marker: ragged M and
    N % 4 != 0 take the scalar stores and the row / feature guards — the bands before and after come back untouched, the
    inside is the run_layer result bit for bit.  Observes only: every argument is in range."""
    layer = layer_of(N, K, bias, prior)
    lib = _C.lib()
    S, base, band, mark = 3, 77, 8192, 12345.0
    with compute_dtype(cdt_name) as cdt:
        x = make_input(M, K, cdt if x16 else None)
        want, lp_want = fused_run(layer, x, S, base)
        xs = x.repeat(S, 1).contiguous()
        w, b = _C.bf_tensor_t(), _C.bf_tensor_t()
        assert ops.fill_tensor(w, layer.weight, layer.weight_prior, 0)
        if bias:
            assert ops.fill_tensor(b, layer.bias, layer.bias_prior, 1)
        dt = ops._TORCH2BF[x.dtype]
        need = lib.bf_linear_fwd_workspace_bytes(S, M, N, K, int(bias), ops._TORCH2BF[cdt], dt)
        ws = ops.workspace(x.device, need)
        lp = torch.zeros((S, 2), dtype=torch.float64, device="cuda")
        n = S * M * N
        buf = torch.full((n + 2 * band,), mark, device="cuda", dtype=x.dtype)
        guard = torch.full((band,), mark, device="cuda", dtype=x.dtype)
        got = buf[band:band + n]
        with launches() as c:
            _C.check(lib.bf_linear_fwd(xs.data_ptr(), dt, M * K, ctypes.byref(w), ctypes.byref(b) if bias else None,
                                       got.data_ptr(), dt, ops._TORCH2BF[cdt], S, M, N, K, SEED, base, lp.data_ptr(),
                                       ws.data_ptr(), ws.numel(), ops._stream_ptr()), "bf_linear_fwd")
        assert_fused(c)
        assert torch.equal(buf[:band], guard) and torch.equal(buf[band + n:], guard)
        assert torch.equal(got.view(S, M, N), want) and torch.equal(lp, lp_want)
