"""Bayesian mixture-of-experts layers on the device: bf_moe_route / bf_moe_gate_up / bf_moe_down / bf_moe_combine against
float64 (tests/moe_ref.py) on each stage's own inputs, their refusals, bnn.Experts (log-probs, output, gradients, checkpoint
recomputation) and converted tiny Mixtral / Qwen3-MoE decoders through sample_bayesian, training_step and sample_generate.
Bounds: one rounding to a 16-bit output is 2^-7 (bf16) / 2^-10 (fp16) of max |ref| (tests/test_gpu_backward.py); an fp32
result of 16-bit operands 2^-8 / 2^-11 of max |ref| plus 1e-5 sqrt(contraction length) (tests/test_gpu_kept_weights.py).  The
layer's bounds are measured per run: twice the error the framework's own 16-bit ops make against float64 on the same input
and the same draws, never below the one-rounding bound."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import moe_ref  # noqa: E402

import bayeformers_amd as bf  # noqa: E402
import bayeformers_amd.nn as bnn  # noqa: E402
from bayeformers_amd import _C, ops  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 0x30E
ROUND = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}
ACC32 = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
DTYPES = [torch.bfloat16, torch.float16]
# S, M, E, k, H, I, routing
CASES = [(1, 1, 2, 1, 64, 32, "random"),      # the smallest case
         (2, 5, 4, 2, 96, 40, "random"),      # both tails
         (3, 37, 8, 2, 128, 72, "random"),    # groups that cross tile boundaries
         (1, 70, 4, 1, 64, 32, "first"),      # one long group, all others empty
         (2, 3, 128, 8, 64, 32, "random"),    # 256 groups, almost all empty
         (2, 5, 4, 2, 96, 40, "dropped")]     # some indices set to E
IDS = ["smallest", "tails", "cross-tile", "one-group", "256-groups", "dropped"]


def _err(got, ref):
    return (got.double().cpu() - ref.double().cpu()).abs().max().item()


def _routing(S, M, E, k, kind, g):
    R = S * M
    wts, idx = torch.topk(torch.softmax(torch.randn(R, E, generator=g), -1), k, dim=-1)
    if kind == "first":
        idx = torch.zeros_like(idx)
    if kind == "dropped":
        idx[::3, 0] = E
        idx[4, 1] = E
        idx[7] = E  # a row with no expert at all
    return idx.contiguous(), wts.contiguous()


_REF = {}


def _problem(case, dt):
    """Operands of one case (host copies, the device copies) and its float64 route; made once per (case, dtype)."""
    key = (case, dt)
    if key not in _REF:
        S, M, E, k, H, I, kind = case
        g = torch.Generator().manual_seed(7 + 13 * CASES.index(case))
        x = torch.randn(S * M, H, generator=g).to(dt)
        w_gu = (torch.randn(S, E, 2 * I, H, generator=g) / H ** 0.5).to(dt)
        w_d = (torch.randn(S, E, H, I, generator=g) / I ** 0.5).to(dt)
        idx, wts = _routing(S, M, E, k, kind, g)
        _REF[key] = dict(x=x, w_gu=w_gu, w_d=w_d, idx=idx, wts=wts, route=moe_ref.route(idx, S, E),
                         h=moe_ref.gate_up(x, idx, w_gu, S))
    return _REF[key]


# ------------------------------------------------------------------------------------------------------------ 1. kernels
@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_stages_against_fp64(case, dt):
    S, M, E, k, H, I, _ = case
    R = S * M
    p = _problem(case, dt)
    x, w_gu, w_d, idx, wts = (p[n].cuda() for n in ("x", "w_gu", "w_d", "idx", "wts"))
    live = moe_ref.live_mask(p["idx"], E)
    slot_live = live.reshape(-1)

    # route: equal to the reference exactly
    offsets, slots, tiles = ops.moe_route(idx, S, E)
    off_ref, slots_ref = p["route"]
    n_live = int(off_ref[-1])
    assert n_live == int(slot_live.sum())
    assert offsets.dtype == torch.int32 and torch.equal(offsets.cpu().long(), off_ref)
    assert torch.equal(slots.cpu().long()[:n_live], slots_ref)
    nt = ops.moe_max_tiles(S, E, R, k)
    assert tiles.shape == (nt, 3) and torch.equal(tiles.cpu().long(), moe_ref.tiles(off_ref, nt))
    route = (offsets, slots, tiles)

    # gate_up: h = silu(gate) * up, rounded once
    h = ops.moe_gate_up(x, w_gu, route, k)
    assert h.dtype == dt and h.shape == (R * k, I)
    eh, bh = _err(h[slot_live.cuda()], p["h"][slot_live]), ROUND[dt] * p["h"].abs().max().item()
    # down on the h the kernel produced: fp32 of 16-bit operands
    y = ops.moe_down(h, w_d, route, k)
    assert y.dtype == torch.float32 and y.shape == (R, k, H)
    h_host = torch.where(slot_live[:, None], h.cpu().double(), torch.zeros((), dtype=torch.float64))
    y_ref = moe_ref.down(h_host, p["idx"], w_d, S)
    ey, by = _err(y[live.cuda()], y_ref[live]), ACC32[dt] * y_ref.abs().max().item() + 1e-5 * I ** 0.5
    # combine on the y the kernel produced: one rounding
    out = ops.moe_combine(y, idx, wts, E, dt)
    y_host = torch.where(live[:, :, None], y.cpu().double(), torch.zeros((), dtype=torch.float64))
    out_ref = moe_ref.combine(y_host, p["idx"], p["wts"], E)
    eo, bo = _err(out, out_ref), ROUND[dt] * out_ref.abs().max().item()
    print(f"moe {dt} {case}: h err {eh:.3e} (bound {bh:.3e}), y err {ey:.3e} (bound {by:.3e}), out err {eo:.3e} (bound {bo:.3e})")
    assert out.dtype == dt and out.shape == (R, H) and torch.isfinite(out).all()
    assert eh <= bh and ey <= by and eo <= bo
    if not live.all():
        assert not out[(~live).all(1).cuda()].any()  # a row whose slots were all dropped is zero
    # the weights in the compute dtype are read as they are
    out16 = ops.moe_combine(y, idx, wts.to(dt), E, dt)
    assert _err(out16, moe_ref.combine(y_host, p["idx"], p["wts"].to(dt), E)) <= bo

    # no atomics: every entry run again gives the same bits
    offsets2, slots2, tiles2 = ops.moe_route(idx, S, E)
    assert torch.equal(offsets2, offsets) and torch.equal(slots2[:n_live], slots[:n_live]) and torch.equal(tiles2, tiles)
    h2 = ops.moe_gate_up(x, w_gu, route, k)
    y2 = ops.moe_down(h, w_d, route, k)
    assert torch.equal(h2[slot_live.cuda()], h[slot_live.cuda()]) and torch.equal(y2[live.cuda()], y[live.cuda()])
    assert torch.equal(ops.moe_combine(y, idx, wts, E, dt), out)
    # the four entries as moe_forward strings them together
    c0 = dict(ops.MOE_CALLS)
    whole = ops.moe_forward(x, idx, wts, w_gu, w_d, S, torch.nn.functional.silu)
    assert torch.equal(whole, out) and ops.MOE_CALLS["composite_fwd"] == c0["composite_fwd"]
    assert [ops.MOE_CALLS[n] - c0[n] for n in ("route", "gate_up", "down", "combine")] == [1, 1, 1, 1]


def _host_waits(fn):
    """Synchronising framework calls (a read-back to the host: .item(), .nonzero(), .tolist(), ...) one call of `fn` makes."""
    import warnings

    fn()
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    return sum("synchroniz" in str(w.message).lower() for w in seen)


def test_kernel_route_never_waits_for_the_host():
    """What makes a decode step with experts capturable: the four entries read nothing back, where the framework's loop (its
    own module, and ops.moe_composite) waits for the device once or more per call."""
    case, dt = CASES[2], torch.bfloat16
    S, M, E, k, H, I, _ = case
    p = _problem(case, dt)
    x, w_gu, w_d, idx, wts = (p[n].cuda() for n in ("x", "w_gu", "w_d", "idx", "wts"))
    assert _host_waits(lambda: ops.moe_forward(x, idx, wts, w_gu, w_d, S, torch.nn.functional.silu)) == 0
    loop = _host_waits(lambda: ops.moe_composite(x, idx, wts, w_gu, w_d, S, torch.nn.functional.silu))
    src = _framework_experts(E, H, I).cuda().to(dt)
    with torch.no_grad():
        module = _host_waits(lambda: src(x[:M], idx[:M], wts[:M]))
    print(f"host waits per call: kernel route 0, ops.moe_composite {loop}, the framework's experts module {module}")
    assert loop >= S and module >= 1


def test_long_groups_take_the_loop_eagerly_and_the_kernels_in_a_capture():
    """ops.moe_kernel_wins sends an eager call with more than 128 rows per group to the framework loop
    (profiles/bayesian_moe.md); a capturing stream takes the kernels whatever the size, because the loop cannot be captured."""
    dt, S, E, k, H, I, R = torch.bfloat16, 1, 2, 1, 64, 32, 300
    g = torch.Generator().manual_seed(21)
    x = torch.randn(R, H, generator=g).to(dt).cuda()
    w_gu = (torch.randn(S, E, 2 * I, H, generator=g) / H ** 0.5).to(dt).cuda()
    w_d = (torch.randn(S, E, H, I, generator=g) / I ** 0.5).to(dt).cuda()
    idx = torch.randint(0, E, (R, k), generator=g).cuda()
    wts = torch.rand(R, k, generator=g).cuda()
    silu = torch.nn.functional.silu
    assert not ops.moe_kernel_wins(S, E, k, R) and ops.moe_supported(dt, H, I, E, k, silu, x, w_gu, w_d, S=S)
    assert not ops.moe_supported(dt, H, I, E, k, silu, x, w_gu, w_d, S=S, rows=R)
    route = ops.moe_route(idx, S, E)
    want = ops.moe_combine(ops.moe_down(ops.moe_gate_up(x, w_gu, route, k), w_d, route, k), idx, wts, E, dt)
    c0 = dict(ops.MOE_CALLS)
    eager = ops.moe_forward(x, idx, wts, w_gu, w_d, S, silu)
    assert ops.MOE_CALLS["composite_fwd"] == c0["composite_fwd"] + 1 and ops.MOE_CALLS["gate_up"] == c0["gate_up"]
    ref = moe_ref.forward(x.cpu(), idx.cpu(), wts.cpu(), w_gu.cpu(), w_d.cpu(), S)
    assert _err(eager, ref) <= 4 * ROUND[dt] * ref.abs().max().item()  # (the loop rounds h, y and the sum: a few roundings)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.moe_forward(x, idx, wts, w_gu, w_d, S, silu)
    assert ops.MOE_CALLS["gate_up"] == c0["gate_up"] + 1 and ops.MOE_CALLS["composite_fwd"] == c0["composite_fwd"] + 1
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    idx.copy_(1 - idx)  # another routing through the same captured launches: the grid never depended on the data
    route = ops.moe_route(idx, S, E)
    want = ops.moe_combine(ops.moe_down(ops.moe_gate_up(x, w_gu, route, k), w_d, route, k), idx, wts, E, dt)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)


def test_refusals_name_the_entry_and_the_condition():
    dt = torch.bfloat16
    S, E, k, H, R = 1, 4, 2, 64, 4
    idx = torch.zeros(R, k, dtype=torch.long, device="cuda")
    route = ops.moe_route(idx, S, E)

    def operands(I, dtype=dt):
        return (torch.zeros(R, H, dtype=dtype, device="cuda"), torch.zeros(S, E, 2 * I, H, dtype=dtype, device="cuda"),
                torch.zeros(R * k, I, dtype=dtype, device="cuda"), torch.zeros(S, E, H, I, dtype=dtype, device="cuda"))

    x, w_gu, h, w_d = operands(36)
    with pytest.raises(_C.BayeFormersAMDError) as e:
        ops.moe_gate_up(x, w_gu, route, k)
    assert "bf_moe_gate_up" in str(e.value) and "I % 8 == 0" in str(e.value)
    with pytest.raises(_C.BayeFormersAMDError) as e:
        ops.moe_down(h, w_d, route, k)
    assert "bf_moe_down" in str(e.value) and "I % 8 == 0" in str(e.value)
    assert not ops.moe_supported(dt, H, 36, E, k, "silu", x, w_gu, w_d)
    x, w_gu, h, w_d = operands(32, torch.float32)
    with pytest.raises(_C.BayeFormersAMDError) as e:
        ops.moe_gate_up(x, w_gu, route, k)
    assert "bf_moe_gate_up" in str(e.value) and "16-bit" in str(e.value)
    with pytest.raises(_C.BayeFormersAMDError) as e:
        ops.moe_down(h, w_d, route, k)
    assert "bf_moe_down" in str(e.value) and "16-bit" in str(e.value)
    assert not ops.moe_supported(torch.float32, H, 32, E, k, "silu", x, w_gu, w_d)
    big_k = ops.MOE_MAX_TOPK + 1
    with pytest.raises(_C.BayeFormersAMDError) as e:
        ops.moe_route(torch.zeros(R, big_k, dtype=torch.long, device="cuda"), S, 32)
    assert "bf_moe_route" in str(e.value) and f"k <= {ops.MOE_MAX_TOPK}" in str(e.value)
    assert not ops.moe_supported(dt, H, 32, 32, big_k, "silu")
    with pytest.raises(_C.BayeFormersAMDError) as e:
        ops.moe_route(idx, 2, ops.MOE_MAX_GROUPS // 2 + 1)
    assert "bf_moe_route" in str(e.value) and f"S*E <= {ops.MOE_MAX_GROUPS}" in str(e.value)
    assert not ops.moe_supported(dt, H, 32, ops.MOE_MAX_GROUPS // 2 + 1, k, "silu", S=2)
    x, w_gu, h, w_d = operands(32)
    assert ops.moe_supported(dt, H, 32, E, k, "silu", x, w_gu, w_d)
    assert not ops.moe_supported(dt, H, 32, E, k, "gelu", x, w_gu, w_d)


# -------------------------------------------------------------------------------------------------------------- 2. layer
@pytest.fixture
def _restore_dtype():
    prev = bf.get_compute_dtype()
    yield
    bf.set_compute_dtype({torch.float32: "fp32", torch.bfloat16: "bf16", torch.float16: "fp16"}[prev])
    bf.set_kl_gradient(False)


def _framework_experts(E, H, I, seed=4):
    from transformers import MixtralConfig
    from transformers.models.mixtral.modeling_mixtral import MixtralExperts

    mod = MixtralExperts(MixtralConfig(hidden_size=H, intermediate_size=I, num_local_experts=E, num_experts_per_tok=2))
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        mod.gate_up_proj.copy_(torch.randn(E, 2 * I, H, generator=g) / H ** 0.5)
        mod.down_proj.copy_(torch.randn(E, H, I, generator=g) / I ** 0.5)
    return mod


def _layer(E, H, I, dt, rho=None, delta=0.05):
    src = _framework_experts(E, H, I)
    layer = bnn.Experts.from_frequentist(src, delta=delta)
    if rho is not None:
        with torch.no_grad():
            layer.gate_up_proj.rho.fill_(rho)
            layer.down_proj.rho.fill_(rho)
    model = bnn.Model(layer).cuda().to(dt)
    bf.set_compute_dtype("bf16" if dt == torch.bfloat16 else "fp16")
    return model, model.model, src


def _framework16(x, idx, wts, w_gu, w_d, S):
    """The layer's formula on the framework's own 16-bit ops (gathered weights, batched matmuls): the measure of what 16 bits
    cost on this input.  Differentiable."""
    R, k = idx.shape
    E, I = w_gu.shape[1], w_gu.shape[2] // 2
    g = (torch.arange(R, device=idx.device) // (R // S))[:, None] * E + idx
    gu = torch.einsum("rkih,rh->rki", w_gu.reshape(S * E, 2 * I, -1)[g], x)
    h = torch.nn.functional.silu(gu[..., :I]) * gu[..., I:]
    y = torch.einsum("rkhi,rki->rkh", w_d.reshape(S * E, -1, I)[g], h)
    return (wts[:, :, None] * y).sum(1).to(x.dtype)


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
def test_layer_with_zero_sigma_is_the_framework_module(dt, _restore_dtype):
    """rho = -40 (sigma ~ 4e-18) and S = 1: the output is the framework module's on the device."""
    E, H, I, k, R = 4, 96, 40, 2, 37
    model, layer, src = _layer(E, H, I, dt, rho=-40.0)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(R, H, generator=g).to(dt).cuda()
    wts, idx = torch.topk(torch.softmax(torch.randn(R, E, generator=g), -1), k, dim=-1)
    idx, wts = idx.cuda(), wts.cuda()
    c0 = dict(ops.MOE_CALLS)
    with torch.no_grad():
        out = layer(x, idx, wts)  # bare: S = 1, a private log-prob slot
        want16 = src.cuda().to(dt)(x, idx, wts)
    assert ops.MOE_CALLS["gate_up"] == c0["gate_up"] + 1 and ops.MOE_CALLS["composite_fwd"] == c0["composite_fwd"]
    assert layer.log_prob_samples.shape == (1, 2) and torch.isfinite(layer.log_prob_samples).all()
    ref = moe_ref.forward(x.cpu(), idx.cpu(), wts.cpu(), src.gate_up_proj.detach().cpu()[None], src.down_proj.detach().cpu()[None], 1)
    e_k, e_f = _err(out, ref), _err(want16, ref)
    bound = max(2.0 * e_f, ROUND[dt] * ref.abs().max().item())
    print(f"layer sigma=0 {dt}: kernel err {e_k:.3e}, framework module err {e_f:.3e}, bound {bound:.3e}")
    assert out.dtype == dt and e_k <= bound


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
def test_layer_forward_and_backward_against_reference(dt, _restore_dtype):
    S, M, E, H, I, k = 3, 5, 4, 96, 40, 2
    R = S * M
    model, layer, _ = _layer(E, H, I, dt)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(M, H, generator=g).to(dt).cuda()
    logits = torch.randn(R, E, generator=g).cuda().requires_grad_(True)
    dy = torch.randn(R, H, generator=g).to(dt).cuda()
    bf.manual_seed(SEED, next_sample=5)
    c0 = dict(ops.MOE_CALLS)
    xin = x.repeat(S, 1).requires_grad_(True)
    wts, idx = torch.topk(torch.softmax(logits, -1), k, dim=-1)
    wts.retain_grad()
    with model.monte_carlo(S):
        y = model(xin, idx, wts)
    assert [ops.MOE_CALLS[n] - c0[n] for n in ("sample", "route", "gate_up", "down", "combine", "composite_fwd")] == [1, 1, 1, 1, 1, 0]
    base, seed = model._last_base, bf.random.STATE.seed
    sids = [2 * layer.layer_id, 2 * layer.layer_id + 1]
    gs, priors = [layer.gate_up_proj, layer.down_proj], [layer.gate_up_proj_prior, layer.down_proj_prior]
    assert base == 5 and [sid for _, _, sid in layer.gaussians()] == sids
    # log-probs: a direct sample_logprob of the same Gaussians, seed and base, bitwise
    (w_gu, w_d), lp = ops.sample_logprob(gs, priors, sids, S, seed, base, out_dtype=dt)
    assert torch.equal(model.log_prob_samples(), lp) and torch.equal(layer.log_prob_samples, lp)
    y.backward(dy)
    assert ops.MOE_CALLS["composite_bwd"] == c0["composite_bwd"] + 1
    assert logits.grad is not None and logits.grad.abs().max() > 0  # the router trains through top_k_weights

    # float64 autograd of the reference on the same draws
    x64 = xin.detach().double().requires_grad_(True)
    wt64 = wts.detach().double().requires_grad_(True)
    gu64, d64 = w_gu.double().requires_grad_(True), w_d.double().requires_grad_(True)
    y_ref = moe_ref.forward(x64, idx, wt64, gu64, d64, S)
    y_ref.backward(dy.double())
    # ... and of the same formula on the framework's 16-bit ops
    x16 = xin.detach().clone().requires_grad_(True)
    wt16 = wts.detach().clone().requires_grad_(True)
    gu16, d16 = w_gu.clone().requires_grad_(True), w_d.clone().requires_grad_(True)
    y_c = _framework16(x16, idx, wt16, gu16, d16, S)
    y_c.backward(dy)

    def param_grads(dw, gauss, sid):
        eps = moe_ref.eps_host(tuple(gauss.mu.shape), seed, base, S, sid).to(dw.device)
        dw = dw.double()
        return dw.sum(0), (dw * eps).sum(0) * torch.sigmoid(gauss.rho.detach().double())

    def check(name, got, comp, want, floor):
        e_k, e_c = _err(got, want), _err(comp.reshape(want.shape), want)
        bound = max(2.0 * e_c, floor)
        print(f"layer {dt} {name}: kernel-route err {e_k:.3e}, framework 16-bit err {e_c:.3e}, bound {bound:.3e}")
        assert e_k <= bound, name

    top = lambda t: t.abs().max().item()
    check("y", y, y_c, y_ref.detach(), ROUND[dt] * top(y_ref))
    check("dx", xin.grad, x16.grad, x64.grad, ROUND[dt] * top(x64.grad))
    check("d top_k_weights", wts.grad, wt16.grad, wt64.grad, ACC32[dt] * top(wt64.grad) + 1e-5 * H ** 0.5)
    for name, gauss, sid, dw64, dw16 in (("gate_up_proj", layer.gate_up_proj, sids[0], gu64.grad, gu16.grad),
                                         ("down_proj", layer.down_proj, sids[1], d64.grad, d16.grad)):
        dmu, drho = param_grads(dw64, gauss, sid)
        dmu_c, drho_c = param_grads(dw16, gauss, sid)
        check(name + ".mu", gauss.mu.grad, dmu_c, dmu, ACC32[dt] * top(dmu) + 1e-5 * R ** 0.5)
        check(name + ".rho", gauss.rho.grad, drho_c, drho, ACC32[dt] * top(drho) + 1e-5 * R ** 0.5)


def test_layer_unsupported_calls_run_the_composite(_restore_dtype):
    """fp32 compute, and I % 8 != 0, run the framework loop on the draws the kernel made."""
    S, M, E, H, I, k = 2, 3, 4, 40, 12, 2
    src = _framework_experts(E, H, I)
    layer = bnn.Experts.from_frequentist(src, delta=0.05)
    model = bnn.Model(layer).cuda()
    bf.set_compute_dtype("fp32")
    g = torch.Generator().manual_seed(6)
    xin = torch.randn(M, H, generator=g).cuda().repeat(S, 1).requires_grad_(True)
    wts, idx = torch.topk(torch.softmax(torch.randn(S * M, E, generator=g), -1), k, dim=-1)
    idx, wts = idx.cuda(), wts.cuda().requires_grad_(True)
    bf.manual_seed(SEED)
    c0 = dict(ops.MOE_CALLS)
    with model.monte_carlo(S):
        y = model(xin, idx, wts)
    dy = torch.randn_like(y)
    y.backward(dy)
    assert ops.MOE_CALLS["composite_fwd"] == c0["composite_fwd"] + 1 and ops.MOE_CALLS["gate_up"] == c0["gate_up"]
    base, seed = model._last_base, bf.random.STATE.seed
    ws = []
    for gauss, _, sid in layer.gaussians():
        eps = moe_ref.eps_host(tuple(gauss.mu.shape), seed, base, S, sid)
        ws.append((moe_ref.sample(gauss.mu.detach().cpu(), gauss.rho.detach().cpu(), eps).requires_grad_(True), eps, gauss))
    x64, wt64 = xin.detach().cpu().double().requires_grad_(True), wts.detach().cpu().double().requires_grad_(True)
    y_ref = moe_ref.forward(x64, idx.cpu(), wt64, ws[0][0], ws[1][0], S)
    y_ref.backward(dy.cpu().double())
    pairs = [("y", y, y_ref.detach()), ("dx", xin.grad, x64.grad), ("d top_k_weights", wts.grad, wt64.grad)]
    for w, eps, gauss in ws:
        pairs += [("dmu", gauss.mu.grad, w.grad.sum(0)),
                  ("drho", gauss.rho.grad, (w.grad * eps).sum(0) * torch.sigmoid(gauss.rho.detach().cpu().double()))]
    for name, got, want in pairs:
        assert _err(got, want) <= 2e-5 * max(1.0, want.abs().max().item()), name  # fp32 arithmetic end to end


def test_layer_edge_inputs(_restore_dtype):
    dt = torch.bfloat16
    model, layer, _ = _layer(4, 64, 32, dt)
    idx = torch.zeros(5, 2, dtype=torch.long, device="cuda")
    with torch.no_grad(), model.monte_carlo(2), pytest.raises(ValueError, match="multiple of the sample count"):
        model(torch.zeros(5, 64, dtype=dt, device="cuda"), idx, torch.ones(5, 2, device="cuda"))
    with torch.no_grad(), model.monte_carlo(2):
        out = model(torch.zeros(0, 64, dtype=dt, device="cuda"), idx[:0], torch.ones(0, 2, device="cuda"))
    assert out.shape == (0, 64) and model.log_prob_samples().shape == (2, 2) and torch.isfinite(model.log_prob_samples()).all()


def test_layer_under_reentrant_checkpoint_gives_the_same_gradients(_restore_dtype):
    from torch.utils.checkpoint import checkpoint

    dt = torch.bfloat16
    S, M, E, H, I, k = 3, 5, 4, 64, 32, 2

    class Block(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.gate = torch.nn.Parameter(torch.randn(E, H) / H ** 0.5)
            self.experts = _framework_experts(E, H, I)
            self.proj = torch.nn.Linear(H, H)
            self.ckpt = False

        def block(self, x):
            wts, idx = torch.topk(torch.softmax(torch.nn.functional.linear(x, self.gate).float(), -1), k, dim=-1)
            return self.proj(self.experts(x, idx, wts))

        def forward(self, x):
            return checkpoint(self.block, x, use_reentrant=True) if self.ckpt else self.block(x)

    torch.manual_seed(0)
    model = bf.to_bayesian(Block(), delta=0.05, experts=True).cuda().to(dt)
    assert isinstance(model.model.experts, bnn.Experts)
    bf.set_compute_dtype("bf16")
    x = torch.randn(M, H, device="cuda").to(dt)
    dy = torch.randn(S * M, H, device="cuda").to(dt)

    def run(ckpt):
        model.model.ckpt = ckpt
        for p in model.parameters():
            p.grad = None
        bf.manual_seed(SEED, next_sample=3)
        xin = x.repeat(S, 1).requires_grad_(True)
        with model.monte_carlo(S):
            out = model(xin)
        lps = model.log_prob_samples().clone()
        out.backward(dy)
        grads = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
        grads["x"] = xin.grad.clone()
        return out.detach().clone(), lps, grads

    out0, lp0, g0 = run(False)
    out1, lp1, g1 = run(True)
    assert torch.equal(out0, out1) and torch.equal(lp0, lp1)
    assert g0.keys() == g1.keys() and {n for n in g0 if "experts" in n} == {
        "model.experts.gate_up_proj.mu", "model.experts.gate_up_proj.rho", "model.experts.down_proj.mu", "model.experts.down_proj.rho"}
    assert "model.gate" in g0 and g0["model.gate"].abs().max() > 0
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n


# -------------------------------------------------------------------------------------------------------------- 3. models
def _tiny_src(kind, norm_topk_prob=True):
    if kind == "mixtral":
        from transformers import MixtralConfig, MixtralForCausalLM

        cfg = MixtralConfig(hidden_size=64, intermediate_size=32, num_local_experts=4, num_experts_per_tok=2,
                            num_attention_heads=4, num_key_value_heads=2, num_hidden_layers=2, vocab_size=256,
                            max_position_embeddings=128, sliding_window=None, tie_word_embeddings=False, attention_dropout=0.0,
                            attn_implementation="sdpa")
        torch.manual_seed(0)
        return MixtralForCausalLM(cfg).eval()
    from transformers import Qwen3MoeConfig, Qwen3MoeForCausalLM

    cfg = Qwen3MoeConfig(hidden_size=64, intermediate_size=96, moe_intermediate_size=32, num_experts=8, num_experts_per_tok=2,
                         norm_topk_prob=norm_topk_prob, num_attention_heads=4, num_key_value_heads=2, head_dim=16,
                         num_hidden_layers=2, vocab_size=256, max_position_embeddings=128, decoder_sparse_step=1,
                         mlp_only_layers=[], tie_word_embeddings=False, attention_dropout=0.0, attn_implementation="sdpa")
    torch.manual_seed(0)
    return Qwen3MoeForCausalLM(cfg).eval()


def _to16(model, dt):
    """model.to(dt) with the rotary frequencies kept in fp32 (as tests/test_gpu_kept_weights.py does)."""
    freqs = {n: b.detach().clone() for n, b in model.named_buffers() if "inv_freq" in n}
    model = model.to(dt)
    for n, b in freqs.items():
        setattr(model.get_submodule(n.rsplit(".", 1)[0]), n.rsplit(".", 1)[1], b)
    return model


def _converted(src, experts=True, dt=torch.bfloat16, freeze=True):
    bmodel = _to16(bf.to_bayesian(src, delta=0.05, freeze=freeze, experts=experts).eval().cuda(), dt)
    assert bf.fuse_attention(bmodel)
    bf.set_compute_dtype("bf16" if dt == torch.bfloat16 else "fp16")
    return bmodel


def _ids(B=2, T=21, vocab=256, seed=11):
    return torch.randint(0, vocab, (B, T), generator=torch.Generator().manual_seed(seed)).cuda()


MODELS = [("mixtral", True), ("qwen3_moe", True), ("qwen3_moe", False)]
MODEL_IDS = ["mixtral", "qwen3moe-norm", "qwen3moe-raw"]


@pytest.mark.parametrize("kind,norm", MODELS, ids=MODEL_IDS)
def test_sample_bayesian_counts_the_experts(kind, norm, _restore_dtype):
    from bayeformers_amd.sampling import sample_bayesian

    src, S, ids = _tiny_src(kind, norm), 3, _ids()
    with_e, without = _converted(src, True), _converted(src, False)
    layers = [m for m in with_e.modules() if isinstance(m, bnn.Experts)]
    assert len(layers) == 2 and not any(isinstance(m, bnn.Experts) for m in without.modules())
    lps = []
    for m in (with_e, without):
        bf.manual_seed(SEED)
        c0 = dict(ops.MOE_CALLS)
        with torch.no_grad():
            raw, _, _, _ = sample_bayesian(m, {"input_ids": ids, "use_cache": False}, S)
        assert torch.isfinite(raw[0]).all() and raw[0].shape[:3] == (S, 2, ids.shape[1])
        used = ops.MOE_CALLS["gate_up"] - c0["gate_up"]
        assert used == (2 if m is with_e else 0) and ops.MOE_CALLS["composite_fwd"] == c0["composite_fwd"]
        lps.append(m.log_prob_samples().clone())
    base, seed = with_e._last_base, bf.random.STATE.seed
    assert without._last_base == base
    extra = torch.zeros_like(lps[0])
    for l in layers:
        gs, priors, sids = zip(*l.gaussians())
        extra += ops.sample_logprob(list(gs), list(priors), list(sids), S, seed, base)[1]
    assert extra[:, 0].abs().min() > 0
    assert torch.allclose(lps[0], lps[1] + extra, rtol=1e-12, atol=0)
    assert torch.allclose(with_e.log_prior().double(), (lps[1] + extra)[:, 0].mean(), rtol=1e-6)


@pytest.mark.parametrize("kind,norm", MODELS[:2], ids=MODEL_IDS[:2])
def test_training_step_reaches_the_experts_and_the_router(kind, norm, _restore_dtype):
    from bayeformers_amd import training

    bmodel = _converted(_tiny_src(kind, norm), True, freeze=False).train()
    ids = _ids()
    params = [p for p in bmodel.parameters() if p.requires_grad]
    opt = torch.optim.SGD(params, lr=0.0)

    def nll(mean):
        logits = mean[0][:, :-1].float()
        return torch.nn.functional.cross_entropy(logits.reshape(-1, logits.shape[-1]), ids[:, 1:].reshape(-1))

    bf.manual_seed(SEED)
    c0 = dict(ops.MOE_CALLS)
    loss = training.training_step(bmodel, {"input_ids": ids, "use_cache": False}, 3, nll, opt, n_batches=10)
    assert torch.isfinite(loss)
    assert ops.MOE_CALLS["gate_up"] == c0["gate_up"] + 2 and ops.MOE_CALLS["composite_bwd"] == c0["composite_bwd"] + 2
    seen = 0
    for n, p in bmodel.named_parameters():
        if ".experts." in n and n.endswith((".mu", ".rho")) and "_prior" not in n:
            assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, n
            seen += 1
        if n.endswith("mlp.gate.weight"):
            assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, n
            seen += 1
    assert seen == 2 * 4 + 2


def _same(a, b, log_probs=True):
    """Two Generations bitwise; log_probs=False: their log-probs to 2e-6 instead (tests/test_gpu_generate_graph.py's bound for
    sums the kept-weight plan and the per-layer launches form in different orders)."""
    import dataclasses

    for f in dataclasses.fields(a):
        x, y = getattr(a, f.name), getattr(b, f.name)
        if not log_probs and f.name in ("log_prior", "log_variational_posterior"):
            assert torch.allclose(x, y, rtol=2e-6, atol=0), f.name
        else:
            assert torch.equal(x, y), f.name


@pytest.mark.parametrize("kind,norm", MODELS[:2], ids=MODEL_IDS[:2])
def test_generation_modes_agree(kind, norm, _restore_dtype):
    from bayeformers_amd.sampling import sample_generate

    bmodel = _converted(_tiny_src(kind, norm), True)
    ids = _ids()
    S, n, T0 = 3, 8, ids.shape[1]

    def gen(**kw):
        bf.manual_seed(SEED)
        with torch.no_grad():
            return sample_generate(bmodel, ids, samples=S, max_new_tokens=n, **kw)

    c0 = dict(ops.MOE_CALLS)
    plain = gen()
    assert ops.MOE_CALLS["sample"] - c0["sample"] == 2 * n  # every forward draws both layers' weights again
    assert plain.sequences.shape == (2, T0 + n) and torch.isfinite(plain.token_prob).all()
    c0 = dict(ops.MOE_CALLS)
    kept = gen(keep_weights=True)
    assert ops.MOE_CALLS["sample"] - c0["sample"] == 2  # ... inside keep_weights=True each layer draws once
    assert ops.MOE_CALLS["gate_up"] - c0["gate_up"] == 2 * n and ops.MOE_CALLS["composite_fwd"] == c0["composite_fwd"]
    _same(kept, plain, log_probs=False)  # the same draws: the same text and statistics
    static = gen(static_cache=True, keep_weights=True)
    c0 = dict(ops.MOE_CALLS)
    graphed = gen(graph=True, keep_weights=True)
    # the prefill, the eager warm-up step and the capture: the other steps are replays with no host in them
    assert ops.MOE_CALLS["gate_up"] - c0["gate_up"] == 2 * 3 and ops.MOE_CALLS["composite_fwd"] == c0["composite_fwd"]
    _same(graphed, static)
    assert torch.equal(graphed.sequences, kept.sequences)
    for f in ("predictive_entropy", "expected_entropy", "mutual_information"):  # tests/test_gpu_generate_graph.py's tolerance
        assert (getattr(graphed, f) - getattr(kept, f)).abs().max().item() < 0.05, f
    assert torch.equal(graphed.log_prior, kept.log_prior)
    fresh = gen(graph=True)  # without kept weights the captured step samples too
    assert torch.equal(fresh.sequences, plain.sequences)
    with torch.no_grad(), pytest.raises(ValueError, match="Experts"):
        sample_generate(bmodel, ids, samples=S, max_new_tokens=n, keep_weights="fp8")
