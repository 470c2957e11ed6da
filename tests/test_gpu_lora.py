"""Bayesian LoRA on the device: bf_lora_fwd / bf_lora_bwd against float64 (tests/lora_ref.py), their refusals, bnn.LoRALinear
(log-probs, output, gradients, KL gradient, checkpoint recomputation) and a converted tiny Llama through sample_bayesian,
training_step and sample_generate.  Bounds: one rounding to the output type is 2^-7 (bf16) / 2^-10 (fp16) of max |ref|
(tests/test_gpu_backward.py); an fp32 output of 16-bit operands 2^-8 / 2^-11 of max |ref| plus 1e-5 sqrt(contraction length)
(tests/test_gpu_kept_weights.py).  The end-to-end bounds are measured per run: twice the error the framework's own 16-bit
ops make on the same formula and the same A_s, never below the one-rounding bound."""
import copy
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lora_ref  # noqa: E402

import bayeformers_amd as bf  # noqa: E402
import bayeformers_amd.nn as bnn  # noqa: E402
from bayeformers_amd import _C, ops  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 0xB10B
ROUND = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}
ACC32 = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
SHAPES = [(1, 1, 64, 64, 8), (3, 5, 200, 136, 16), (2, 64, 256, 512, 64), (3, 130, 264, 192, 24)]
DTYPES = [torch.bfloat16, torch.float16]


def _err(got, ref):
    return (got.double().cpu() - ref.double().cpu()).abs().max().item()


def _operands(S, M, N, K, r, dt, seed=1):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(S * M, K, generator=g).to(dt).cuda()
    a_s = (0.2 * torch.randn(S, r, K, generator=g)).to(dt).cuda()
    b = (0.3 * torch.randn(N, r, generator=g)).cuda()
    y_in = torch.randn(S * M, N, generator=g).to(dt).cuda()
    dy = torch.randn(S * M, N, generator=g).to(dt).cuda()
    dx_in = torch.randn(S * M, K, generator=g).to(dt).cuda()
    return x, a_s, b, y_in, dy, dx_in


# ------------------------------------------------------------------------------------------------------ 1. bf_lora_fwd
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("S,M,N,K,r", SHAPES)
def test_lora_fwd_against_fp64(S, M, N, K, r, dt):
    scale = 2.0
    x, a_s, b, y_in, _, _ = _operands(S, M, N, K, r, dt)
    y = y_in.clone()
    h = ops.lora_fwd(x, a_s, b, y, scale, S)
    h_ref = torch.bmm(x.double().view(S, M, K), a_s.double().transpose(1, 2)).view(S * M, r)
    eh = _err(h, h_ref)
    y_ref = y_in.double() + scale * (h.double().view(S, M, r) @ b.to(dt).double().t()).view(S * M, N)
    ey = _err(y, y_ref)
    print(f"lora_fwd {dt} {(S, M, N, K, r)}: h err {eh:.3e} (bound {ROUND[dt] * h_ref.abs().max().item():.3e}), "
          f"y err {ey:.3e} (bound {ROUND[dt] * y_ref.abs().max().item():.3e})")
    assert h.dtype == dt and eh <= ROUND[dt] * h_ref.abs().max().item()
    assert ey <= ROUND[dt] * y_ref.abs().max().item()
    y2 = y_in.clone()
    h2 = ops.lora_fwd(x, a_s, b, y2, scale, S)
    assert torch.equal(y2, y) and torch.equal(h2, h)  # no atomics: the same bits
    y0 = y_in.clone()
    ops.lora_fwd(x, a_s, torch.zeros_like(b), y0, scale, S)
    assert torch.equal(y0, y_in)  # B = 0: the base product passes through untouched


# ------------------------------------------------------------------------------------------------------ 2. bf_lora_bwd
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("S,M,N,K,r", SHAPES)
def test_lora_bwd_against_fp64(S, M, N, K, r, dt):
    scale = 2.0
    x, a_s, b, _, dy, dx_in = _operands(S, M, N, K, r, dt)
    h = ops.lora_fwd(x, a_s, b, None, scale, S)
    dx = dx_in.clone()
    da, db = ops.lora_bwd(x, dy, a_s, b, h, dx, scale, S)
    b16 = b.to(dt).double()
    g16 = (dy.double().view(S, M, N) @ b16).to(dt).double()  # g as the kernel keeps it: rounded to the compute dtype
    dx_ref = dx_in.double() + scale * torch.bmm(g16, a_s.double()).view(S * M, K)
    da_ref = scale * torch.bmm(g16.transpose(1, 2), x.double().view(S, M, K))
    db_ref = scale * (dy.double().t() @ h.double())
    edx, eda, edb = _err(dx, dx_ref), _err(da, da_ref), _err(db, db_ref)
    bdx = ROUND[dt] * dx_ref.abs().max().item()
    bda = ACC32[dt] * da_ref.abs().max().item() + 1e-5 * M ** 0.5
    bdb = ACC32[dt] * db_ref.abs().max().item() + 1e-5 * (S * M) ** 0.5
    print(f"lora_bwd {dt} {(S, M, N, K, r)}: dx err {edx:.3e} (bound {bdx:.3e}), dA err {eda:.3e} (bound {bda:.3e}), "
          f"dB err {edb:.3e} (bound {bdb:.3e})")
    assert da.dtype == torch.float32 and da.shape == (S, r, K) and db.shape == (N, r)
    assert edx <= bdx and eda <= bda and edb <= bdb
    dx2 = dx_in.clone()
    da2, db2 = ops.lora_bwd(x, dy, a_s, b, h, dx2, scale, S)
    assert torch.equal(dx2, dx) and torch.equal(da2, da) and torch.equal(db2, db)
    da3, db3 = ops.lora_bwd(x, dy, a_s, b, h, None, scale, S)  # dx = NULL
    assert torch.equal(da3, da) and torch.equal(db3, db)
    dx4 = dx_in.clone()
    da4, db4 = ops.lora_bwd(x, dy, a_s, b, h, dx4, scale, S, need_db=False)  # dB = NULL
    assert db4 is None and torch.equal(da4, da) and torch.equal(dx4, dx)


# --------------------------------------------------------------------------------------------------------- 3. refusals
@pytest.mark.parametrize("N,K,r,word", [(64, 64, 12, "r % 8 == 0"), (64, 60, 8, "K % 8 == 0"), (64, 64, 72, "8 <= r <= 64")])
def test_refusals_name_the_condition(N, K, r, word):
    dt = torch.bfloat16
    x = torch.zeros(4, K, dtype=dt, device="cuda")
    a_s = torch.zeros(2, r, K, dtype=dt, device="cuda")
    b = torch.zeros(N, r, device="cuda")
    y = torch.zeros(4, N, dtype=dt, device="cuda")
    with pytest.raises(_C.BayeFormersAMDError) as e:
        ops.lora_fwd(x, a_s, b, y, 1.0, 2)
    assert "bf_lora_fwd" in str(e.value) and word in str(e.value)
    with pytest.raises(_C.BayeFormersAMDError) as e:
        ops.lora_bwd(x, y, a_s, b, torch.zeros(4, r, dtype=dt, device="cuda"), None, 1.0, 2)
    assert "bf_lora_bwd" in str(e.value) and word in str(e.value)
    assert not ops.lora_supported(dt, N, K, r, x, a_s, b, y)
    assert ops.lora_supported(dt, 64, 64, 8)
    assert not ops.lora_supported(torch.float32, 64, 64, 8)


# ------------------------------------------------------------------------------------------------------------ 4. layer
def _layer(K, N, r, alpha, dt, bias=True, b_std=0.3):
    torch.manual_seed(4)
    lin = torch.nn.Linear(K, N, bias=bias)
    layer = bnn.LoRALinear.from_frequentist(lin, r=r, alpha=alpha)
    with torch.no_grad():
        layer.lora_B.normal_(0.0, b_std)
    model = bnn.Model(layer).cuda().to(dt)
    bf.set_compute_dtype("bf16" if dt == torch.bfloat16 else "fp16")
    return model, model.model


@pytest.fixture
def _restore_dtype():
    prev = bf.get_compute_dtype()
    yield
    bf.set_compute_dtype({torch.float32: "fp32", torch.bfloat16: "bf16", torch.float16: "fp16"}[prev])
    bf.set_kl_gradient(False)


def test_default_routes_follow_the_measurement():
    """profiles/bayesian_lora.md: the forward kernel at r = 16, the composite at r = 64 and for every backward."""
    assert ops.lora_kernel_wins(16, False) and not ops.lora_kernel_wins(64, False) and not ops.lora_kernel_wins(16, True)
    assert ops.lora_supported(torch.bfloat16, 64, 64, 16, backward=False)
    assert not ops.lora_supported(torch.bfloat16, 64, 64, 64, backward=False)
    assert not ops.lora_supported(torch.bfloat16, 64, 64, 16, backward=True)
    assert ops.lora_supported(torch.bfloat16, 64, 64, 64)  # the kernels' class itself


@pytest.mark.parametrize("dt", DTYPES)
def test_layer_forward_and_backward_against_reference(dt, _restore_dtype, monkeypatch):
    S, M, K, N, r, alpha = 3, 5, 136, 200, 16, 32
    monkeypatch.setattr(ops, "lora_kernel_wins", lambda r, backward: True)  # both directions on the kernels
    model, layer = _layer(K, N, r, alpha, dt)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(M, K, generator=g).to(dt).cuda()
    dy = torch.randn(S * M, N, generator=g).to(dt).cuda()
    bf.manual_seed(SEED, next_sample=5)
    k0 = dict(ops.LORA_CALLS)
    xin = x.repeat(S, 1).requires_grad_(True)
    with model.monte_carlo(S):
        y = model(xin)
    assert ops.LORA_CALLS["fwd"] == k0["fwd"] + 1 and ops.LORA_CALLS["composite_fwd"] == k0["composite_fwd"]
    base, seed, sid = model._last_base, bf.random.STATE.seed, 2 * layer.layer_id
    assert base == 5
    (a16,), lp = ops.sample_logprob([layer.lora_A], [layer.lora_A_prior], [sid], S, seed, base, out_dtype=dt)
    assert torch.equal(model.log_prob_samples(), lp) and torch.equal(layer.log_prob_samples, lp)
    y.backward(dy)
    assert ops.LORA_CALLS["bwd"] == k0["bwd"] + 1

    # float64 reference on A_s from the host twin of the generator
    mu, rho, b = layer.lora_A.mu.detach().cpu(), layer.lora_A.rho.detach().cpu(), layer.lora_B.detach().cpu()
    w0, b0 = layer.base_weight.detach().cpu(), layer.base_bias.detach().cpu()
    eps = lora_ref.eps_host((r, K), seed, base, S, sid)
    a64 = lora_ref.sample_a(mu, rho, eps)
    assert _err(a16, a64) <= ROUND[dt] / 2 * a64.abs().max().item()  # the device draw, rounded once
    xs = xin.detach().cpu()
    y_ref, _ = lora_ref.forward(xs, a64, b, w0, b0, layer.scale, S)
    ref = lora_ref.backward(xs, dy.cpu(), a64, b, w0, layer.scale, S, eps, rho)

    # the same formula on the framework's 16-bit ops and the same A_s: the measure of what 16 bits cost here
    xd, b16, sc = xin.detach(), layer.lora_B.detach().to(dt), layer.scale
    h_c = torch.bmm(xd.view(S, M, K), a16.transpose(1, 2))
    y_c = torch.nn.functional.linear(xd, layer.base_weight, layer.base_bias).view(S, M, N) + sc * (h_c @ b16.t())
    g_c = dy.view(S, M, N) @ b16
    dx_c = (dy @ layer.base_weight).view(S, M, K) + sc * torch.bmm(g_c, a16)
    da_c = sc * torch.bmm(g_c.transpose(1, 2), xd.view(S, M, K)).float()
    db_c = sc * (dy.t() @ h_c.reshape(S * M, r)).float()
    dmu_c = da_c.sum(0)
    drho_c = (da_c * eps.float().cuda()).sum(0) * torch.sigmoid(layer.lora_A.rho.detach())

    def check(name, got, comp, want, floor):
        e_k, e_c = _err(got, want), _err(comp.reshape(want.shape), want)
        bound = max(2.0 * e_c, floor)
        print(f"layer {dt} {name}: kernel err {e_k:.3e}, framework 16-bit err {e_c:.3e}, bound {bound:.3e}")
        assert e_k <= bound, name

    check("y", y, y_c, y_ref, ROUND[dt] * y_ref.abs().max().item())
    check("dx", xin.grad, dx_c, ref["dx"], ROUND[dt] * ref["dx"].abs().max().item())
    check("dmu_A", layer.lora_A.mu.grad, dmu_c, ref["dmu"], ACC32[dt] * ref["dmu"].abs().max().item() + 1e-5 * (S * M) ** 0.5)
    check("drho_A", layer.lora_A.rho.grad, drho_c, ref["drho"],
          ACC32[dt] * ref["drho"].abs().max().item() + 1e-5 * (S * M) ** 0.5)
    check("dB", layer.lora_B.grad, db_c, ref["dB"], ACC32[dt] * ref["dB"].abs().max().item() + 1e-5 * (S * M) ** 0.5)
    assert layer.base_weight.grad is None and layer.base_bias.grad is None  # there is no dW0


def test_layer_with_zero_b_is_the_base_projection(_restore_dtype):
    dt = torch.bfloat16
    model, layer = _layer(136, 200, 16, 32, dt, b_std=0.0)
    assert not layer.lora_B.any()
    x = torch.randn(7, 136, device="cuda").to(dt)
    with torch.no_grad():
        y = layer(x)  # bare: S = 1, a private log-prob slot
        base = ops.lora_base_forward(x, layer.base_weight, layer._bias32())
    assert torch.equal(y, base)
    assert layer.log_prob_samples.shape == (1, 2) and torch.isfinite(layer.log_prob_samples).all()
    ref = torch.nn.functional.linear(x.double(), layer.base_weight.double(), layer.base_bias.double())
    assert _err(y, ref) <= ROUND[dt] * ref.abs().max().item()


def test_layer_unsupported_shapes_run_the_composite(_restore_dtype):
    """fp32 compute and r % 8 != 0 run the framework composite of the same formula on the A_s the kernel drew."""
    S, M, K, N, r = 2, 3, 40, 24, 4
    torch.manual_seed(1)
    layer = bnn.LoRALinear.from_frequentist(torch.nn.Linear(K, N), r=r, alpha=8)
    with torch.no_grad():
        layer.lora_B.normal_(0.0, 0.3)
    model = bnn.Model(layer).cuda()
    bf.set_compute_dtype("fp32")
    x = torch.randn(M, K, device="cuda")
    bf.manual_seed(SEED)
    k0 = dict(ops.LORA_CALLS)
    xin = x.repeat(S, 1).requires_grad_(True)
    with model.monte_carlo(S):
        y = model(xin)
    dy = torch.randn_like(y)
    y.backward(dy)
    assert ops.LORA_CALLS["composite_fwd"] == k0["composite_fwd"] + 1 and ops.LORA_CALLS["fwd"] == k0["fwd"]
    assert ops.LORA_CALLS["composite_bwd"] == k0["composite_bwd"] + 1
    base, seed, sid = model._last_base, bf.random.STATE.seed, 2 * layer.layer_id
    eps = lora_ref.eps_host((r, K), seed, base, S, sid)
    rho = layer.lora_A.rho.detach().cpu()
    a64 = lora_ref.sample_a(layer.lora_A.mu.detach().cpu(), rho, eps)
    w0 = layer.base_weight.detach().cpu()
    y_ref, _ = lora_ref.forward(xin.detach().cpu(), a64, layer.lora_B.detach().cpu(), w0, layer.base_bias.detach().cpu(),
                                layer.scale, S)
    ref = lora_ref.backward(xin.detach().cpu(), dy.cpu(), a64, layer.lora_B.detach().cpu(), w0, layer.scale, S, eps, rho)
    for name, got, want in (("y", y, y_ref), ("dx", xin.grad, ref["dx"]), ("dmu", layer.lora_A.mu.grad, ref["dmu"]),
                            ("drho", layer.lora_A.rho.grad, ref["drho"]), ("dB", layer.lora_B.grad, ref["dB"])):
        assert _err(got, want) <= 2e-5 * max(1.0, want.abs().max().item()), name  # fp32 arithmetic end to end


def test_layer_kl_gradient_is_kl_grad(_restore_dtype):
    dt = torch.bfloat16
    S = 3
    model, layer = _layer(64, 64, 8, 16, dt)
    x = torch.randn(4, 64, device="cuda").to(dt)
    bf.set_kl_gradient(True)
    bf.manual_seed(SEED)
    with model.monte_carlo(S):
        model(x.repeat(S, 1))
    w = torch.tensor([[0.5, -1.0], [2.0, 0.25], [-0.75, 1.5]], dtype=torch.float64, device="cuda")
    lp = model.log_prob_samples()
    assert lp.requires_grad
    (lp * w).sum().backward()
    dmu, drho = ops.kl_grad(layer.lora_A, layer.lora_A_prior, 2 * layer.layer_id, S, bf.random.STATE.seed, model._last_base, w, True)
    assert torch.equal(layer.lora_A.mu.grad, dmu) and torch.equal(layer.lora_A.rho.grad, drho)
    assert layer.lora_B.grad is None


def test_layer_under_reentrant_checkpoint_gives_the_same_bits(_restore_dtype, monkeypatch):
    from torch.utils.checkpoint import checkpoint

    monkeypatch.setattr(ops, "lora_kernel_wins", lambda r, backward: True)  # both directions on the kernels

    dt = torch.bfloat16
    S, M, K, N, r = 3, 5, 136, 200, 16

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a, self.b = torch.nn.Linear(K, N), torch.nn.Linear(N, K)
            self.ckpt = False

        def block(self, x):
            return self.b(torch.tanh(self.a(x)))

        def forward(self, x):
            return checkpoint(self.block, x, use_reentrant=True) if self.ckpt else self.block(x)

    torch.manual_seed(0)
    model = bf.to_bayesian_lora(Net(), r=r, alpha=32, target_modules=("a", "b"))
    for m in model.modules():
        if isinstance(m, bnn.LoRALinear):
            with torch.no_grad():
                m.lora_B.normal_(0.0, 0.3)
    model = model.cuda().to(dt)
    bf.set_compute_dtype("bf16")
    x = torch.randn(M, K, device="cuda").to(dt)
    dy = torch.randn(S * M, K, device="cuda").to(dt)

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
    assert g0.keys() == g1.keys() and len(g0) == 7
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n


# ------------------------------------------------------------------------------------------------------------ 5. model
def _tiny_llama_src():
    from transformers import LlamaConfig, LlamaForCausalLM

    cfg = LlamaConfig(hidden_size=256, num_attention_heads=4, num_key_value_heads=2, num_hidden_layers=2,
                      intermediate_size=512, vocab_size=256, max_position_embeddings=128, tie_word_embeddings=False,
                      attention_dropout=0.0, attn_implementation="sdpa")
    torch.manual_seed(0)
    return LlamaForCausalLM(cfg).eval()


def _to16(model, dt):
    """model.to(dt) with the rotary frequencies kept in fp32 (as tests/test_gpu_kept_weights.py does)."""
    freqs = {n: b.detach().clone() for n, b in model.named_buffers() if "inv_freq" in n}
    model = model.to(dt)
    for n, b in freqs.items():
        setattr(model.get_submodule(n.rsplit(".", 1)[0]), n.rsplit(".", 1)[1], b)
    return model


def _converted(src, dt=torch.bfloat16, fuse=True, backward=False):
    torch.manual_seed(7)  # (mu_A and rho_A are drawn from torch's global generator: two conversions must agree)
    bmodel = bf.to_bayesian_lora(src, r=8, alpha=16)
    g = torch.Generator().manual_seed(9)
    for m in bmodel.modules():
        if isinstance(m, bnn.LoRALinear):
            with torch.no_grad():
                m.lora_B.copy_(0.05 * torch.randn(m.lora_B.shape, generator=g))
    bmodel = _to16(bmodel.eval().cuda(), dt)
    if fuse:
        assert bf.fuse_attention(bmodel)
        assert bf.fuse_decoder_blocks(bmodel, backward=backward) == 2
    bf.set_compute_dtype("bf16" if dt == torch.bfloat16 else "fp16")
    return bmodel


def _ids(B=2, T=37, vocab=256, seed=11):
    return torch.randint(0, vocab, (B, T), generator=torch.Generator().manual_seed(seed)).cuda()


def test_model_logits_against_merged_fp32_reference(monkeypatch, _restore_dtype):
    dt, S = torch.bfloat16, 3
    src = _tiny_llama_src()
    ids = _ids()
    from bayeformers_amd.sampling import sample_bayesian

    # the unfused converted model on the framework's 16-bit ops (lora_supported -> False: the composite route)
    plain = _converted(src, dt, fuse=False)
    bf.manual_seed(SEED)
    with monkeypatch.context() as mp, torch.no_grad():
        mp.setattr(ops, "lora_supported", lambda *a, **k: False)
        k0 = ops.LORA_CALLS["fwd"]
        raw_c, _, _, _ = sample_bayesian(plain, {"input_ids": ids, "use_cache": False}, S)
        assert ops.LORA_CALLS["fwd"] == k0
    base, seed = plain._last_base, bf.random.STATE.seed
    # the kernels, fused attention and decoder blocks
    fused = _converted(src, dt, fuse=True)
    bf.manual_seed(SEED)
    k0 = dict(ops.LORA_CALLS)
    with torch.no_grad():
        raw_k, _, _, _ = sample_bayesian(fused, {"input_ids": ids, "use_cache": False}, S)
    assert ops.LORA_CALLS["fwd"] == k0["fwd"] + 14 and ops.LORA_CALLS["composite_fwd"] == k0["composite_fwd"]
    assert fused._last_base == base
    # fp32 reference: the source model (parameters as the 16-bit model holds them) with W0 + scale * B A_s merged in
    errs_k, errs_c, top = [], [], 0.0
    for s in range(S):
        ref = copy.deepcopy(src).cuda()
        ref.config._attn_implementation = "eager"
        for p in ref.parameters():
            p.data = p.data.to(dt).float()
        for n, m in fused.model.named_modules():
            if isinstance(m, bnn.LoRALinear):
                eps = lora_ref.eps_host((m.r, m.in_features), seed, base + s, 1, 2 * m.layer_id)
                a = lora_ref.sample_a(m.lora_A.mu.detach().cpu(), m.lora_A.rho.detach().cpu(), eps)[0]
                w = m.base_weight.detach().double().cpu() + m.scale * (m.lora_B.detach().double().cpu() @ a)
                ref.get_submodule(n).weight.data = w.float().cuda()
        with torch.no_grad():
            logits = ref(input_ids=ids, use_cache=False).logits.double()
        errs_k.append(_err(raw_k[0][s], logits))
        errs_c.append(_err(raw_c[0][s], logits))
        top = max(top, logits.abs().max().item())
    e_k, e_c = max(errs_k), max(errs_c)
    bound = max(2.0 * e_c, ROUND[dt] * top)
    print(f"model logits {dt}: kernel path err {e_k:.3e}, unfused framework 16-bit err {e_c:.3e}, max |logit| {top:.3f}, "
          f"bound {bound:.3e}")
    assert e_k <= bound


def test_training_steps_move_only_the_adapters(_restore_dtype):
    from bayeformers_amd import training

    bmodel = _converted(_tiny_llama_src(), torch.bfloat16, fuse=True, backward=True).train()
    ids = _ids()
    start = {n: p.detach().clone() for n, p in bmodel.named_parameters()}
    adapters = set(bf.lora_state_dict(bmodel))
    params = [p for p in bmodel.parameters() if p.requires_grad]
    assert len(params) == 3 * 14
    opt = torch.optim.AdamW(params, lr=1e-2)

    def nll(mean):
        logits = mean[0][:, :-1].float()
        return torch.nn.functional.cross_entropy(logits.reshape(-1, logits.shape[-1]), ids[:, 1:].reshape(-1))

    bf.manual_seed(SEED)
    k0 = dict(ops.LORA_CALLS)
    for _ in range(2):
        loss = training.training_step(bmodel, {"input_ids": ids, "use_cache": False}, 3, nll, opt, n_batches=10)
        assert torch.isfinite(loss)
    # (the backward runs the route ops.lora_kernel_wins gives it: today the composite)
    assert ops.LORA_CALLS["bwd"] + ops.LORA_CALLS["composite_bwd"] == k0["bwd"] + k0["composite_bwd"] + 2 * 14
    assert ops.LORA_CALLS["fwd"] == k0["fwd"] + 2 * 14
    moved = {n for n, p in bmodel.named_parameters() if not torch.equal(p.detach(), start[n])}
    lp_names = {n for n in moved if n.endswith(("log_prior", "log_variational_posterior"))}  # the layers' lazy scalars
    assert moved - lp_names == adapters
    for n, p in bmodel.named_parameters():
        if n in adapters:
            assert p.grad is not None and torch.isfinite(p.grad).all(), n
        if n.endswith("base_weight"):
            assert torch.equal(p, start[n]) and p.grad is None


# ------------------------------------------------------------------------------------------------------- 6. generation
def _same(a, b):
    import dataclasses

    for f in dataclasses.fields(a):
        assert torch.equal(getattr(a, f.name), getattr(b, f.name)), f.name


def test_generation_modes_agree(_restore_dtype):
    from bayeformers_amd.sampling import mc_predictive, sample_bayesian, sample_generate

    bmodel = _converted(_tiny_llama_src(), torch.bfloat16)
    ids = _ids()
    S, n, T0 = 3, 6, ids.shape[1]

    def gen(**kw):
        bf.manual_seed(SEED)
        with torch.no_grad():
            return sample_generate(bmodel, ids, samples=S, max_new_tokens=n, **kw)

    plain = gen()
    k0 = dict(ops.LORA_CALLS)
    s0 = ops.SKINNY_CALLS[0]
    kept = gen(keep_weights=True)
    # every decode step (S * B = 6 rows): each LoRA layer's base projection is ONE skinny launch with S = 1
    assert ops.LORA_CALLS["base_skinny"] - k0["base_skinny"] == 14 * (n - 1)
    assert ops.LORA_CALLS["base_gemm"] - k0["base_gemm"] == 14  # the prefill
    assert ops.SKINNY_CALLS[0] - s0 == 14 * (n - 1)
    _same(kept, plain)
    static = gen(static_cache=True)
    graphed = gen(graph=True)
    _same(graphed, static)
    assert torch.equal(static.sequences, plain.sequences)
    # step 0 against teacher forcing on the prompt, with tests/test_gpu_kept_weights.py's bound for this comparison
    bf.manual_seed(SEED)
    with torch.no_grad():
        raw, _, _, _ = sample_bayesian(bmodel, {"input_ids": ids, "use_cache": False}, S)
    assert torch.equal(bmodel.log_prob_samples()[:, 0], plain.log_prior)
    pred = mc_predictive(raw[0][:, :, T0 - 1:])
    assert torch.equal(pred.prediction[:, 0], plain.sequences[:, T0])
    for ours, ref in ((plain.predictive_entropy, pred.predictive_entropy), (plain.expected_entropy, pred.expected_entropy),
                      (plain.mutual_information, pred.mutual_information)):
        assert (ours[:, 0] - ref[:, 0]).abs().max().item() < 0.05
    for kw in ({"kv_cache": "fp8"}, {"prefill_chunk": 32}, {"keep_weights": "fp8"}):
        out = gen(**kw)
        for f in ("predictive_entropy", "expected_entropy", "mutual_information", "token_prob"):
            assert torch.isfinite(getattr(out, f)).all(), (kw, f)
        assert out.sequences.shape == (ids.shape[0], T0 + n)
