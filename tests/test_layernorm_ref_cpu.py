"""Host side of tests/test_gpu_layernorm.py (no GPU): the float64 restatement of tests/layernorm_ref.py against torch's
layer_norm, float64 autograd and HF BertEmbeddings run in float64; the bounds of test_gpu_layernorm.py admit a correct fp32
implementation (torch's own layer_norm and autograd, rounded to each dtype) on every input the GPU tests use, and reject
eight subtly wrong ones."""
import itertools

import pytest
import torch
import torch.nn.functional as F

import test_gpu_layernorm as G
from layernorm_ref import add_layernorm_bwd_ref, add_layernorm_ref, dropout_product_ref, embed_layernorm_ref


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


# ------------------------------------------------------------------------------ the restatement is torch's arithmetic
def test_reference_equals_torch_layer_norm_and_autograd_in_float64():
    """Only reassociation separates the restatement from layer_norm and its autograd in float64 (1e-11 relative: the
    large-mean rows lose four digits to z - mean in either)."""
    gen = torch.Generator().manual_seed(31)
    for family, (rows, N), eps in itertools.product(G.FAMILIES, ((5, 8), (3, 200), (4, 520)), G.EPS):
        c = G.make_case(family, rows, N, torch.float32)
        keep = (torch.rand(rows, N, generator=gen) > 0.3).double()
        for res, kp, two in itertools.product((c.r, None), (None, keep), (False, True)):
            scale = 1.0 / 0.7 if kp is not None else 1.0
            x, g, b = (t.double().requires_grad_(True) for t in (c.x, c.gamma, c.beta))
            r = (res.double() if res is not None else torch.zeros(rows, N, dtype=torch.float64)).requires_grad_(True)
            z = (x * kp * scale if kp is not None else x) + r
            y = F.layer_norm(z, (N,), g, b, eps)
            dy = c.dy.double() + (c.dy2.double() if two else 0.0)
            y.backward(dy)
            y64, cond = add_layernorm_ref(c.x, res, c.gamma, c.beta, eps, kp, scale)
            dz, dx, dgamma, dbeta, m = add_layernorm_bwd_ref(c.x, res, c.gamma, c.dy, eps, c.dy2 if two else None, kp, scale)
            assert _rel(y64, y.detach()) < 1e-11
            assert _rel(dz, r.grad) < 1e-9 and _rel(dx, x.grad) < 1e-9, (family, rows, N, eps)
            assert _rel(dgamma, g.grad) < 1e-9 and _rel(dbeta, b.grad) < 1e-12
            assert y64.dtype == cond.dtype == dz.dtype == dgamma.dtype == torch.float64
            assert bool((cond >= (y64 - c.beta.double()).abs() * (1 - 1e-12)).all())  # the magnitude before cancellation
            assert bool((m.zmag >= m.zh * (1 - 1e-12)).all())


def test_embedding_reference_equals_hf_bert_embeddings_in_float64():
    transformers = pytest.importorskip("transformers")
    from transformers.models.bert.modeling_bert import BertEmbeddings

    N = 40
    cfg = transformers.BertConfig(vocab_size=G.EMBED_VOCAB, hidden_size=N, type_vocab_size=G.EMBED_TYPES,
                                  max_position_embeddings=G.EMBED_POS, layer_norm_eps=1e-5, hidden_dropout_prob=0.0,
                                  pad_token_id=0)
    torch.manual_seed(5)
    emb = BertEmbeddings(cfg).double().eval()
    with torch.no_grad():
        emb.LayerNorm.weight.copy_(1.0 + 0.1 * torch.randn(N))
        emb.LayerNorm.bias.copy_(0.1 * torch.randn(N))
    c = G.make_embed_case(N, torch.float32)
    tables = (emb.word_embeddings.weight.detach(), emb.token_type_embeddings.weight.detach(), emb.position_embeddings.weight.detach())
    for form, type_ids, pos_ids in G.embed_id_forms(c):
        with torch.no_grad():
            hf = emb(input_ids=c.ids, token_type_ids=type_ids if type_ids is not None else torch.zeros_like(c.ids),
                     position_ids=pos_ids)
        y64, cond = embed_layernorm_ref(c.ids, type_ids, pos_ids, *tables, emb.LayerNorm.weight.detach(),
                                        emb.LayerNorm.bias.detach(), 1e-5, G.EMBED_L)
        assert y64.shape == hf.shape == (G.EMBED_B, G.EMBED_L, N) and _rel(y64, hf) < 1e-12, form
        assert bool((cond >= (y64 - emb.LayerNorm.bias.detach()).abs() * (1 - 1e-12)).all())
    ids = c.ids.clone()
    ids[2, 1] = G.EMBED_VOCAB
    y64, cond = embed_layernorm_ref(ids, None, None, *tables, emb.LayerNorm.weight.detach(), emb.LayerNorm.bias.detach(), 1e-5, G.EMBED_L)
    nan = torch.isnan(y64).all(-1)
    assert int(nan.sum()) == 1 and bool(nan[2, 1]) and bool(torch.isnan(cond[2, 1]).all()) and bool(torch.isfinite(y64[~nan]).all())


def test_multipliers_follow_the_dispatch():
    """K and KR as the docstring of test_gpu_layernorm.py derives them, at the widths where the dispatch changes kernel."""
    assert [G.fwd_lane_adds(N) for N in (8, 256, 504, 512, 520, 768, 1024, 1032, 2048, 2056, 4096, 4104, 8192)] == \
        [8, 8, 8, 16, 16, 24, 32, 32, 32, 64, 64, 128, 128]
    assert [G.bwd_lane_adds(N) for N in (8, 512, 520, 1024, 1032, 2048, 2056, 4096)] == [8, 8, 16, 16, 32, 32, 64, 64]
    assert G.K_of(8) == 32 and G.K_of(24) == 56 and G.K_of(128) == 212
    assert [G.KR_of(r) for r in (1, 5, 37, 4096, 4097, 8195)] == [72, 72, 72, 87, 88, 89]


# ------------------------------------------------------------------------------------------- an fp32 implementation
MUTATIONS = ("one_pass_variance", "n_minus_1", "eps_after_sqrt", "eps_dropped", "zh_s2_dropped", "mean_before_gamma",
             "dgamma_unnormalised", "scale_on_residual")


def chain32(c, gdt, has_res, eps, keep, scale, two, dtype, mutation=None):
    """The formulas of layernorm_ref.py evaluated in fp32 with torch ops, results rounded to `dtype` (the parameter
    gradients stay fp32): (y, dz, dx, dgamma, dbeta).  `mutation` names one deliberate mistake."""
    f32 = torch.float32
    x, g, b = c.x.to(f32), c.gamma.to(gdt).to(f32), c.beta.to(gdt).to(f32)
    r = c.r.to(f32) if has_res else torch.zeros_like(x)
    N = x.shape[-1]
    ks = keep.to(f32) * torch.tensor(scale, dtype=f32) if keep is not None else None
    z = x * ks if ks is not None else x
    z = (x * keep.to(f32) + r) * torch.tensor(scale, dtype=f32) if (mutation == "scale_on_residual" and ks is not None) else z + r
    mean = z.sum(-1, keepdim=True) / N
    d = z - mean
    if mutation == "one_pass_variance":
        var = (z * z).sum(-1, keepdim=True) / N - mean * mean
    elif mutation == "n_minus_1":
        var = (d * d).sum(-1, keepdim=True) / (N - 1)
    else:
        var = (d * d).sum(-1, keepdim=True) / N
    e = torch.tensor(eps, dtype=f32)
    if mutation == "eps_after_sqrt":
        rstd = 1.0 / (torch.sqrt(var) + e)
    elif mutation == "eps_dropped":
        rstd = 1.0 / torch.sqrt(var)
    else:
        rstd = 1.0 / torch.sqrt(var + e)
    zh = d * rstd
    y = zh * g + b
    gy = c.dy.to(f32) + c.dy2.to(f32) if two else c.dy.to(f32)
    a = gy * g
    s1 = a.sum(-1, keepdim=True) / N
    if mutation == "mean_before_gamma":
        s1 = gy.sum(-1, keepdim=True) / N * g
    s2 = (a * zh).sum(-1, keepdim=True) / N
    dz = rstd * (a - s1 - (0.0 if mutation == "zh_s2_dropped" else zh * s2))
    dx = dz * ks if ks is not None else dz
    dgamma = (gy * (d if mutation == "dgamma_unnormalised" else zh)).sum(0)
    return y.to(dtype), dz.to(dtype), dx.to(dtype), dgamma, gy.sum(0)


def torch32(c, gdt, has_res, eps, keep, scale, two, dtype):
    """torch's own fp32 layer_norm and autograd on the same inputs, rounded to `dtype`."""
    f32 = torch.float32
    x, g, b = (t.clone().requires_grad_(True) for t in (c.x.to(f32), c.gamma.to(gdt).to(f32), c.beta.to(gdt).to(f32)))
    r = (c.r.to(f32).clone() if has_res else torch.zeros_like(x)).requires_grad_(True)
    z = (x * (keep.to(f32) * torch.tensor(scale, dtype=f32)) if keep is not None else x) + r
    y = F.layer_norm(z, (x.shape[-1],), g, b, eps)
    y.backward(c.dy.to(f32) + c.dy2.to(f32) if two else c.dy.to(f32))
    return y.detach().to(dtype), r.grad.to(dtype), x.grad.to(dtype), g.grad, b.grad


def ratios(outs, c, gdt, has_res, eps, keep, scale, two, dtype, K_fwd):
    """{output: (within the bound and finite, worst error / bound)} of an implementation's five results."""
    res = c.r if has_res else None
    g, b = c.gamma.to(gdt), c.beta.to(gdt)
    y64, cond = add_layernorm_ref(c.x, res, g, b, eps, keep, scale)
    prod = dropout_product_ref(c.x, res, g, eps, keep, scale) if keep is not None else None
    bounds = {"y": (y64, G.fwd_bound(y64, cond, K_fwd, dtype, prod))}
    if len(outs) > 1:
        dz64, dx64, dg64, db64, m = add_layernorm_bwd_ref(c.x, res, g, c.dy, eps, c.dy2 if two else None, keep, scale)
        b_dz, b_dx, b_dg, b_db = G.bwd_bounds(dz64, dx64, m, G.K_of(G.bwd_lane_adds(c.N)), G.KR_of(c.rows), dtype)
        bounds.update({"dz": (dz64, b_dz), "dx": (dx64, b_dx), "dgamma": (dg64, b_dg), "dbeta": (db64, b_db)})
    return {k: G.worst_ratio(got, *bounds[k])[:2] for k, got in zip(bounds, outs)}


def _mask(rows, N, p):
    return G.keep_mask(rows, N, p) if p else (None, 1.0)


def _some(configs, i, n):
    """n of the configurations, a different selection for every i: over the inputs each one has its turn."""
    step = max(1, len(configs) // n)
    return [configs[(i + j * step) % len(configs)] for j in range(n)]


@pytest.mark.parametrize("name", list(G.DTYPES))
def test_bounds_admit_the_fp32_torch_chain(name):
    """torch's fp32 layer_norm and autograd, rounded to the dtype, stay below error / bound 1.0 on every input of the GPU
    tests: forward and dropout shapes with the forward's K, backward shapes with the backward's K and KR.  Every input
    (family x shape x dtype) is run; of the crossed settings (gamma dtype, residual, eps, dropout, two gradients) each
    input takes a few, in rotation."""
    dtype = G.DTYPES[name]
    worst, i = {}, 0
    for family in G.FAMILIES:
        shapes = [(rows, N, 0.0) for N in G.FWD_WIDTHS for rows in G.FWD_ROWS]
        shapes += [(rows, N, p) for p in G.DROP_P for N in G.DROP_WIDTHS for rows in G.DROP_ROWS]
        for rows, N, p in shapes:
            c = G.make_case(family, rows, N, dtype)
            keep, scale = _mask(rows, N, p)
            for gdt, has_res, eps in _some(G.fwd_configs(dtype), i, 2):
                i += 1
                args = (c, gdt, has_res, eps, keep, scale, False, dtype)
                ok, w = ratios(torch32(*args)[:1], *args, G.K_of(G.fwd_lane_adds(N)))["y"]
                assert ok, ("y", family, rows, N, gdt, has_res, eps, p, w)
                worst["y"] = max(worst.get("y", 0.0), w)
        for rows, N in G.BWD_SHAPES:
            c = G.make_case(family, rows, N, dtype)
            for gdt, has_res, eps, p, two in _some(G.bwd_configs(dtype, family), i, 3):
                i += 1
                keep, scale = _mask(rows, N, p)
                args = (c, gdt, has_res, eps, keep, scale, two, dtype)
                got = ratios(torch32(*args), *args, G.K_of(G.bwd_lane_adds(N)))
                for k in ("dz", "dx", "dgamma", "dbeta"):
                    assert got[k][0], (k, family, rows, N, gdt, has_res, eps, p, two, got[k][1])
                    worst[k] = max(worst.get(k, 0.0), got[k][1])
    print(f"[fp32 torch chain {name}] worst error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("name", list(G.DTYPES))
def test_bounds_admit_the_fp32_embedding_chain(name):
    """torch's embedding lookups added in fp32 and its fp32 layer_norm, on every table, id form, gamma dtype and eps of the
    GPU test."""
    dtype = G.DTYPES[name]
    worst = 0.0
    for N, scale in itertools.product(G.EMBED_WIDTHS, G.EMBED_SCALES):
        c = G.make_embed_case(N, dtype, scale)
        for gdt, eps in G.param_configs(dtype):
            g, b = c.gamma.to(gdt), c.beta.to(gdt)
            for form, type_ids, pos_ids in G.embed_id_forms(c):
                ti = type_ids if type_ids is not None else torch.zeros_like(c.ids)
                pi = pos_ids if pos_ids is not None else torch.arange(G.EMBED_L)[None]
                z = (c.word.float()[c.ids] + c.typ.float()[ti]) + c.pos.float()[pi.expand_as(c.ids)]
                y = F.layer_norm(z, (N,), g.float(), b.float(), eps).to(dtype)
                y64, cond = embed_layernorm_ref(c.ids, type_ids, pos_ids, c.word, c.typ, c.pos, g, b, eps, G.EMBED_L)
                ok, w, at = G.worst_ratio(y, y64, G.fwd_bound(y64, cond, G.K_of(G.bwd_lane_adds(N)) + 2, dtype))
                assert ok, (N, scale, gdt, eps, form, at, w)
                worst = max(worst, w)
    # and the tiny tables are what makes the place of eps visible: eps added after the square root breaks the bound there
    c = G.make_embed_case(520, dtype, 1e-3)
    z = (c.word.float()[c.ids] + c.typ.float()[c.type_ids]) + c.pos.float()[c.pos_bl]
    d = z - z.mean(-1, keepdim=True)
    wrong = (d / (torch.sqrt((d * d).mean(-1, keepdim=True)) + 1e-5) * c.gamma + c.beta).to(dtype)
    y64, cond = embed_layernorm_ref(c.ids, c.type_ids, c.pos_bl, c.word, c.typ, c.pos, c.gamma, c.beta, 1e-5, G.EMBED_L)
    assert not G.worst_ratio(wrong, y64, G.fwd_bound(y64, cond, G.K_of(G.bwd_lane_adds(520)) + 2, dtype))[0]
    print(f"[fp32 embedding chain {name}] worst error / bound {worst:.3f}")


# (mutation, the input family of the GPU tests that exposes it, the output that breaks its bound, dropout)
REJECTED = (("one_pass_variance", "large_mean", "y", 0.0), ("n_minus_1", "plain", "y", 0.0), ("eps_after_sqrt", "tiny", "y", 0.0),
            ("eps_dropped", "zero_row", "y", 0.0), ("zh_s2_dropped", "plain", "dz", 0.0), ("mean_before_gamma", "plain", "dz", 0.0),
            ("dgamma_unnormalised", "plain", "dgamma", 0.0), ("scale_on_residual", "plain", "y", 0.1))


@pytest.mark.parametrize("mutation,family,output,p", REJECTED)
def test_bounds_reject_a_subtly_wrong_implementation(mutation, family, output, p):
    """Each mistake, made in the fp32 chain that the bounds admit when it is right, breaks the named output's bound on the
    named family in EVERY dtype, on inputs, settings and eps of the GPU test of that output: the forward's (7 rows; with
    dropout at its widths) for y, the backward's (5 rows) for the gradients."""
    assert set(m for m, _, _, _ in REJECTED) == set(MUTATIONS)
    forward = output == "y"
    rows, widths = (7, (200, 520, 768) if p else (8, 200, 768)) if forward else (5, (8, 200, 768))
    assert rows in (G.DROP_ROWS if p else G.FWD_ROWS if forward else (5,))
    assert set(widths) <= set(G.DROP_WIDTHS if p else G.FWD_WIDTHS if forward else G.BWD_WIDTHS)
    for name, dtype in G.DTYPES.items():
        caught = []
        for N in widths:
            c = G.make_case(family, rows, N, dtype)
            keep, scale = _mask(rows, N, p)
            for eps in (G.EPS if forward else G.eps_set(dtype, family)):
                args = (c, torch.float32, True, eps, keep, scale, False, dtype)
                K = G.K_of(G.fwd_lane_adds(N))
                cut = slice(0, 1) if forward else slice(None)
                assert all(ok for ok, _ in ratios(chain32(*args)[cut], *args, K).values()), (name, N, eps)
                ok, w = ratios(chain32(*args, mutation=mutation)[cut], *args, K)[output]
                if not ok:
                    caught.append((N, eps, round(w, 2)))
        assert caught, (mutation, family, output, name)
        print(f"[{mutation} / {family} / {name}] {output} breaks its bound at (N, eps, error / bound) {caught}")
