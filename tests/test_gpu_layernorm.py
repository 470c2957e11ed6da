"""The LayerNorm kernels of bayeformers_amd/csrc/bf_norm.hip, element by element against the float64 restatement of
tests/layernorm_ref.py: add_layernorm (wave and half-wave kernels, dropout, strided residual rows), embed_layernorm and
add_layernorm_backward (dropout, two gradients), every template instantiation the dispatch can reach.

Bounds are derived, not measured.  Inputs are the rounded values of the tested dtype and the reference is float64 on
those.  ULP is the unit roundoff of the output format (2^-8 bf16, 2^-11 fp16, 2^-24 fp32): the most one correct rounding
adds, relative to the result.  TINY is the absolute term for results the format cannot hold to that precision: half the
fp16 subnormal spacing (2^-25), and for bf16 / fp32 the smallest normal fp32 (2^-126).  E = 2^-24 is the unit roundoff of
the fp32 registers the kernels compute in.  tests/test_layernorm_ref_cpu.py shows that these bounds admit torch's own fp32
layer_norm and autograd on every input used here and reject eight subtly wrong fp32 implementations.

K(A), the fp32 roundings that reach one element, to first order in E.  A lane adds its A = 8 VPL elements one after the
other (half-wave kernel: A = 8 V = N / 32) and a 6-step tree over the lanes follows, so a sum is D = A + 6 roundings deep.
Counted in units of E (|z| + mean_row |z|) rstd, which bounds |zh| = |z - mean| rstd:
    1          z = x + residual
    D + 2      mean: the sum, 1 / N, the product
    1          z - mean
    D / 2 + 5  rstd: the sum of squares is D deep, 1 / N and + eps, halved by the square root; the square root, the
               division, and the roundings of z and z - mean under the squares (the common shift of the mean cancels in
               the sum of squares to first order)
    1          (z - mean) * rstd
    1          the fused multiply-add with gamma and beta, whose fp32 rounding a 16-bit output rounds once more
so K = 1.5 D + 11 = 1.5 (A + 6) + 11: 32 at VPL 1, 56 at N = 768 (V = 3), 212 at N = 8192 (VPL 16).  K and KR below are
worst-case counts: every rounding on the longest path of a sequential sum is taken at full size and with the same sign.
They are deliberately not the statistical multipliers a random-walk model of the same sums would give (a few times
smaller; fp32 kernels measure 0.03 to 0.3 of these bounds), because a bound that a correct kernel could break on an
unlucky input would have to be widened later, and a counted one never has to be.
With dropout z = xs + residual, xs = x * keep / (1 - p): the product is rounded ONCE before the add, relative to |xs| and
not to |z|.  It reaches zh directly and through the mean: one more term, with coefficient E and not K,
    exs = E (|xs| + mean_row |xs|) rstd            (0 without dropout)

Forward:   |err| <= ULP |y| + K E cond + exs |gamma| + TINY,  cond = (|z| + mean_row |z|) rstd |gamma|.  An all-zero row
has cond = 0: the kernel must return beta rounded to the output dtype, and the test also asks for that bit for bit.

Backward, dz = rstd (a - s1 - zh s2) with a = (dy + dy2) gamma, s1 = mean_row a, s2 = mean_row(a zh): the same K covers
every factor (a: the sum dy + dy2 and the product, 2; s1 and s2: D + 3 each; the two subtractions and the product zh s2,
3; rstd and the last product: D / 2 + 6), and the error of zh enters s2 and the product zh s2:
    ezh = K E (|z| + mean_row |z|) rstd + exs
    es2 = K E mean_row |a zh| + mean_row(|a| ezh)
    mag = rstd (K E (|a| + mean_row |a| + |zh| |s2|) + ezh |s2| + |zh| es2) + K E |dz|
    dz:  |err| <= ULP |dz| + mag + TINY
    dx = dz o keep / (1 - p) is the fp32 dz scaled and rounded:  |err| <= ULP |dx| + (mag + E |dz|) keep / (1 - p) + TINY
dgamma = sum_rows g zh and dbeta = sum_rows g, g = dy + dy2, stay fp32.  A lane adds its rows one after the other
(ceil(rows / (4 blocks)) of them, blocks = min(1024, ceil(rows / 4))), the 4 waves of a workgroup are added (4), then
layernorm_param_grad_kernel adds ceil(blocks / 64) partials per lane and 64 lanes one after the other; 2 more for g and the
product:  KR = ceil(rows / (4 blocks)) + ceil(blocks / 64) + 70, and
    dgamma: |err| <= KR E sum_rows |g zh| + sum_rows(|g| ezh)
    dbeta:  |err| <= KR E sum_rows |g|
Through AddLayerNormFn a 16-bit gamma receives them rounded once more: + ULP |.| + TINY."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from layernorm_ref import add_layernorm_bwd_ref, add_layernorm_ref, dropout_product_ref, embed_layernorm_ref

pytestmark = pytest.mark.gpu

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
ULP = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -24}
TINY = {torch.bfloat16: 2.0 ** -126, torch.float16: 2.0 ** -25, torch.float32: 2.0 ** -126}
E = 2.0 ** -24
SEED, CALL, SITE = 0x5EED, 3, 4

FAMILIES = ("plain", "large_mean", "tiny", "zero_row")
EPS = (1e-12, 1e-5)
FWD_WIDTHS = (8, 200, 256, 504, 512, 520, 768, 1024, 1032, 1544, 2048, 2056, 3072, 4096, 4104, 8192)
FWD_ROWS = (1, 2, 7, 9)
DROP_WIDTHS = (200, 256, 512, 520, 768, 1024, 1032, 3072, 4104)
DROP_ROWS = (1, 7)
DROP_P = (0.1, 0.5)
EMBED_WIDTHS = (8, 128, 512, 520, 768, 1024, 1032, 2048, 2056, 4096)
BWD_WIDTHS = (8, 200, 512, 520, 768, 1024, 1032, 2048, 2056, 4096)
BWD_SHAPES = tuple((rows, N) for N in BWD_WIDTHS for rows in (1, 5, 37)) + ((8195, 64),)
VPL_SHAPES = ((37, 512), (37, 1024), (37, 2048), (37, 4096))  # one width per VPL of the backward: 1, 2, 4, 8


# ------------------------------------------------------------------------------------------------------------ the bounds
def fwd_lane_adds(N):
    """Sequential adds per lane in bf_add_layernorm's dispatch (launch_vpl)."""
    nvec = N // 8
    if nvec % 32 == 0 and nvec <= 128:
        return N // 32  # the half-wave kernel: V = nvec / 32 vectors of 8
    return 8 * next(v for v in (1, 2, 4, 8, 16) if nvec <= 64 * v)


def bwd_lane_adds(N):
    """... in launch_bwd_vpl and launch_embed: VPL 1, 2, 4, 8."""
    return 8 * next(v for v in (1, 2, 4, 8) if N // 8 <= 64 * v)


def K_of(adds):
    return 1.5 * (adds + 6) + 11


def KR_of(rows):
    blocks = min(1024, max(1, -(-rows // 4)))
    return -(-rows // (4 * blocks)) + -(-blocks // 64) + 70


def fwd_bound(y64, cond, K, dtype, prod=None):
    """prod: dropout_product_ref's magnitude, with dropout."""
    return ULP[dtype] * y64.abs() + K * E * cond + (0.0 if prod is None else E * prod) + TINY[dtype]


def bwd_bounds(dz64, dx64, m, K, KR, dtype):
    """(dz, dx, dgamma, dbeta) bounds from add_layernorm_bwd_ref's results and magnitudes."""
    ezh = K * E * m.zmag + (0.0 if m.xsmag is None else E * m.xsmag)
    es2 = K * E * m.azh_mean + (m.a * ezh).sum(-1, keepdim=True) / ezh.shape[-1]
    mag = m.rstd * (K * E * (m.a + m.a_mean + m.zh * m.s2) + ezh * m.s2 + m.zh * es2) + K * E * dz64.abs()
    b_dz = ULP[dtype] * dz64.abs() + mag + TINY[dtype]
    b_dx = b_dz if m.scale is None else ULP[dtype] * dx64.abs() + (mag + E * dz64.abs()) * m.scale + TINY[dtype]
    return b_dz, b_dx, KR * E * m.gzh_sum + (m.g * ezh).sum(0), KR * E * m.g_sum


def worst_ratio(got, ref, bound):
    """(every element finite and within its bound, worst error / bound, its index) — one host transfer."""
    err = (got.double() - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    ratio = torch.nan_to_num(ratio, nan=float("inf"))
    bad = ~(err <= bound) | ~torch.isfinite(got)
    flat = ratio.reshape(-1)
    w, at = flat.max(0)
    s = torch.stack((bad.any().double(), w, at.double())).cpu()
    return not bool(s[0]), float(s[1]), np.unravel_index(int(s[2]), tuple(ratio.shape))


def _check(got, ref, bound, what):
    ok, worst, at = worst_ratio(got, ref, bound)
    assert ok, (*what, "at", tuple(int(i) for i in at), "worst error / bound", worst)
    return worst


# ------------------------------------------------------------------------------------------------------------ the inputs
def _seed(*key):
    return 7919 * sum((i + 1) * 104729 * int(k) for i, k in enumerate(key)) % (2 ** 31 - 1) + 1


@functools.lru_cache(maxsize=8)
def make_case(family, rows, N, dtype):
    """x, r, dy, dy2 [rows, N] rounded to `dtype`, gamma / beta fp32 [N], on the CPU, from a generator seeded by the case;
    zero_row: row rows // 2 of x and r is zero."""
    gen = torch.Generator().manual_seed(_seed(FAMILIES.index(family), rows, N))
    rn = lambda *s: torch.randn(*s, generator=gen)
    if family == "large_mean":
        x, r = 0.25 * rn(rows, N) + 100.0, 0.25 * rn(rows, N)
    elif family == "tiny":
        x, r = 1e-3 * rn(rows, N), 1e-3 * rn(rows, N)
    else:
        x, r = 2.0 * rn(rows, N) + 0.5, rn(rows, N)
        if family == "zero_row":
            x[rows // 2] = 0.0
            r[rows // 2] = 0.0
    return SimpleNamespace(x=x.to(dtype), r=r.to(dtype), gamma=1.0 + 0.1 * rn(N), beta=0.1 * rn(N), dy=rn(rows, N).to(dtype),
                           dy2=rn(rows, N).to(dtype), rows=rows, N=N, zero_row=rows // 2 if family == "zero_row" else None)


def _cuda(c):
    return SimpleNamespace(**{k: v.cuda() if torch.is_tensor(v) else v for k, v in vars(c).items()})


@functools.lru_cache(maxsize=None)
def keep_mask(rows, N, p, call=CALL):
    """The oracle's restatement of the kernels' keep decisions: group = 8 consecutive features, row * (N / 8) + n / 8."""
    from oracle import bayes_oracle as bo

    keep = torch.from_numpy(bo.dropout_keep(0, rows * (N // 8), p, SEED, call, SITE).astype(np.float64)).reshape(rows, N)
    return keep, bo.dropout_keep_scale(p)


def param_dtypes(dtype):
    return (torch.float32,) if dtype == torch.float32 else (torch.float32, dtype)


def param_configs(dtype):
    """(gamma / beta dtype, eps)"""
    return [(gdt, eps) for gdt in param_dtypes(dtype) for eps in EPS]


def fwd_configs(dtype):
    """(gamma / beta dtype, with residual, eps)"""
    return [(gdt, res, eps) for gdt in param_dtypes(dtype) for res in (True, False) for eps in EPS]


def eps_set(dtype, family):
    """The backward's eps values.  A zero row under eps = 1e-12 has rstd = 1e6 and |dz| near 4e6, beyond fp16's range
    whoever computes it: fp16 runs the zero-row family with eps = 1e-5 alone."""
    return (1e-5,) if (dtype == torch.float16 and family == "zero_row") else EPS


def bwd_configs(dtype, family):
    """(gamma dtype, with residual, eps, p, two gradients)"""
    return [(gdt, res, eps, p, two) for gdt in param_dtypes(dtype) for res in (True, False) for eps in eps_set(dtype, family)
            for p in (0.0, 0.1) for two in (False, True)]


# --------------------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("name", list(DTYPES))
def test_add_layernorm_matches_float64(name, family):
    """half-wave V = 1..4 (256, 512, 768, 1024), wave VPL = 1, 2, 4, 8, 16; 520 / 1032 / 2056 / 4104: a last chunk whose only
    live lane is lane 0; 504: lane 63 idle; 7 rows: the half-wave kernel's last wave has one live half, 1 row: that alone."""
    from bayeformers_amd import ops

    dtype = DTYPES[name]
    worst = 0.0
    for N in FWD_WIDTHS:
        K = K_of(fwd_lane_adds(N))
        for rows in FWD_ROWS:
            c = _cuda(make_case(family, rows, N, dtype))
            for gdt, has_res, eps in fwd_configs(dtype):
                g, b, r = c.gamma.to(gdt), c.beta.to(gdt), c.r if has_res else None
                y = ops.add_layernorm(c.x, r, g, b, eps)
                assert y.dtype == dtype and y.shape == c.x.shape
                y64, cond = add_layernorm_ref(c.x, r, g, b, eps)
                what = ("add_layernorm", name, family, rows, N, gdt, has_res, eps)
                worst = max(worst, _check(y, y64, fwd_bound(y64, cond, K, dtype), what))
                if c.zero_row is not None:
                    assert torch.equal(y[c.zero_row], b.to(dtype)), what
    print(f"[add_layernorm {name} {family}] worst error / bound {worst:.3f}")


@pytest.mark.parametrize("name", list(DTYPES))
def test_add_layernorm_dropout_matches_float64(name):
    """LayerNorm(dropout(x) + residual) with the oracle's keep mask: DROP = true of the half-wave kernel, V = 1..4 (256, 512,
    768, 1024), and of the wave kernel, VPL 1 (200), 2 (520), 4 (1032), 8 (3072), 16 (4104); 520, 1032 and 4104 with a
    one-lane chunk.  Another call number gives another output."""
    from bayeformers_amd import ops

    dtype = DTYPES[name]
    worst = 0.0
    for p in DROP_P:
        for N in DROP_WIDTHS:
            K = K_of(fwd_lane_adds(N))
            for rows in DROP_ROWS:
                keep, scale = keep_mask(rows, N, p)
                keep = keep.cuda()
                for family in FAMILIES:
                    c = _cuda(make_case(family, rows, N, dtype))
                    for gdt, has_res, eps in fwd_configs(dtype):
                        g, b, r = c.gamma.to(gdt), c.beta.to(gdt), c.r if has_res else None
                        y = ops.add_layernorm(c.x, r, g, b, eps, ops.Dropout(p, SEED, CALL, SITE))
                        y64, cond = add_layernorm_ref(c.x, r, g, b, eps, keep, scale)
                        prod = dropout_product_ref(c.x, r, g, eps, keep, scale)
                        what = ("add_layernorm dropout", name, family, rows, N, gdt, has_res, eps, p)
                        worst = max(worst, _check(y, y64, fwd_bound(y64, cond, K, dtype, prod), what))
                        if c.zero_row is not None:
                            assert torch.equal(y[c.zero_row], b.to(dtype)), what
                c = _cuda(make_case("plain", rows, N, dtype))
                same = ops.add_layernorm(c.x, c.r, c.gamma, c.beta, 1e-12, ops.Dropout(p, SEED, CALL, SITE))
                other = ops.add_layernorm(c.x, c.r, c.gamma, c.beta, 1e-12, ops.Dropout(p, SEED, CALL + 1, SITE))
                y64, cond = add_layernorm_ref(c.x, c.r, c.gamma, c.beta, 1e-12, keep, scale)
                bound = fwd_bound(y64, cond, K, dtype, dropout_product_ref(c.x, c.r, c.gamma, 1e-12, keep, scale))
                assert worst_ratio(same, y64, bound)[0] and not worst_ratio(other, y64, bound)[0], (rows, N, p)
    print(f"[add_layernorm dropout {name}] worst error / bound {worst:.3f}")


@pytest.mark.parametrize("name", list(DTYPES))
def test_add_layernorm_rows_matches_float64(name):
    """bf_add_layernorm_rows at N = 520 with residual rows 528 and 1048 elements apart (multiples of 8 above N): the
    columns between the rows hold NaN, which an address that ignores the stride would read."""
    from bayeformers_amd import ops

    dtype = DTYPES[name]
    rows, N = 7, 520
    K = K_of(fwd_lane_adds(N))
    worst = 0.0
    for family in FAMILIES:
        c = _cuda(make_case(family, rows, N, dtype))
        for stride in (528, 1048):
            buf = torch.full((rows, stride), float("nan"), dtype=dtype, device="cuda")
            buf[:, :N] = c.r
            for gdt, eps in param_configs(dtype):
                g, b = c.gamma.to(gdt), c.beta.to(gdt)
                y = ops.add_layernorm_rows(c.x, buf, stride, g, b, eps)
                y64, cond = add_layernorm_ref(c.x, c.r, g, b, eps)
                worst = max(worst, _check(y, y64, fwd_bound(y64, cond, K, dtype),
                                          ("add_layernorm_rows", name, family, stride, gdt, eps)))
    print(f"[add_layernorm_rows {name}] worst error / bound {worst:.3f}")


# ------------------------------------------------------------------------------------------------------------- embedding
EMBED_B, EMBED_L, EMBED_VOCAB, EMBED_TYPES, EMBED_POS = 3, 7, 50, 2, 9


EMBED_SCALES = (1.0, 1e-3)


@functools.lru_cache(maxsize=4)
def make_embed_case(N, dtype, scale=1.0):
    """Tables (word 50, type 2, position 9 rows; row 0 of each is zero, as a padding row is) and ids on the CPU.  Token
    (0, 3) has word, type and position id 0 under the explicit ids: an all-zero sum.  scale = 1e-3: tables whose rows have
    a variance near 1.5e-6, below eps = 1e-5, so that where eps enters decides the result."""
    gen = torch.Generator().manual_seed(_seed(99, N))
    rn = lambda *s: scale * torch.randn(*s, generator=gen)
    word, typ, pos = rn(EMBED_VOCAB, N), 0.5 * rn(EMBED_TYPES, N) + 0.25 * scale, 0.5 * rn(EMBED_POS, N)
    word[0] = typ[0] = pos[0] = 0.0
    ri = lambda hi, *s: torch.randint(0, hi, s, generator=gen)
    ids, type_ids = ri(EMBED_VOCAB, EMBED_B, EMBED_L), ri(EMBED_TYPES, EMBED_B, EMBED_L)
    pos_1l, pos_bl = ri(EMBED_POS, 1, EMBED_L), ri(EMBED_POS, EMBED_B, EMBED_L)
    ids[0, 3] = type_ids[0, 3] = pos_1l[0, 3] = pos_bl[0, 3] = 0
    gamma, beta = 1.0 + 0.1 * torch.randn(N, generator=gen), 0.1 * torch.randn(N, generator=gen)
    return SimpleNamespace(word=word.to(dtype), typ=typ.to(dtype), pos=pos.to(dtype), gamma=gamma, beta=beta, ids=ids,
                           type_ids=type_ids, pos_1l=pos_1l, pos_bl=pos_bl)


def embed_id_forms(c):
    """(name, type ids, position ids): the defaults, explicit types, [1, L] and [B, L] positions."""
    return (("default", None, None), ("types", c.type_ids, None), ("pos_1L", c.type_ids, c.pos_1l), ("pos_BL", c.type_ids, c.pos_bl))


@pytest.mark.parametrize("name", list(DTYPES))
def test_embed_layernorm_matches_float64(name):
    """ops.embed_layernorm itself, VPL = 1 (8, 128, 512), 2 (520: one live lane in the second chunk; 768, 1024), 4 (1032,
    2048), 8 (2056, 4096), on unit-size and on tiny tables, both gamma dtypes, both eps.  At N = 520 (fp32 gamma,
    eps = 1e-5) one id of each table in turn is out of range: that row is NaN, every other row within its bound."""
    from bayeformers_amd import ops

    dtype = DTYPES[name]
    worst = 0.0
    for N in EMBED_WIDTHS:
        K = K_of(bwd_lane_adds(N)) + 2  # the two adds of the three table rows
        for scale in EMBED_SCALES:
            c = _cuda(make_embed_case(N, dtype, scale))
            for gdt, eps in param_configs(dtype):
                g, b = c.gamma.to(gdt), c.beta.to(gdt)
                for form, type_ids, pos_ids in embed_id_forms(c):
                    y = ops.embed_layernorm(c.ids, type_ids, pos_ids, c.word, c.typ, c.pos, g, b, eps)
                    assert y.shape == (EMBED_B, EMBED_L, N) and y.dtype == dtype
                    y64, cond = embed_layernorm_ref(c.ids, type_ids, pos_ids, c.word, c.typ, c.pos, g, b, eps, EMBED_L)
                    what = ("embed_layernorm", name, N, scale, gdt, eps, form)
                    worst = max(worst, _check(y, y64, fwd_bound(y64, cond, K, dtype), what))
                    if pos_ids is not None:  # the all-zero token: beta
                        assert torch.equal(y[0, 3], b.to(dtype)), what
        if N == 520:
            c = _cuda(make_embed_case(N, dtype))
            g, b, eps = c.gamma, c.beta, 1e-5
            for table, bad_id in (("word", EMBED_VOCAB), ("type", EMBED_TYPES), ("pos", -1)):
                ids, type_ids, pos_ids = c.ids.clone(), c.type_ids.clone(), c.pos_bl.clone()
                {"word": ids, "type": type_ids, "pos": pos_ids}[table][1, 2] = bad_id
                y = ops.embed_layernorm(ids, type_ids, pos_ids, c.word, c.typ, c.pos, g, b, eps)
                y64, cond = embed_layernorm_ref(ids, type_ids, pos_ids, c.word, c.typ, c.pos, g, b, eps, EMBED_L)
                poisoned = torch.isnan(y64).all(-1)
                assert int(poisoned.sum()) == 1 and bool(poisoned[1, 2]) and bool(torch.isnan(y[1, 2]).all()), (N, table)
                _check(y[~poisoned], y64[~poisoned], fwd_bound(y64, cond, K, dtype)[~poisoned],
                       ("embed_layernorm bad id", name, N, table))
    print(f"[embed_layernorm {name}] worst error / bound {worst:.3f}")


# -------------------------------------------------------------------------------------------------------------- backward
def _backward(ops, c, gdt, has_res, eps, p, two):
    drop = ops.Dropout(p, SEED, CALL, SITE) if p else None
    return ops.add_layernorm_backward(c.x, c.r if has_res else None, c.gamma.to(gdt), c.dy, eps, drop, c.dy2 if two else None)


def check_backward(out, c, gdt, has_res, eps, p, two, dtype, what, worst):
    """The kernel's (dz, dgamma, dbeta[, dx]) against the reference; `worst` {output: ratio} is updated."""
    keep, scale = (None, 1.0)
    if p:
        keep, scale = keep_mask(c.rows, c.N, p)
        keep = keep.to(c.x.device)
    dz64, dx64, dg64, db64, m = add_layernorm_bwd_ref(c.x, c.r if has_res else None, c.gamma.to(gdt), c.dy, eps,
                                                       c.dy2 if two else None, keep, scale)
    b_dz, b_dx, b_dg, b_db = bwd_bounds(dz64, dx64, m, K_of(bwd_lane_adds(c.N)), KR_of(c.rows), dtype)
    assert len(out) == (4 if p else 3), what
    dz, dgamma, dbeta = out[:3]
    assert dz.dtype == dtype and dgamma.dtype == dbeta.dtype == torch.float32, what
    worst["dz"] = max(worst.get("dz", 0.0), _check(dz, dz64, b_dz, (*what, "dz")))
    worst["dgamma"] = max(worst.get("dgamma", 0.0), _check(dgamma, dg64, b_dg, (*what, "dgamma")))
    worst["dbeta"] = max(worst.get("dbeta", 0.0), _check(dbeta, db64, b_db, (*what, "dbeta")))
    if p:
        worst["dx"] = max(worst.get("dx", 0.0), _check(out[3], dx64, b_dx, (*what, "dx")))
        assert bool((out[3][keep == 0] == 0).all()), what  # a dropped feature carries no gradient


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("name", list(DTYPES))
def test_add_layernorm_backward_matches_float64(name, family):
    """ops.add_layernorm_backward as the kernels wrote it: VPL 1 (8, 200, 512), 2 (520, 768, 1024), 4 (1032, 2048), 8 (2056,
    4096); 8195 rows of 64: every wave of the 1024-workgroup grid takes two rows of the sweep, three of them a third."""
    from bayeformers_amd import ops

    dtype = DTYPES[name]
    worst = {}
    for rows, N in BWD_SHAPES:
        c = _cuda(make_case(family, rows, N, dtype))
        for gdt, has_res, eps, p, two in bwd_configs(dtype, family):
            out = _backward(ops, c, gdt, has_res, eps, p, two)
            what = ("add_layernorm_backward", name, family, rows, N, gdt, has_res, eps, p, two)
            check_backward(out, c, gdt, has_res, eps, p, two, dtype, what, worst)
    print(f"[add_layernorm_backward {name} {family}] worst error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("name", list(DTYPES))
def test_add_layernorm_fn_casts_the_parameter_gradients(name):
    """AddLayerNormFn, one width per VPL, gamma / beta in the activation dtype: dgamma and dbeta arrive rounded to it."""
    from bayeformers_amd import ops

    dtype = DTYPES[name]
    worst = {}
    for (rows, N), p, family in zip(VPL_SHAPES, (0.0, 0.1, 0.0, 0.1), FAMILIES):
        c = _cuda(make_case(family, rows, N, dtype))
        eps = 1e-5
        x, r, g, b = (t.clone().requires_grad_(True) for t in (c.x, c.r, c.gamma.to(dtype), c.beta.to(dtype)))
        drop = ops.Dropout(p, SEED, CALL, SITE) if p else None
        y = ops.AddLayerNormFn.apply(x, r, g, b, eps, drop)
        y.backward(c.dy)
        keep, scale = (None, 1.0)
        if p:
            keep, scale = keep_mask(rows, N, p)
            keep = keep.cuda()
        y64, cond = add_layernorm_ref(c.x, c.r, g.detach(), b.detach(), eps, keep, scale)
        dz64, dx64, dg64, db64, m = add_layernorm_bwd_ref(c.x, c.r, g.detach(), c.dy, eps, None, keep, scale)
        b_dz, b_dx, b_dg, b_db = bwd_bounds(dz64, dx64, m, K_of(bwd_lane_adds(N)), KR_of(rows), dtype)
        what = ("AddLayerNormFn", name, family, rows, N, p)
        prod = dropout_product_ref(c.x, c.r, g.detach(), eps, keep, scale) if p else None
        _check(y.detach(), y64, fwd_bound(y64, cond, K_of(fwd_lane_adds(N)), dtype, prod), (*what, "y"))
        assert g.grad.dtype == b.grad.dtype == dtype
        cast = 0.0 if dtype == torch.float32 else 1.0  # fp32 parameters take the kernel's fp32 sums as they are
        for key, got, ref, bound in (("dx", x.grad, dx64, b_dx), ("dresidual", r.grad, dz64, b_dz),
                                     ("dgamma", g.grad, dg64, b_dg + cast * (ULP[dtype] * dg64.abs() + TINY[dtype])),
                                     ("dbeta", b.grad, db64, b_db + cast * (ULP[dtype] * db64.abs() + TINY[dtype]))):
            worst[key] = max(worst.get(key, 0.0), _check(got.view_as(ref), ref, bound, (*what, key)))
    print(f"[AddLayerNormFn {name}] worst error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("name", list(DTYPES))
def test_backward_is_deterministic(name):
    """The file header's claim (fixed-order partials, then layernorm_param_grad_kernel): the same launch twice gives the same
    bits in dz, dx, dgamma and dbeta, at one width per VPL and where every wave sweeps several rows."""
    from bayeformers_amd import ops

    dtype = DTYPES[name]
    for rows, N in VPL_SHAPES + ((8195, 64),):
        c = _cuda(make_case("plain", rows, N, dtype))
        for p in (0.0, 0.1):
            for two in (False, True):
                first = [t.clone() for t in _backward(ops, c, torch.float32, True, 1e-12, p, two)]
                torch.cuda.synchronize()
                again = _backward(ops, c, torch.float32, True, 1e-12, p, two)
                assert len(first) == (4 if p else 3)
                assert all(torch.equal(a, b) for a, b in zip(first, again)), (name, rows, N, p, two)
