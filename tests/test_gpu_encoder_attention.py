"""The encoder attention kernels (csrc/bf_attention.hip, csrc/bf_attention_bwd.hip: the forward, the one-tile backward, the
dq and dk / dv kernels, each in bf16 and fp16 and with dropout, and the column-sum tail) against the float64 restatement
of tests/attention_ref.py — out, lse, delta, dq, dk, dv at every point — plus the hard values, bitwise equalities, strided
operands, benchmark shapes, 32-bit boundaries and refusals of the C ABI (include/bayeformers_amd.h).

The kernels are reached through ops.attention_forward / attention_backward / AttentionFn and, for what those wrappers
cannot express (token strides, delta, guard bands, refusals), through _C.lib() with ctypes.  Every output of a ctypes
launch sits between two bands of NaN-pattern words that are checked afterwards."""
import itertools
import types

import numpy as np
import pytest
import torch

from attention_ref import attention_ref
from oracle import bayes_oracle as bo

pytestmark = pytest.mark.gpu

HD = 64
SEED = 0x5EED
# tests/test_gpu_causal_attention.py's TOL (relative to max |reference| per tensor): the same arithmetic contract — the same
# MFMA, P and dS rounded to 16 bits before the second product, fp32 accumulation.  delta takes the dq figure.
TOL = {torch.bfloat16: {"out": 6.3e-3, "dq": 1.5e-2, "dk": 1.1e-2, "dv": 8e-3},
       torch.float16: {"out": 8e-4, "dq": 1.4e-3, "dk": 1.4e-3, "dv": 1.1e-3}}
LSE_ABS = 2e-2  # log2 units, as in the causal file
DT = [torch.bfloat16, torch.float16]
DT_IDS = ["bf16", "fp16"]
BAND = 4096       # guard elements on either side of an output
MARK16 = 0x7FC1   # a NaN in bf16 and in fp16
MARK32 = 0x7FC00001


def name_of(dtype):
    return "bf16" if dtype == torch.bfloat16 else "fp16"


def bf_dtype(dtype):
    from bayeformers_amd import _C

    return {torch.bfloat16: _C.BF_DT_BF16, torch.float16: _C.BF_DT_F16, torch.float32: _C.BF_DT_F32}[dtype]


# ------------------------------------------------------------------------------------------------------------ launching
class Guarded:
    """n elements of `dtype` between two bands of NaN-pattern words."""

    def __init__(self, n, dtype):
        wide = dtype in (torch.float32, torch.int32)
        self.n, self.mark = n, MARK32 if wide else MARK16
        self.buf = torch.full((n + 2 * BAND,), self.mark, dtype=torch.int32 if wide else torch.int16, device="cuda")
        self.t = self.buf[BAND:BAND + n].view(dtype)

    def intact(self):
        return bool((self.buf[:BAND] == self.mark).all()) and bool((self.buf[BAND + self.n:] == self.mark).all())

    def untouched(self):
        return bool((self.buf == self.mark).all())


def ptr(t):
    return None if t is None else t.data_ptr()


def launch(dtype, B, T, H, q, k, v, stride, mask, mask_off, scale, go=None, drop=None, colsum=0):
    """bf_attention_fwd[_dropout] and, given go, bf_attention_bwd[_dropout | _colsum] through ctypes.  q, k, v: tensors whose
    first element is (b, t, h, d) = 0 of an operand with `stride` elements between tokens; drop = (p, seed, call, site);
    colsum = samples.  Returns out / dq / dk / dv [B, T, H, 64], lse / delta [B, H, T], keep [B, H, T, T/32], colsum."""
    from bayeformers_amd import _C, ops

    lib, st = _C.lib(), ops._stream_ptr()
    n = B * T * H * HD
    g = {"out": Guarded(n, dtype), "lse": Guarded(B * H * T, torch.float32)}
    r = types.SimpleNamespace(keep=None, colsum=None, delta=None, dq=None, dk=None, dv=None)
    common = (bf_dtype(dtype), B, T, H, HD, stride, float(scale))
    if drop is not None:
        p, seed, call, site = drop
        g["keep"] = Guarded(B * H * T * (T // 32), torch.int32)
        rc = lib.bf_attention_fwd_dropout(ptr(q), ptr(k), ptr(v), ptr(mask), ptr(mask_off), ptr(g["out"].t), ptr(g["lse"].t),
                                          *common, p, seed, call, site, 0, ptr(g["keep"].t), None, st)
        r.keep = g["keep"].t.view(B, H, T, T // 32)
    else:
        rc = lib.bf_attention_fwd(ptr(q), ptr(k), ptr(v), ptr(mask), ptr(mask_off), ptr(g["out"].t), ptr(g["lse"].t), *common, st)
    assert rc == 0, lib.bf_last_error()
    r.out, r.lse = g["out"].t.view(B, T, H, HD), g["lse"].t.view(B, H, T)
    if go is not None:
        assert go.is_contiguous() and go.dtype == dtype and go.numel() == n
        g["delta"] = Guarded(B * H * T, torch.float32)
        for name in ("dq", "dk", "dv"):
            g[name] = Guarded(n, dtype)
        head = (ptr(q), ptr(k), ptr(v), ptr(mask), ptr(mask_off), ptr(r.out), ptr(go), ptr(r.lse), ptr(g["delta"].t),
                ptr(g["dq"].t), ptr(g["dk"].t), ptr(g["dv"].t)) + common
        if colsum:
            g["partial"] = Guarded(B * H * 3 * HD, torch.float32)
            g["colsum"] = Guarded(3 * colsum * H * HD, torch.float32)
            rc = lib.bf_attention_bwd_colsum(*head, drop[0] if drop else 0.0, ptr(r.keep), colsum, ptr(g["partial"].t),
                                             ptr(g["colsum"].t), st)
            r.colsum = g["colsum"].t.view(3, colsum, H * HD)
        elif drop is not None:
            rc = lib.bf_attention_bwd_dropout(*head, drop[0], ptr(r.keep), st)
        else:
            rc = lib.bf_attention_bwd(*head, st)
        assert rc == 0, lib.bf_last_error()
        r.delta = g["delta"].t.view(B, H, T)
        r.dq, r.dk, r.dv = (g[x].t.view(B, T, H, HD) for x in ("dq", "dk", "dv"))
    torch.cuda.synchronize()
    for name, gd in g.items():
        assert gd.intact(), f"the guard bands around {name} were written"
    r.guards = g
    return r


def run_packed(q, k, v, mask, mask_off, scale, go=None, drop=None, colsum=0):
    """launch() on the [B, H, T, 64] views of packed [B, T, H*64] projections."""
    B, H, T, _ = q.shape
    return launch(q.dtype, B, T, H, q, k, v, H * HD, mask, mask_off, scale, go, drop, colsum)


# --------------------------------------------------------------------------------------------------------------- inputs
def make_inputs(dtype, B, T, H, seed, gain=1.0, order="random"):
    """q, k, v as [B, H, T, 64] views of packed [B, T, H*64] tensors and go [B, T, H, 64].  order "rising" / "falling": the keys
    of tile i scaled by a factor that grows / shrinks with i, so that the running row maximum moves in every key tile."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    q, k, v, go = (torch.randn(B, T, H, HD, device="cuda", generator=g) for _ in range(4))
    if order != "random":
        f = torch.linspace(0.5, 2.0, T // 128, device="cuda")
        f = f if order == "rising" else f.flip(0)
        k = (k.view(B, T // 128, 128, H, HD) * f[None, :, None, None, None]).view(B, T, H, HD)
    q, k, v, go = ((q * gain).to(dtype), k.to(dtype), v.to(dtype), go.to(dtype))
    return q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), go


MASKS = ["right", "left", "holes", "full"]


def make_mask(kind, B, T, fill=float("-inf")):
    """[B, T] additive fp32 mask.  Sequence B - 1 always carries the pattern (B may be 1); the others a variant of it.
    right: a hidden tail; left: a hidden head that crosses a tile edge (T > 128); holes: a hidden run inside a tile and,
    from three tiles on, a whole hidden tile in the middle; full: sequence B - 1 hidden entirely, the others a tail."""
    if kind == "none":
        return None
    m = torch.zeros(B, T)
    for b in range(B):
        last = b == B - 1
        if kind == "right" or (kind == "full" and not last):
            m[b, T - (T // 3 + 17 + 29 * b) % (T - 8) - 1:] = fill
        elif kind == "left":
            m[b, :(128 + 37 if T > 128 else 69) - 16 * (B - 1 - b)] = fill
        elif kind == "holes":
            m[b, 40 + b:77] = fill
            if T >= 384:
                mid = (T // 128) // 2
                m[b, mid * 128:(mid + 1) * 128] = fill
            if T >= 256:
                m[b, T - 128 + 5:T - 128 + 9] = fill
        elif kind == "full":
            m[b] = fill
    return m.cuda()


def flag(value):
    return torch.full((1,), int(value), dtype=torch.uint8, device="cuda")


def rel_err(a, r):
    return (a.double() - r).abs().max().item() / max(r.abs().max().item(), 1e-30)


def compare(r, ref, dtype, label, tol=None):
    """out, lse, delta, dq, dk, dv of a launch against the restatement; prints every figure before it asserts."""
    tol = tol or TOL[dtype]
    for name in ("out", "lse", "delta", "dq", "dk", "dv"):
        assert getattr(r, name).isnan().sum().item() == 0, name
    fin = torch.isfinite(ref.lse)
    same_fin = torch.equal(torch.isfinite(r.lse), fin)
    lse_err = (r.lse[fin].double() - ref.lse[fin]).abs().max().item() if fin.any() else 0.0
    errs = {"out": rel_err(r.out, ref.out), "delta": rel_err(r.delta, ref.delta), "dq": rel_err(r.dq, ref.dq),
            "dk": rel_err(r.dk, ref.dk), "dv": rel_err(r.dv, ref.dv)}
    tols = dict(tol, delta=tol["dq"])
    print(f"[enc-attn] {label} " + " ".join(f"{n}={e:.3e}/{e / tols[n]:.2f}" for n, e in errs.items())
          + f" lse={lse_err:.3e}/{lse_err / LSE_ABS:.2f}")
    assert same_fin, "lse finiteness pattern"
    assert (r.lse[~fin] == float("inf")).all()
    assert lse_err <= LSE_ABS, ("lse", lse_err)
    for n, e in errs.items():
        assert e <= tols[n], (n, e, tols[n])
    for name in ("out", "delta", "dq", "dk", "dv"):
        assert torch.isfinite(getattr(r, name)).all(), name


def kernels_of(T):
    return "tile" if T == 128 else "dq+dkv"


# ----------------------------------------------------------------------------------------------------- a. grid vs float64
def _grid():
    """Every mask variant at every (dtype, T, (B, H)); gain and key order cycle so that each of their values meets every
    kernel (T = 128: the one-tile kernel; T > 128: dq and dk / dv) in both dtypes.  476 points."""
    variants = [("none", None, None)]
    for kind in MASKS:                       # -inf
        variants += [(kind, "inf", None), (kind, "inf", 0)]
    for kind in MASKS[:3]:                   # finite -1e4 (all keys at -1e4: a test of its own below)
        variants += [(kind, "1e4", None), (kind, "1e4", 0)]
    variants += [("right", "bf16min", None), ("right", "bf16min", 0)]
    shapes = {128: [(2, 2), (3, 12), (1, 16)], 256: [(2, 2), (3, 12), (1, 16)], 384: [(2, 2), (3, 12), (1, 16)],
              512: [(2, 2), (3, 12), (1, 16)], 1024: [(2, 2)], 2048: [(1, 4)]}
    gains, orders = [1.0, 4.0, 8.0], ["random", "rising", "falling"]
    pts = []
    for T, bhs in shapes.items():
        i = 0
        for (B, H), (kind, fill, off) in itertools.product(bhs, variants):
            pts.append(pytest.param(T, B, H, kind, fill, off, gains[i % 3], orders[(i // 3) % 3],
                                    id=f"T{T}-B{B}H{H}-{kind}-{fill}-off{off}-g{int(gains[i % 3])}-{orders[(i // 3) % 3]}"))
            i += 1
    return pts


FILLS = {None: 0.0, "inf": float("-inf"), "1e4": -1e4, "bf16min": float(torch.finfo(torch.bfloat16).min)}


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("T,B,H,kind,fill,off,gain,order", _grid())
def test_grid_matches_float64(dtype, T, B, H, kind, fill, off, gain, order):
    from bayeformers_amd import ops

    q, k, v, go = make_inputs(dtype, B, T, H, seed=T * 31 + B * 7 + H, gain=gain, order=order)
    assert ops.attention_supported(q, k, v)
    mask = make_mask(kind, B, T, FILLS[fill])
    mask_off = None if off is None else flag(off)
    scale = HD ** -0.5
    r = run_packed(q, k, v, mask, mask_off, scale, go)
    ref = attention_ref(q, k, v, mask, scale, go=go)
    compare(r, ref, dtype, f"kernels={kernels_of(T)} dtype={name_of(dtype)} T={T} B={B} H={H} mask={kind}/{fill}/off={off} "
                           f"gain={gain:g} order={order}:")
    # the Python wrappers launch the same kernels on the same operands: the same bits
    qr, kr, vr = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    out = ops.AttentionFn.apply(qr, kr, vr, mask, mask_off, scale)
    out.backward(go)
    assert torch.equal(out, r.out)
    for got, want in zip((qr.grad, kr.grad, vr.grad), (r.dq, r.dk, r.dv)):
        assert torch.equal(got.transpose(1, 2), want)
    out2, lse2 = ops.attention_forward(q, k, v, mask, scale, mask_off, want_lse=True)
    assert torch.equal(out2, r.out) and torch.equal(lse2, r.lse)
    if kind == "full":  # the hidden sequence: exact zeros, lse = +inf
        for t in (r.out, r.dq, r.dk, r.dv, r.delta):
            assert (t[B - 1] == 0).all()
        assert (r.lse[B - 1] == float("inf")).all()


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("T,B,H", [(128, 2, 2), (384, 3, 12), (1024, 1, 4)])
def test_every_key_at_minus_1e4_stays_finite_and_within_the_bf16_bounds(dtype, T, B, H):
    """A finite mask over EVERY key (older HF code: -1e4 on a fully padded row) hides nothing: softmax is shift-invariant.
    With every key at -1e4 the fp32 scores sit near -14427 in log2 units, where one ulp is 9.8e-4; that alone is a
    relative error of about 7e-4 per probability, which the fp16 bounds (8e-4 .. 1.4e-3) do not allow for.  So this case
    is pinned on its own: outputs and gradients finite, and within the bf16 tolerances of float64 for BOTH dtypes."""
    q, k, v, go = make_inputs(dtype, B, T, H, seed=T + 3)
    mask = torch.full((B, T), -1e4, device="cuda")
    mask[0, T // 2:] = 0.0 if B > 1 else -1e4  # (one mixed sequence next to the shifted ones)
    r = run_packed(q, k, v, mask, None, 0.125, go)
    ref = attention_ref(q, k, v, mask, 0.125, go=go)
    compare(r, ref, dtype, f"all-keys-at--1e4 dtype={name_of(dtype)} T={T} B={B} H={H} (bf16 bounds):", tol=TOL[torch.bfloat16])


# ------------------------------------------------------------------------------------------------------------- b. dropout
def keep_mask_of(b, h, H, T, p, seed, call, site):
    """[T(query), T(key)] keep mask of one (sequence, head), from the oracle's group numbering (bf_attention_fwd_dropout)."""
    kp = bo.dropout_keep((b * H + h) * T * (T // 8), T * (T // 8), p, seed, call, site)
    kp = kp.reshape(T, T // 128, 4, 4, 2, 4)                    # [query, tile, c, lg, e, j]
    return np.ascontiguousarray(kp.transpose(0, 1, 2, 4, 3, 5)).reshape(T, T)  # key = tile*128 + (2c + e)*16 + 4 lg + j


def keep_words(keep):
    """The kernels' keep words from a [..., T, T] keep mask: word (query, key tile, lg), bit c*8 + e*4 + j (AttnParams)."""
    T = keep.shape[-1]
    km = keep.to(torch.int64).reshape(*keep.shape[:-1], T // 128, 8, 4, 4)  # [.., tile, 2c + e, lg, j]
    bit = (torch.arange(8, device=keep.device)[:, None, None] * 4 + torch.arange(4, device=keep.device)[None, None, :])
    w = (km << bit).sum((-3, -1))                                           # [.., tile, lg]
    w = torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)
    return w.reshape(*keep.shape[:-1], T // 32)


def _dropout_cases():
    out = []
    for i, (T, p, masked) in enumerate(itertools.product([128, 256, 512, 1024], [0.1, 0.25, 0.5], [False, True])):
        B, H = [(2, 2), (3, 2), (1, 4)][i % 3] if T < 1024 else (2, 2)
        out.append(pytest.param(T, p, masked, B, H, 1 + 7 * i, 3 + 5 * i, id=f"T{T}-p{p}-{'masked' if masked else 'open'}-B{B}H{H}"))
    return out


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("T,p,masked,B,H,call,site", _dropout_cases())
def test_dropout_matches_float64_with_the_oracles_mask(dtype, T, p, masked, B, H, call, site):
    """The DROP instantiations, forward and backward: the returned keep words bit for bit against the oracle's mask, and the
    results against float64 with that mask, in the bounds of test_gpu_dropout.py."""
    from bayeformers_amd import ops

    q, k, v, go = make_inputs(dtype, B, T, H, seed=T + int(p * 100))
    mask = make_mask({0.1: "holes", 0.25: "left", 0.5: "right"}[p], B, T) if masked else None
    keep = torch.from_numpy(bo.attention_keep_mask(B, H, T, p, SEED, call, site)).cuda()
    assert abs(float(keep.double().mean()) - (1 - p)) < 0.01
    for b, h in ((0, 0), (B - 1, H - 1)):  # the per-(sequence, head) numbering the large cases below rely on
        assert np.array_equal(keep_mask_of(b, h, H, T, p, SEED, call, site), keep[b, h].cpu().numpy())
    r = run_packed(q, k, v, mask, None, 0.125, go, drop=(p, SEED, call, site))
    assert torch.equal(r.keep, keep_words(keep))
    ref = attention_ref(q, k, v, mask, 0.125, keep=keep, p=p, go=go)
    bf16 = dtype == torch.bfloat16
    tol_o, tol_g = (2.0 ** -7, 2.0 ** -6) if bf16 else (2.0 ** -10, 2.0 ** -9)
    e_out = (r.out.double() - ref.out).abs().max().item()
    errs = {n: rel_err(getattr(r, n), getattr(ref, n)) for n in ("dq", "dk", "dv", "delta")}
    lse_err = (r.lse.double() - ref.lse).abs().max().item()
    print(f"[enc-attn] dropout kernels={kernels_of(T)} dtype={name_of(dtype)} T={T} B={B} H={H} p={p} masked={masked}: "
          f"out={e_out:.3e}/{e_out / (tol_o * ref.out.abs().max().item() + 1e-3):.2f} "
          + " ".join(f"{n}={e:.3e}/{e / tol_g:.2f}" for n, e in errs.items()) + f" lse={lse_err:.3e}/{lse_err / LSE_ABS:.2f}")
    assert e_out <= tol_o * ref.out.abs().max().item() + 1e-3
    for n, e in errs.items():
        assert e <= tol_g, (n, e)
    assert lse_err <= LSE_ABS
    # through the wrappers: the same bits
    qr, kr, vr = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    out = ops.AttentionFn.apply(qr, kr, vr, mask, None, 0.125, ops.Dropout(p, SEED, call, site))
    out.backward(go)
    assert torch.equal(out, r.out)
    for got, want in zip((qr.grad, kr.grad, vr.grad), (r.dq, r.dk, r.dv)):
        assert torch.equal(got.transpose(1, 2), want)


# --------------------------------------------------------------------------------------------------------- c. hard values
@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("T,visible", [(128, 128), (128, 64), (384, 256), (384, 64), (1024, 512)])
def test_zero_queries_average_the_visible_values(dtype, T, visible):
    """q = 0: every visible key weighs 1 / count.  v from {-2 .. 2} and a power-of-two count: the sums are exact in fp32, so
    out is the float64 mean rounded once to the 16-bit type, exactly; lse = log2(count)."""
    B, H = 2, 3
    g = torch.Generator(device="cuda").manual_seed(T + visible)
    k = torch.randn(B, T, H, HD, device="cuda", generator=g).to(dtype).transpose(1, 2)
    v = torch.randint(-2, 3, (B, T, H, HD), device="cuda", generator=g).to(dtype).transpose(1, 2)
    q = torch.zeros_like(k)
    mask = None
    if visible < T:
        perm = torch.stack([torch.randperm(T, device="cuda", generator=g) for _ in range(B)])
        mask = torch.zeros(B, T, device="cuda")
        mask.scatter_(1, perm[:, visible:], float("-inf"))  # hidden keys scattered over all tiles
    r = run_packed(q, k, v, mask, None, 0.125)
    vis = torch.ones(B, T, device="cuda", dtype=torch.float64) if mask is None else (mask == 0).double()
    mean = torch.einsum("bt,bhtd->bhd", vis, v.double()) / visible
    want = mean.to(dtype)[:, None].expand(B, T, H, HD)
    assert torch.equal(r.out, want)
    assert (r.lse.double() - np.log2(visible)).abs().max().item() <= 1e-5


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("T", [128, 384, 512])
def test_one_hot_rows_copy_the_chosen_value_row_bitwise(dtype, T):
    """q_i = 64 k_pi(i) for a permutation pi that crosses the tiles: the chosen key's score beats every other by >= 160 in
    log2 units (asserted in float64 first), so every other probability is exactly 0 in fp32 and P is a permutation matrix.
    out_i must be v_pi(i) and dv_pi(i) must be go_i, bit for bit — which pins the fixed key permutation that the transpose
    reads of all four kernels apply to both operands of the second product.  dq and dk are zero up to the fp32
    summation-order difference between dP and delta."""
    B, H, gain, scale = 2, 2, 64.0, 0.125
    g = torch.Generator(device="cuda").manual_seed(T)
    # keys of +-1: |k|^2 = 64 for every key, and two different keys agree in far fewer than 64 places
    k = (torch.randint(0, 2, (B, T, H, HD), device="cuda", generator=g) * 2 - 1).to(dtype)
    v, go = (torch.randn(B, T, H, HD, device="cuda", generator=g).to(dtype) for _ in range(2))
    pi = torch.randperm(T, device="cuda", generator=g)
    assert T == 128 or bool(((pi // 128) != (torch.arange(T, device="cuda") // 128)).any())
    q = (k[:, pi] * gain).to(dtype)
    assert torch.equal(q.double(), k[:, pi].double() * gain)  # a power of two: exact
    s = torch.einsum("bihd,bjhd->bhij", q.double(), k.double()) * scale * 1.4426950408889634
    chosen = s.gather(-1, pi.view(1, 1, T, 1).expand(B, H, T, 1))
    others = s.scatter(-1, pi.view(1, 1, T, 1).expand(B, H, T, 1), float("-inf")).amax(-1, keepdim=True)
    assert (chosen - others).min().item() >= 160.0
    q, k, v = q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2)
    r = run_packed(q, k, v, None, None, scale, go)
    assert torch.equal(r.out, v.transpose(1, 2)[:, pi])
    want_dv = torch.empty_like(go)
    want_dv[:, pi] = go
    assert torch.equal(r.dv, want_dv)
    mx = lambda t: t.double().abs().max().item()
    bound = 1e-5 * scale * mx(go) * mx(v)
    assert mx(r.dq) <= bound * mx(k), (mx(r.dq), bound * mx(k))
    assert mx(r.dk) <= bound * mx(q), (mx(r.dk), bound * mx(q))
    assert (r.lse.double() - chosen[..., 0]).abs().max().item() <= 1e-3  # the chosen score itself: log2(1) = 0 on top


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("T", [128, 384])
@pytest.mark.parametrize("p", [0.0, 0.25])
def test_a_fully_masked_sequence_is_exact_zeros_and_leaves_its_neighbours_alone(dtype, T, p):
    B, H = 3, 2
    q, k, v, go = make_inputs(dtype, B, T, H, seed=T + 1)
    mask = torch.zeros(B, T, device="cuda")
    mask[1] = float("-inf")
    mask[2, T - 30:] = float("-inf")
    drop = (p, SEED, 2, 3) if p else None
    r = run_packed(q, k, v, mask, flag(0), 0.125, go, drop=drop)
    for t in (r.out, r.lse, r.delta, r.dq, r.dk, r.dv):
        assert t.isnan().sum().item() == 0
    for t in (r.out, r.dq, r.dk, r.dv, r.delta):
        assert (t[1] == 0).all()
    assert (r.lse[1] == float("inf")).all() and torch.isfinite(r.lse[[0, 2]]).all()
    if p:
        return  # (the dropout groups are numbered by sequence: a batch without sequence 1 draws other masks)
    sel = [0, 2]
    qs, ks, vs = (t.transpose(1, 2)[sel].contiguous().transpose(1, 2) for t in (q, k, v))
    r2 = run_packed(qs, ks, vs, mask[sel].contiguous(), flag(0), 0.125, go[sel].contiguous())
    for name in ("out", "lse", "delta", "dq", "dk", "dv"):
        assert torch.equal(getattr(r, name)[sel], getattr(r2, name)), name


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("T", [128, 384])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_mask_off_skips_a_mask_that_does_hide_keys(dtype, T, p):
    """The contract of d_mask_off: non-zero = the mask is skipped — bit-equal to mask = NULL, forward and backward."""
    B, H = 2, 3
    q, k, v, go = make_inputs(dtype, B, T, H, seed=T + 2)
    mask = make_mask("holes", B, T)
    drop = (p, SEED, 4, 5) if p else None
    a = run_packed(q, k, v, mask, flag(1), 0.125, go, drop=drop)
    b = run_packed(q, k, v, None, None, 0.125, go, drop=drop)
    c = run_packed(q, k, v, mask, flag(0), 0.125, go, drop=drop)
    for name in ("out", "lse", "delta", "dq", "dk", "dv"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert not torch.equal(c.out, b.out)


# ------------------------------------------------------------------------------------------------------ d. strided operands
@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("T", [128, 384])
@pytest.mark.parametrize("layout", ["qkv_slabs", "padded"])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_strided_operands_give_the_bits_of_packed_copies(dtype, T, layout, p):
    """token_stride > H*64 — q, k, v as the column slabs of one stacked [B*T, 3*H*64] projection, or rows padded by 8
    elements: q / k / v are addressed with token_stride, out / dout / dq / dk / dv stay packed.  Bitwise the results of packed
    copies of the same values; nothing outside the outputs is written (guard bands in launch())."""
    B, H = 2, 3
    q, k, v, go = make_inputs(dtype, B, T, H, seed=T + 9)
    packed = [t.transpose(1, 2).reshape(B * T, H * HD) for t in (q, k, v)]
    if layout == "qkv_slabs":
        stride = 3 * H * HD
        big = torch.cat(packed, dim=1).contiguous()
        ops_ = [big[:, i * H * HD:] for i in range(3)]           # data_ptr() = the slab's first element
        assert ops_[2].data_ptr() + ((B * T - 1) * stride + H * HD) * 2 == big.data_ptr() + big.numel() * 2  # v ends with the buffer
    else:
        stride = H * HD + 8
        ops_ = []
        for t in packed:
            w = torch.full((B * T, stride), float("nan"), dtype=dtype, device="cuda")
            w[:, :H * HD] = t
            ops_.append(w)
    mask = make_mask("right", B, T)
    drop = (p, SEED, 6, 7) if p else None
    a = launch(dtype, B, T, H, ops_[0], ops_[1], ops_[2], stride, mask, None, 0.125, go, drop=drop)
    b = run_packed(q, k, v, mask, None, 0.125, go, drop=drop)
    for name in ("out", "lse", "delta", "dq", "dk", "dv") + (("keep",) if p else ()):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert not a.out.isnan().any() and not a.dq.isnan().any()  # (the NaN padding between the rows was never read as data)


# ------------------------------------------------------------------------------------------------------------ e. equalities
@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("T", [128, 512])
def test_two_runs_agree_and_a_batch_is_its_sequences_one_at_a_time(dtype, T):
    B, H = 3, 4
    q, k, v, go = make_inputs(dtype, B, T, H, seed=T + 4, gain=2.0)
    mask = make_mask("left", B, T)
    a = run_packed(q, k, v, mask, None, 0.125, go)
    b = run_packed(q, k, v, mask, None, 0.125, go)
    for name in ("out", "lse", "delta", "dq", "dk", "dv"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    for i in range(B):
        qs, ks, vs = (t.transpose(1, 2)[i:i + 1].contiguous().transpose(1, 2) for t in (q, k, v))
        one = run_packed(qs, ks, vs, mask[i:i + 1].contiguous(), None, 0.125, go[i:i + 1].contiguous())
        for name in ("out", "lse", "delta", "dq", "dk", "dv"):
            assert torch.equal(getattr(a, name)[i:i + 1], getattr(one, name)), (name, i)


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("S", [1, 2, 5, 10])
@pytest.mark.parametrize("H", [2, 12])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_column_sum_launch(dtype, S, H, p):
    """bf_attention_bwd_colsum: dq / dk / dv bit-equal to the plain launch, and the [3, S, H*64] sums against float64 sums of
    the stored 16-bit gradients — fp32 summation of 128 * B / S values: 1e-5 relative to sum |x|."""
    B, T = 2 * S, 128
    q, k, v, go = make_inputs(dtype, B, T, H, seed=S * 13 + H)
    mask = make_mask("right", B, T)
    drop = (p, SEED, 8, 9) if p else None
    plain = run_packed(q, k, v, mask, None, 0.125, go, drop=drop)
    folded = run_packed(q, k, v, mask, None, 0.125, go, drop=drop, colsum=S)
    for name in ("out", "lse", "delta", "dq", "dk", "dv"):
        assert torch.equal(getattr(plain, name), getattr(folded, name)), name
    for t, name in enumerate(("dq", "dk", "dv")):
        x = getattr(folded, name).double().reshape(S, (B // S) * T, H * HD)
        err = (folded.colsum[t].double() - x.sum(1)).abs()
        bound = 1e-5 * x.abs().sum(1)
        assert (err <= bound).all(), (name, (err / bound.clamp_min(1e-30)).max().item())


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("masked", [False, True])
def test_gqa_entry_non_causal_group1_d64_is_the_encoder_kernel_bitwise_at_8_tiles(dtype, masked):
    """tests/test_gpu_causal_attention.py holds this at T = 128 and 384; here T = 1024."""
    from bayeformers_amd import ops

    B, H, T = 2, 2, 1024
    q, k, v, go = make_inputs(dtype, B, T, H, seed=77 + masked)
    mask, off = (make_mask("right", B, T), flag(0)) if masked else (None, None)
    a, la = ops.attention_forward_gqa(q, k, v, mask, 0.125, False, off, want_lse=True)
    b, lb = ops.attention_forward(q, k, v, mask, 0.125, off, want_lse=True)
    assert torch.equal(a, b) and torch.equal(la, lb)
    ga = ops.attention_backward_gqa(q, k, v, mask, off, a, go, la, 0.125, False)
    gb = ops.attention_backward(q, k, v, mask, off, b, go, lb, 0.125)
    for x, y in zip(ga, gb):
        assert torch.equal(x, y)


# --------------------------------------------------------------------------------- f. benchmark shapes, 32-bit boundaries
@pytest.mark.parametrize("dtype,B,H,T", [(torch.bfloat16, 320, 12, 128), (torch.float16, 160, 16, 384)],
                         ids=["bert_base_bf16", "bert_large_qa_fp16"])
def test_benchmark_shapes_every_row_against_float64(dtype, B, H, T):
    """The README's shapes — BERT-base S = 10, B = 32, L = 128 and BERT-large QA L = 384 — all rows, forward and backward."""
    q, k, v, go = make_inputs(dtype, B, T, H, seed=B + T)
    mask = torch.zeros(B, T)
    lens = torch.randint(T // 4, T + 1, (B,), generator=torch.Generator().manual_seed(B))
    mask.masked_fill_(torch.arange(T)[None, :] >= lens[:, None], float("-inf"))
    mask = mask.cuda()
    r = run_packed(q, k, v, mask, flag(0), 0.125, go)
    ref = attention_ref(q, k, v, mask, 0.125, go=go)
    compare(r, ref, dtype, f"benchmark-shape kernels={kernels_of(T)} dtype={name_of(dtype)} T={T} B={B} H={H}:")


def _big_randn(shape, dtype, gen):
    out = torch.empty(shape, dtype=dtype, device="cuda")
    flat = out.view(-1)
    step = 1 << 26
    for i in range(0, flat.numel(), step):
        flat[i:i + step] = torch.randn(min(step, flat.numel() - i), device="cuda", generator=gen).to(dtype)
    return out


@pytest.mark.parametrize("dtype,B,H,T,p", [(torch.bfloat16, 16384, 16, 128, 0.0), (torch.float16, 8192, 16, 256, 0.1)],
                         ids=["tile_bf16_2p31", "dq_dkv_fp16_dropout_2p31"])
def test_operands_of_2_to_the_31_elements(dtype, B, H, T, p):
    """B*T*H*64 = 2^31 elements (4 GiB) per operand: the last element index is 2^31 - 1 and byte offsets pass 2^31 half way.
    Checked against float64 on sampled (sequence, head) pairs: the first, the last, the pair either side of element 2^30
    (byte 2^31, where a 32-bit signed byte offset would wrap) and twenty random ones; plus guard bands around every output."""
    free = torch.cuda.mem_get_info()[0]
    if free < 64 << 30:
        reason = f"needs about 40 GiB of device memory, {free / 2 ** 30:.1f} GiB free"
        print("[enc-attn] skipped:", reason)
        pytest.skip(reason)
    assert B * T * H * HD == 2 ** 31
    gen = torch.Generator(device="cuda").manual_seed(B + T)
    q, k, v, go = (_big_randn((B, T, H, HD), dtype, gen) for _ in range(4))
    mask = torch.zeros(B, T, device="cuda")
    mask[1::2, T - 31:] = float("-inf")
    drop = (p, SEED, 11, 12) if p else None
    r = launch(dtype, B, T, H, q, k, v, H * HD, mask, None, 0.125, go, drop=drop)
    per_b = T * H * HD
    mid = 2 ** 30 // per_b
    assert mid * per_b == 2 ** 30
    rnd = np.random.default_rng(B)
    pairs = [(0, 0), (B - 1, H - 1), (mid - 1, H - 1), (mid, 0)] + [(int(rnd.integers(B)), int(rnd.integers(H))) for _ in range(20)]
    bs = torch.tensor([b for b, _ in pairs], device="cuda")
    hs = torch.tensor([h for _, h in pairs], device="cuda")
    pick = lambda t: t[bs, :, hs][:, None]                       # [B, T, H, 64] -> [n, 1, T, 64]
    keep = None
    if p:
        keep = torch.from_numpy(np.stack([keep_mask_of(b, h, H, T, p, SEED, 11, 12) for b, h in pairs])).cuda()[:, None]
        assert torch.equal(r.keep[bs, hs], keep_words(keep[:, 0]))
    ref = attention_ref(pick(q), pick(k), pick(v), mask[bs], 0.125, keep=keep, p=p, go=pick(go).transpose(1, 2))
    got = types.SimpleNamespace(out=pick(r.out).transpose(1, 2), dq=pick(r.dq).transpose(1, 2), dk=pick(r.dk).transpose(1, 2),
                                dv=pick(r.dv).transpose(1, 2), lse=r.lse[bs, hs][:, None], delta=r.delta[bs, hs][:, None])
    tol = TOL[dtype]
    if p:  # test_gpu_dropout.py's bounds (out: + 1e-3 absolute, folded in relative to max |ref| >= ~1 here)
        tol = {"out": 2.0 ** -10 + 1e-3 / ref.out.abs().max().item(), "dq": 2.0 ** -9, "dk": 2.0 ** -9, "dv": 2.0 ** -9}
    compare(got, ref, dtype, f"2^31-elements kernels={kernels_of(T)} dtype={name_of(dtype)} T={T} B={B} H={H} p={p}:", tol=tol)
    assert torch.isfinite(r.out).all() and torch.isfinite(r.dq).all() and torch.isfinite(r.dk).all() and torch.isfinite(r.dv).all()
    del q, k, v, go, r, got
    torch.cuda.empty_cache()


# --------------------------------------------------------------------------------------------------------------- g. refusals
def test_what_the_entries_refuse_is_refused_on_the_host():
    """Status 1 with bf_last_error() set and nothing launched: every output buffer keeps its marker words."""
    from bayeformers_amd import _C, ops

    lib, st = _C.lib(), ops._stream_ptr()
    B, T, H = 2, 256, 2
    n = B * T * H * HD
    q, k, v, go, o = (torch.randn(n + 64, device="cuda").to(torch.bfloat16) for _ in range(5))
    f32in = torch.randn(n + 64, device="cuda")
    lse_in = torch.zeros(B * H * T + 64, device="cuda")
    mask = torch.zeros(B * T + 64, device="cuda")
    outs = {name: Guarded(n, torch.bfloat16) for name in ("out", "dq", "dk", "dv")}
    outs.update({name: Guarded(B * H * T, torch.float32) for name in ("lse", "delta")})
    outs["partial"] = Guarded(B * H * 3 * HD, torch.float32)
    outs["colsum"] = Guarded(3 * 2 * H * HD, torch.float32)
    outs["keep"] = Guarded(B * H * T * (T // 32), torch.int32)
    bf16 = _C.BF_DT_BF16

    def fwd(q=q, k=k, v=v, mask=None, out=outs["out"].t, dtype=bf16, B=B, T=T, H=H, D=HD, stride=H * HD, off=0, moff=0):
        return lib.bf_attention_fwd(q.data_ptr() + off, k.data_ptr(), v.data_ptr(), None if mask is None else mask.data_ptr() + moff,
                                    None, out.data_ptr(), outs["lse"].t.data_ptr(), dtype, B, T, H, D, stride, 0.125, st)

    def fwd_drop(moff):
        return lib.bf_attention_fwd_dropout(q.data_ptr(), k.data_ptr(), v.data_ptr(), mask.data_ptr() + moff, None,
                                            outs["out"].t.data_ptr(), outs["lse"].t.data_ptr(), bf16, B, T, H, HD, H * HD, 0.125,
                                            0.1, SEED, 1, 1, 0, outs["keep"].t.data_ptr(), None, st)

    def bwd_args(mask=None, dtype=bf16, B=B, T=T, H=H, D=HD, stride=H * HD, off=0, moff=0):
        return (q.data_ptr() + off, k.data_ptr(), v.data_ptr(), None if mask is None else mask.data_ptr() + moff, None,
                o.data_ptr(), go.data_ptr(), lse_in.data_ptr(), outs["delta"].t.data_ptr(), outs["dq"].t.data_ptr(),
                outs["dk"].t.data_ptr(), outs["dv"].t.data_ptr(), dtype, B, T, H, D, stride, 0.125)

    def bwd(**kw):
        return lib.bf_attention_bwd(*bwd_args(**kw), st)

    def colsum(samples, **kw):
        return lib.bf_attention_bwd_colsum(*bwd_args(**kw), 0.0, None, samples, outs["partial"].t.data_ptr(),
                                           outs["colsum"].t.data_ptr(), st)

    cases = [
        ("T = 64", lambda: fwd(T=64), lambda: bwd(T=64), b"multiple of 128"),
        ("T = 200", lambda: fwd(T=200), lambda: bwd(T=200), b"multiple of 128"),
        ("head_dim 128", lambda: fwd(D=128, H=1), lambda: bwd(D=128, H=1), b"head size"),
        ("fp32", lambda: fwd(q=f32in, k=f32in, v=f32in, dtype=_C.BF_DT_F32), lambda: bwd(dtype=_C.BF_DT_F32), b"dtype"),
        ("token_stride < H*64", lambda: fwd(stride=H * HD - 8), lambda: bwd(stride=H * HD - 8), b"token stride"),
        ("token_stride % 8", lambda: fwd(stride=H * HD + 4), lambda: bwd(stride=H * HD + 4), b"token stride"),
        ("pointer + 2 bytes", lambda: fwd(off=2), lambda: bwd(off=2), b"16-byte aligned"),
        ("B = 65536", lambda: fwd(B=65536, T=128, H=1), lambda: bwd(B=65536, T=128, H=1), b"exceeds the grid"),
        ("mask + 4 bytes", lambda: fwd(mask=mask, moff=4), lambda: bwd(mask=mask, moff=4), b"mask must be 16-byte aligned"),
        ("mask + 4 bytes, dropout", lambda: fwd_drop(4), None, b"mask must be 16-byte aligned"),
        ("column sums with T = 256", None, lambda: colsum(2), b"column sums"),
        ("column sums with B % S != 0", None, lambda: colsum(3, B=4, T=128, H=1), b"column sums"),
    ]
    for what, f, b, text in cases:
        for call in (f, b):
            if call is None:
                continue
            rc = call()
            err = lib.bf_last_error()
            assert rc == 1, (what, rc)
            assert err and text in err, (what, err)
    torch.cuda.synchronize()
    for name, gd in outs.items():
        assert gd.untouched(), f"{name} was written by a refused call"
    # and the accepted neighbours of two of them: the aligned mask, the stride that is a multiple of 8
    assert fwd(mask=mask) == 0 and fwd(stride=H * HD) == 0
    torch.cuda.synchronize()
    assert outs["out"].intact() and outs["lse"].intact() and not outs["out"].untouched()
