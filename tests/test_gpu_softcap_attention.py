"""Logit soft-capping (Gemma 2) on the causal grouped-query kernels and the decode kernel: bf_attention_fwd_gqa_softcap,
bf_attention_bwd_gqa_softcap and bf_attention_decode_gqa_softcap against the float64 restatement of tests/softcap_ref.py,
the tail forms bitwise against the zero-padded launch, the fixed-capacity form against the plain one, a cap far above the
logits against the entries without a cap, and a two-layer Gemma 2 against its own eager attention.

The bound is the criterion of tests/test_gpu_head256_attention.py: on the same inputs the model's eager chain WITH the cap
(transformers' gemma2 eager_attention_forward: repeat_kv, q @ k^T * scaling in the 16-bit type, / softcap, tanh, * softcap,
the additive mask, an fp32 softmax cast back, @ v; autograd for the gradients) is evaluated in the tested type, and each of
out, dq, dk, dv must be within 2x that chain's error against float64.  The same two exceptions, decided from the arithmetic:
  * W = 1: a query sees itself only, the exact dq and dk are 0 (and so are the chain's); the kernel's error is taken
    relative to a gradient's noise floor, 1e-3 max |dO|, and held to the TOL entry of tests/test_gpu_causal_attention.py;
  * a row with no visible key: out = 0 and zero gradients by contract; the chain's output is multiplied by the rows'
    liveness.
Every case first asserts that the cap matters: the capped and the uncapped float64 references differ by more than 10x the
bound the kernel is held to (20x the chain's error), so a kernel that ignored the cap could not pass.  One place where
that has no meaning: where every query sees ONE key (W = 1, or a decode step of one query on a cache of one key) the
softmax is 1 whatever the score, and no output depends on the cap; there the condition is that the references agree.
Largest errors measured on the MI355X: profiles/softcap_attention.md."""
import pytest
import torch

import softcap_ref
from test_gpu_causal_attention import TOL, make_inputs, make_mask, rel_err
from test_gpu_head256_attention import _decode_mask
from test_gpu_ragged_attention import _go, _zero_extend
from test_gpu_sliding_window import decode_inputs

pytestmark = pytest.mark.gpu

SEED = 0x5EED
CAP = 2.0  # on randn inputs with scaling D^-0.5 the logits have unit spread: a cap of 50 would change nothing measurable
DTYPES = [torch.bfloat16, torch.float16]
HEADS = [(4, 4), (4, 2), (4, 1)]
MASKS = ["none", "right", "left"]


def eager_chain(q, k, v, allowed, scale, softcap, go=None):
    """gemma2's eager attention in q's dtype: q [B, H, Tq, D], k / v [B, Hkv, Tk, D], allowed bool [B, 1, Tq, Tk].
    Returns out [B, Tq, H, D] (rows with no allowed key: 0) and, given go, dq [B, Tq, H, D], dk / dv [B, Tk, Hkv, D]."""
    B, H, Tq, D = q.shape
    Hkv, Tk = k.shape[1], k.shape[2]
    G = H // Hkv
    qr, kr, vr = (t.detach().clone().requires_grad_(go is not None) for t in (q, k, v))
    kk = kr[:, :, None].expand(B, Hkv, G, Tk, D).reshape(B, H, Tk, D)  # repeat_kv
    vv = vr[:, :, None].expand(B, Hkv, G, Tk, D).reshape(B, H, Tk, D)
    add = torch.zeros(allowed.shape, dtype=q.dtype, device=q.device).masked_fill(~allowed, torch.finfo(q.dtype).min)
    w = torch.matmul(qr, kk.transpose(2, 3)) * scale
    if softcap is not None:
        w = torch.tanh(w / softcap) * softcap
    w = torch.nn.functional.softmax(w + add, dim=-1, dtype=torch.float32).to(q.dtype)
    live = allowed.any(-1)[:, 0]  # [B, Tq]
    out = torch.matmul(w, vv).transpose(1, 2).contiguous() * live[:, :, None, None].to(q.dtype)
    if go is None:
        return (out.detach(),)
    out.backward(go)
    return out.detach(), qr.grad.transpose(1, 2), kr.grad.transpose(1, 2), vr.grad.transpose(1, 2)


def _allowed(B, Tq, Tk, W, key_mask):
    a = softcap_ref.visible(Tq, Tk, W, "cuda")[None, None].expand(B, 1, Tq, Tk)
    if key_mask is not None:
        a = a & torch.isfinite(key_mask)[:, None, None, :]
    return a


WORST = {}  # (dtype, quantity) -> (kernel error, chain error, ratio), printed as it grows


def _hold(name, dtype, got, chain, ref, plain, go, zero_ref=(), one_key=False, margin=10):
    """each of out, dq, dk, dv: the kernel's rel_err against float64 <= 2x the eager chain's, after the condition that the
    capped reference `ref` and the uncapped `plain` differ by more than `margin` x that bound (one_key / zero_ref / margin:
    see the module's docstring); every figure is printed before anything is asserted"""
    names = ("out", "dq", "dk", "dv")[:len(got)]
    floor = 1e-3 * go.abs().max().item() if go is not None else 0.0
    lines, bad, weak = [], [], []
    for n, a, c, r, u in zip(names, got, chain, ref, plain):
        assert torch.isfinite(a).all(), n
        moved = rel_err(u, r)
        if n in zero_ref:
            assert r.abs().max().item() < 1e-9 * floor  # (float64's own rounding of dP - delta)
            ek = (a.double() - r).abs().max().item() / floor
            lines.append(f"{n}: kernel {ek:.2e} of the noise floor (float64 is 0), / TOL {ek / TOL[dtype][n]:.2f}")
            if ek > TOL[dtype][n]:
                bad.append((n, ek))
            continue
        ek, ec = rel_err(a, r), rel_err(c, r)
        lines.append(f"{n}: kernel {ek:.2e} chain {ec:.2e} ratio {ek / max(ec, 1e-30):.2f} cap moves {moved:.2e}")
        key = (str(dtype)[6:], n if go is not None else "decode")
        if ek > WORST.get(key, (0.0,))[0]:
            WORST[key] = (ek, ec, ek / max(ec, 1e-30))
        if one_key:
            if moved > 1e-12:
                weak.append((n, moved))
        elif not moved > margin * 2 * ec:
            weak.append((n, moved, ec))
        if ek > 2 * ec:
            bad.append((n, ek, ec))
    print(f"{name}: " + "; ".join(lines))
    print("  worst so far: " + ", ".join(f"{k[0]} {k[1]} {v[0]:.2e} (chain {v[1]:.2e}, ratio {v[2]:.2f})"
                                         for k, v in sorted(WORST.items())))
    assert not weak, ("the cap does not matter enough on these inputs", weak)
    assert not bad, bad


def _run(q, k, v, key_mask, mask_off, go, scale, W, softcap):
    from bayeformers_amd import ops

    out, lse = ops.attention_forward_gqa(q, k, v, key_mask, scale, True, mask_off, want_lse=True, window=W, softcap=softcap)
    dq, dk, dv = ops.attention_backward_gqa(q, k, v, key_mask, mask_off, out, go, lse, scale, True, window=W, softcap=softcap)
    return out, lse, dq, dk, dv


def _case(dtype, D, H, Hkv, T, W, mask, layout, softcap=CAP, qscale=1, margin=10):
    from bayeformers_amd import ops

    B, scale = 2, D ** -0.5
    q, k, v = make_inputs(dtype, B, T, H, Hkv, D, layout, seed=T * 31 + H * 7 + Hkv + D + (W or 0))
    if qscale != 1:
        q = q * qscale  # (a power of two: exact, and the strides stay)
    assert ops.attention_supported(q, k, v, causal=True, kv_heads=Hkv)
    key_mask, mask_off, keep = make_mask(mask, B, T)
    go = _go(dtype, B, T, H, D, T + D)
    qr, kr, vr = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    c0, g0, d0 = dict(ops.SOFTCAP_CALLS), dict(ops.GQA_CALLS), dict(ops.DECODE_CALLS)
    out = ops.AttentionGqaFn.apply(qr, kr, vr, key_mask, mask_off, scale, True, W, softcap)
    out.backward(go)
    moved = {n: ops.SOFTCAP_CALLS[n] - c0[n] for n in c0}
    assert moved == {"fwd": 1, "bwd": 1, "decode": 0, "decode_len": 0} and ops.GQA_CALLS == g0 and ops.DECODE_CALLS == d0
    out2, lse, dq2, dk2, dv2 = _run(q, k, v, key_mask, mask_off, go, scale, W, softcap)
    dq, dk, dv = qr.grad.transpose(1, 2), kr.grad.transpose(1, 2), vr.grad.transpose(1, 2)
    for a, b in ((out, out2), (dq, dq2), (dk, dk2), (dv, dv2)):  # deterministic
        assert torch.equal(a, b)
    r_out, r_lse, r_dq, r_dk, r_dv = softcap_ref.reference(q, k, v, key_mask, scale, W, softcap, go)
    u_out, _, u_dq, u_dk, u_dv = softcap_ref.reference(q, k, v, key_mask, scale, W, None, go)
    chain = eager_chain(q, k, v, _allowed(B, T, T, W, key_mask), scale, softcap, go)
    fin = torch.isfinite(r_lse)
    assert lse.isnan().sum().item() == 0 and torch.equal(torch.isfinite(lse), fin)
    assert (lse[~fin] == float("inf")).all()
    lse_err = (lse[fin].double() - r_lse[fin]).abs().max().item()
    name = (f"softcap {softcap} q*{qscale} {str(dtype)[6:]} D={D} H={H} Hkv={Hkv} T={T} W={W} mask={mask} {layout} "
            f"lse={lse_err:.2e}")
    _hold(name, dtype, (out, dq, dk, dv), chain, (r_out, r_dq, r_dk, r_dv), (u_out, u_dq, u_dk, u_dv), go,
          zero_ref=("dq", "dk") if W == 1 else (), one_key=W == 1, margin=margin)
    assert lse_err < 2e-2
    if mask == "left":  # rows of the padding that see no key at all: exactly 0, gradients 0
        dead = ~keep[1].cuda() & (torch.arange(T, device="cuda") < (~keep[1]).sum().item())
        assert dead.any()
        assert (out[1][dead] == 0).all() and (dq[1][dead] == 0).all()
        assert (dk[1][dead] == 0).all() and (dv[1][dead] == 0).all()
        assert (lse[1][:, dead] == float("inf")).all()


# ---------------------------------------------------------------------------------------------------- 1. the kernel grid
SHAPES = [(128, None), (333, None), (333, 48), (333, 200), (128, 1)]  # (T, W)
GRID = [(dtype, D, H, Hkv, T, W, MASKS[(i + j + m) % 3], ("view", "cache")[(i + j + m) % 2])
        for dtype in DTYPES for i, D in enumerate((64, 128, 256)) for j, (H, Hkv) in enumerate(HEADS)
        for m, (T, W) in enumerate(SHAPES)]  # the masks and layouts rotate over the grid: each meets every D, head layout and shape


def _id(c):
    return f"{str(c[0])[6:]}-D{c[1]}-H{c[2]}-Hkv{c[3]}-T{c[4]}-W{c[5]}-{c[6]}-{c[7]}"


@pytest.mark.parametrize("case", GRID, ids=_id)
def test_softcap_matches_float64_within_twice_the_eager_chain(case):
    _case(*case)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("D,H,Hkv,T,W,mask", [(256, 4, 2, 333, None, "right"), (128, 4, 1, 333, 48, "left"),
                                              (64, 4, 4, 128, None, "none")])
def test_softcap_50_on_gemma_range_logits(dtype, D, H, Hkv, T, W, mask):
    """Gemma 2's own cap with q scaled by 32: logits of spread 32, many beyond the cap (saturated tanh).  The condition that
    the cap matters holds with its factor of 10 in fp16.  In bf16 it cannot: logits of that size carry an absolute error of
    2^-9 * |logit|, up to 0.2, in the chain's 16-bit q @ k^T, so the chain's own error against float64 is 4 - 10 % of the
    largest value and 20x that exceeds 1, more than dropping the cap moves anything (0.23 - 2.3; figures of the float64
    reference and the bf16 chain on the CPU, none of them the kernel's).  There the condition is the purpose itself: the
    uncapped reference misses the bound the kernel is held to (by 2.6x - 23x on those figures)."""
    _case(dtype, D, H, Hkv, T, W, mask, "view", softcap=50.0, qscale=32, margin=10 if dtype == torch.float16 else 1)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("D,H,Hkv,T,W,mask", [(256, 4, 2, 333, None, "right"), (128, 4, 1, 333, 48, "left"),
                                              (64, 4, 4, 128, None, "none")])
def test_softcap_at_the_gemma_ratio_of_logits_to_cap_with_the_full_condition(dtype, D, H, Hkv, T, W, mask):
    """The same problem at an eighth of the size: softcap 6.25 with q scaled by 4 has Gemma range's ratio of logit spread
    to cap (32 / 50), so as many scores saturate, but logits small enough for the bf16 chain to resolve (its error: 0.4 - 1.2
    %, CPU figures).  Here the condition that the cap matters holds with its factor of 10 in both types (dropping the cap
    moves the float64 reference by 0.5 - 2.4 of its largest value, at least 39x the bound)."""
    _case(dtype, D, H, Hkv, T, W, mask, "view", softcap=6.25, qscale=4)


# ---------------------------------------------------------------------------------------------------- 2. tails
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("D", [64, 128, 256])
@pytest.mark.parametrize("T", [100, 333])
@pytest.mark.parametrize("W", [None, 48])
def test_softcap_tail_is_bitwise_the_padded_launch(dtype, D, T, W):
    """Rows < T of out, lse, dq, dk, dv equal a launch zero-padded to the next multiple of 128 (dO = 0 on the added rows)."""
    B, H, Hkv, scale = 2, 4, 2, D ** -0.5
    Tp = (T + 127) // 128 * 128
    q, k, v = make_inputs(dtype, B, T, H, Hkv, D, "cache", seed=T + D)
    go = _go(dtype, B, T, H, D, 7)
    got = _run(q, k, v, None, None, go, scale, W, CAP)
    qp, kp, vp = (_zero_extend(t, 2, Tp) for t in (q, k, v))
    pad = _run(qp, kp, vp, None, None, _zero_extend(go, 1, Tp), scale, W, CAP)
    for n, a, b in zip(("out", "lse", "dq", "dk", "dv"), got, pad):
        b = b[:, :, :T] if n == "lse" else b[:, :T]
        assert a.shape == b.shape
        assert torch.equal(a, b), (n, (a.double() - b.double()).abs().max().item())


# ---------------------------------------------------------------------------------------------------- 3. decode
def _decode_case(dtype, D, H, Hkv, Tq, Tk, mask, W):
    from bayeformers_amd import ops

    N, scale = 3, D ** -0.5
    q, k, v = decode_inputs(dtype, N, H, Hkv, Tq, Tk, D, seed=Tk * 13 + Tq + H + Hkv)
    assert ops.attention_decode_supported(q, k, v)
    key_mask = _decode_mask(mask, N, Tk)
    ref = softcap_ref.reference(q, k, v, key_mask, scale, W, CAP)[0]
    plain = softcap_ref.reference(q, k, v, key_mask, scale, W, None)[0]
    chain = eager_chain(q, k, v, _allowed(N, Tq, Tk, W, key_mask), scale, CAP)
    nbytes = ops.attention_decode_workspace_bytes(q, k, v)  # exactly the reported workspace, then a guard
    assert nbytes >= 0 and nbytes % 16 == 0
    buf = torch.full((nbytes + 256,), 0x5A, dtype=torch.uint8, device="cuda")
    ws = buf[:nbytes] if nbytes else None
    c0, g0, d0 = dict(ops.SOFTCAP_CALLS), dict(ops.GQA_CALLS), dict(ops.DECODE_CALLS)
    out = ops.attention_forward_decode(q, k, v, key_mask, scale, workspace=ws, window=W, softcap=CAP)
    again = ops.attention_forward_decode(q, k, v, key_mask, scale, workspace=ws, window=W, softcap=CAP)
    assert ops.SOFTCAP_CALLS["decode"] - c0["decode"] == 2 and ops.GQA_CALLS == g0 and ops.DECODE_CALLS == d0
    assert (buf[nbytes:] == 0x5A).all()
    assert out.shape == (N, Tq, H, D) and torch.equal(out, again)
    _hold(f"softcap decode {str(dtype)[6:]} D={D} H={H} Hkv={Hkv} Tq={Tq} Tk={Tk} mask={mask} W={W} ws={nbytes}", dtype,
          (out,), chain, (ref,), (plain,), None, one_key=Tk == 1)


DECODE = [(dtype, D, *[(8, 8), (8, 2), (4, 1)][(i + a + b) % 3], Tq, Tk, ("none", "left")[(i + a + b + c) % 2], W)
          for dtype in DTYPES for i, D in enumerate((64, 128, 256)) for a, Tq in enumerate((1, 5, 16))
          for b, Tk in enumerate(("Tq", 65, 1000)) for c, W in enumerate((None, 48))]


@pytest.mark.parametrize("case", DECODE, ids=lambda c: f"{str(c[0])[6:]}-D{c[1]}-H{c[2]}-Hkv{c[3]}-Tq{c[4]}-Tk{c[5]}-{c[6]}-W{c[7]}")
def test_softcap_decode_matches_float64_within_twice_the_eager_chain(case):
    dtype, D, H, Hkv, Tq, Tk, mask, W = case
    _decode_case(dtype, D, H, Hkv, Tq, Tq if Tk == "Tq" else Tk, mask, W)


@pytest.mark.parametrize("D", [64, 128, 256])
@pytest.mark.parametrize("Tq", [1, 5, 16])
@pytest.mark.parametrize("W", [None, 48])
def test_softcap_decode_len_is_the_plain_softcap_call_on_the_first_L_keys(D, Tq, W):
    """A cache of capacity 1024 filled to L: the keys past L are NaN (never read) and the result is the soft-cap call without
    a kv_len on the first L keys, bit for bit (at L = capacity: on the whole cache)."""
    from bayeformers_amd import ops

    dtype, N, H, Hkv, cap, scale = torch.bfloat16, 3, 8, 2, 1024, D ** -0.5
    q, k, v = decode_inputs(dtype, N, H, Hkv, Tq, cap, D, seed=cap + Tq + H + Hkv)
    key_mask = _decode_mask("left", N, cap)
    nbytes = ops.attention_decode_workspace_bytes(q, k, v)
    buf = torch.full((nbytes + 256,), 0x5A, dtype=torch.uint8, device="cuda")
    ws = buf[:nbytes] if nbytes else None
    c0, d0 = dict(ops.SOFTCAP_CALLS), dict(ops.DECODE_CALLS)
    for L in (Tq, 65, cap):
        kc, vc = k.clone(), v.clone()
        kc[:, :, L:] = float("nan")
        vc[:, :, L:] = float("nan")
        mc = key_mask.clone()
        mc[:, L:] = float("nan")
        Lt = torch.tensor([L], device="cuda")
        got = ops.attention_forward_decode_len(q, kc, vc, Lt, mc, scale, workspace=ws, window=W, softcap=CAP)
        assert torch.equal(got, ops.attention_forward_decode_len(q, kc, vc, Lt, mc, scale, workspace=ws, window=W, softcap=CAP))
        plain = ops.attention_forward_decode(q, k[:, :, :L], v[:, :, :L], key_mask[:, :L].contiguous(), scale, window=W,
                                             softcap=CAP)
        assert torch.isfinite(got).all() and (buf[nbytes:] == 0x5A).all()
        assert torch.equal(got, plain), L
    assert ops.SOFTCAP_CALLS["decode_len"] - c0["decode_len"] == 6 and ops.SOFTCAP_CALLS["decode"] - c0["decode"] == 3
    assert ops.DECODE_CALLS == d0


# ---------------------------------------------------------------------------------------------------- 4. the constants
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("D", [64, 128, 256])
@pytest.mark.parametrize("W", [None, 48])
def test_a_cap_far_above_the_logits_gives_the_entries_without_a_cap(dtype, D, W):
    """softcap = 1e30: softcap * tanh(z / softcap) is z to rounding, so the soft-cap entries must give what the plain ones
    give — held, like everything here, to 2x the eager chain's (uncapped) error; it guards the folding of the constants."""
    from bayeformers_amd import ops

    B, H, Hkv, T, scale = 2, 4, 2, 333, D ** -0.5
    q, k, v = make_inputs(dtype, B, T, H, Hkv, D, "view", seed=D + (W or 0))
    key_mask, mask_off, _ = make_mask("right", B, T)
    go = _go(dtype, B, T, H, D, 5)
    got = _run(q, k, v, key_mask, mask_off, go, scale, W, 1e30)
    want = _run(q, k, v, key_mask, mask_off, go, scale, W, None)
    ref = softcap_ref.reference(q, k, v, key_mask, scale, W, None, go)
    chain = eager_chain(q, k, v, _allowed(B, T, T, W, key_mask), scale, None, go)
    bad = []
    for n, a, b, r, c in zip(("out", "dq", "dk", "dv"), (got[0],) + got[2:], (want[0],) + want[2:], [ref[0]] + ref[2:], chain):
        d, ec = rel_err(a, b.double()), rel_err(c, r)
        print(f"softcap 1e30 {str(dtype)[6:]} D={D} W={W} {n}: against the plain entry {d:.2e}, chain {ec:.2e}")
        if d > 2 * ec:
            bad.append((n, d, ec))
    fin = torch.isfinite(want[1])  # lse: +inf on the rows whose window holds padding only
    assert torch.equal(torch.isfinite(got[1]), fin) and (got[1][fin] - want[1][fin]).abs().max().item() < 1e-3
    assert not bad, bad
    qd, kd, vd = decode_inputs(dtype, 3, 8, 2, 5, 1000, D, seed=D)
    a = ops.attention_forward_decode(qd, kd, vd, None, scale, window=W, softcap=1e30)
    b = ops.attention_forward_decode(qd, kd, vd, None, scale, window=W)
    ec = rel_err(eager_chain(qd, kd, vd, _allowed(3, 5, 1000, W, None), scale, None)[0],
                 softcap_ref.reference(qd, kd, vd, None, scale, W, None)[0])
    print(f"softcap 1e30 {str(dtype)[6:]} D={D} W={W} decode: against the plain entry {rel_err(a, b.double()):.2e}, chain {ec:.2e}")
    assert rel_err(a, b.double()) <= 2 * ec


def test_softcap_counters_move_and_the_old_ones_do_not():
    from bayeformers_amd import ops

    q, k, v = make_inputs(torch.bfloat16, 1, 100, 4, 2, 64, "view", seed=1)
    go = _go(torch.bfloat16, 1, 100, 4, 64, 1)
    qd, kd, vd = decode_inputs(torch.bfloat16, 1, 4, 2, 1, 70, 64, seed=1)
    c0, g0, d0 = dict(ops.SOFTCAP_CALLS), dict(ops.GQA_CALLS), dict(ops.DECODE_CALLS)
    _run(q, k, v, None, None, go, 0.125, 48, 30.0)
    ops.attention_forward_decode(qd, kd, vd, None, 0.125, softcap=30.0)
    ops.attention_forward_decode_len(qd, kd, vd, torch.tensor([70], device="cuda"), None, 0.125, window=48, softcap=30.0)
    assert {n: ops.SOFTCAP_CALLS[n] - c0[n] for n in c0} == {"fwd": 1, "bwd": 1, "decode": 1, "decode_len": 1}
    assert ops.GQA_CALLS == g0 and ops.DECODE_CALLS == d0
    _run(q, k, v, None, None, go, 0.125, 48, None)  # no cap: exactly the calls of before
    assert ops.GQA_CALLS["fwd_window"] - g0["fwd_window"] == 1 and ops.GQA_CALLS["bwd_window"] - g0["bwd_window"] == 1
    assert {n: ops.SOFTCAP_CALLS[n] - c0[n] for n in c0} == {"fwd": 1, "bwd": 1, "decode": 1, "decode_len": 1}


# ---------------------------------------------------------------------------------------------------- 5. a Gemma 2
@pytest.fixture
def softcap_on():
    import bayeformers_amd as bf

    bf.softcap_attention()
    yield
    bf.softcap_attention(False)


MODEL_CAP = 1.0  # attn_logit_softcapping of the test model: small enough to shape the logits of a random-weight model
# (query_pre_attn_scalar = 1, the smallest the config takes: scaling 1; on the CPU the fp32 eager logits then move by 1.08 of
# their largest without the cap, against 10 (2 e16 + 2e-3) = 0.25)


def _gemma2(dtype, fuse, softcap=MODEL_CAP):
    """test_gpu_head256_attention._gemma's recipe for a Gemma 2 (sliding W = 100, then full; head size 256) on its EAGER
    attention: the only implementation of the framework that applies the cap"""
    from transformers import AutoConfig, AutoModelForCausalLM

    import bayeformers_amd as bf

    cfg = AutoConfig.for_model("gemma2", hidden_size=256, num_attention_heads=4, num_key_value_heads=2, head_dim=256,
                               num_hidden_layers=2, intermediate_size=512, vocab_size=512, max_position_embeddings=1024,
                               tie_word_embeddings=False, attention_dropout=0.0, attn_implementation="eager",
                               sliding_window=100, layer_types=["sliding_attention", "full_attention"],
                               attn_logit_softcapping=softcap, final_logit_softcapping=None, query_pre_attn_scalar=1)
    torch.manual_seed(0)
    bmodel = bf.to_bayesian(AutoModelForCausalLM.from_config(cfg).eval(), delta=0.05, freeze=True).eval().cuda()
    if dtype != torch.float32:
        freqs = {n: b.detach().clone() for n, b in bmodel.named_buffers() if "inv_freq" in n}
        bmodel = bmodel.to(dtype)
        for n, b in freqs.items():
            setattr(bmodel.get_submodule(n.rsplit(".", 1)[0]), n.rsplit(".", 1)[1], b)
    if fuse:
        assert bf.fuse_attention(bmodel)
    return bmodel


MODES = (("ref", torch.float32, False), ("eager16", torch.bfloat16, False), ("fused", torch.bfloat16, True))


def _prompt(B=2, T=256, pad=37):
    ids = torch.randint(0, 512, (B, T), generator=torch.Generator().manual_seed(11)).cuda()
    mask = torch.ones_like(ids)
    mask[B - 1, T - pad:] = 0  # right padding: no query row without a visible key
    return ids, mask


def _logits(model, ids, mask, S=2):
    import bayeformers_amd as bf
    from bayeformers_amd.sampling import sample_bayesian

    bf.manual_seed(SEED)
    with torch.no_grad():
        raw, _, _, _ = sample_bayesian(model, {"input_ids": ids, "attention_mask": mask, "use_cache": False}, S)
    return raw[0].float().view(S, *ids.shape, -1)


def test_gemma2_logits_match_the_eager_model(softcap_on):
    """The fused bf16 logits against the fp32 EAGER model, ef <= 2 e16 + 2e-3 with e16 the bf16 eager model's error (the
    criterion of test_gemma3_head256_logits_match_the_framework_model with the reference that applies the cap), after the
    condition that the cap shapes this model's logits: without it the fp32 eager logits move by more than 10x that bound."""
    from bayeformers_amd import ops

    ids, mask = _prompt()
    outs = {}
    for name, dtype, fuse in MODES:
        model = _gemma2(dtype, fuse)
        assert model.model.model.layers[0].self_attn.head_dim == 256
        c0, g0 = dict(ops.SOFTCAP_CALLS), dict(ops.GQA_CALLS)
        outs[name] = _logits(model, ids, mask)
        moved = {k: ops.SOFTCAP_CALLS[k] - c0[k] for k in c0}
        assert moved == ({"fwd": 2, "bwd": 0, "decode": 0, "decode_len": 0} if fuse else dict.fromkeys(c0, 0)), moved
        assert ops.GQA_CALLS == g0
    outs["uncapped"] = _logits(_gemma2(torch.float32, False, softcap=None), ids, mask)
    valid = mask.bool()[None, :, :, None].expand_as(outs["ref"])
    ref = outs["ref"][valid]
    e16 = (outs["eager16"][valid] - ref).abs().max().item() / ref.abs().max().item()
    ef = (outs["fused"][valid] - ref).abs().max().item() / ref.abs().max().item()
    cap = (outs["uncapped"][valid] - ref).abs().max().item() / ref.abs().max().item()
    print(f"[gemma2 D=256 cap {MODEL_CAP}] fused bf16 {ef:.3e}, eager bf16 {e16:.3e}, fp32 without the cap {cap:.3e} "
          "(max |logit - fp32 eager| / max |fp32 eager|)")
    assert cap > 10 * (2 * e16 + 2e-3)
    assert ef <= 2 * e16 + 2e-3


def test_gemma2_training_step_runs_the_softcap_backward(softcap_on):
    """One training step: both layers run bf_attention_bwd_gqa_softcap, every gradient is finite and the q / k / v
    projections' mu-gradients are within 2x the bf16 eager model's error against the fp32 eager model."""
    from test_gpu_causal_attention import _token_nll

    import bayeformers_amd as bf
    from bayeformers_amd import ops
    from bayeformers_amd.sampling import elbo, sample_bayesian

    ids, mask = _prompt()
    grads = {}
    for name, dtype, fuse in MODES:
        model = _gemma2(dtype, fuse)
        for p in model.parameters():
            p.requires_grad_(p.dtype.is_floating_point)
        c0, g0 = dict(ops.SOFTCAP_CALLS), dict(ops.GQA_CALLS)
        bf.manual_seed(SEED)
        _, mean, lp, lq = sample_bayesian(model, {"input_ids": ids, "attention_mask": mask, "use_cache": False}, 2)
        loss = elbo(lp, lq, _token_nll(mean[0].float(), ids, mask).double(), 4)
        loss.backward()
        moved = {k: ops.SOFTCAP_CALLS[k] - c0[k] for k in c0}
        if fuse:  # both layers, forward and backward
            assert moved["fwd"] >= 2 and moved["bwd"] >= 2 and moved["decode"] == moved["decode_len"] == 0, moved
        else:
            assert moved == dict.fromkeys(c0, 0), moved
        assert ops.GQA_CALLS == g0
        grads[name] = {n: p.grad.double().clone() for n, p in model.named_parameters() if p.grad is not None}
        assert all(torch.isfinite(g).all() for g in grads[name].values())
    assert grads["fused"].keys() == grads["ref"].keys()
    proj = [n for n in grads["ref"] if any(n.endswith(f"{p}_proj.weight.mu") for p in "qkv")]
    assert len(proj) >= 6, sorted(grads["ref"])[:20]
    bad = []
    for n in proj:
        g = grads["ref"][n]
        e16, ef = rel_err(grads["eager16"][n], g), rel_err(grads["fused"][n], g)
        print(f"[gemma2 D=256] {n}: fused {ef:.3e}, eager bf16 {e16:.3e}, ratio {ef / max(e16, 1e-30):.2f}")
        if ef > 2 * e16:
            bad.append((n, ef, e16))
    assert not bad, bad


def test_gemma2_graph_generation_is_static_and_matches_teacher_forcing(softcap_on):
    """bf16 with kept weights: graph=True returns the static_cache=True Generation field for field, bit for bit, the decode
    steps run bf_attention_decode_gqa_softcap with the fill (two layers a step), and the greedy tokens are teacher
    forcing's on the same fused model."""
    from dataclasses import fields

    import bayeformers_amd as bf
    from bayeformers_amd import ops
    from bayeformers_amd.sampling import mc_predictive, sample_bayesian, sample_generate

    bmodel = _gemma2(torch.bfloat16, True)
    bf.set_compute_dtype("bf16")
    ids = torch.randint(0, 512, (2, 96), generator=torch.Generator().manual_seed(11)).cuda()
    S, n, T0 = 3, 8, ids.shape[1]  # 96 + 8 tokens against W = 100: the window is crossed during the decode
    out = {}
    for mode in ("static_cache", "graph"):
        bf.manual_seed(SEED)
        c0, d0, g0 = dict(ops.SOFTCAP_CALLS), dict(ops.DECODE_CALLS), dict(ops.GQA_CALLS)
        with torch.no_grad():
            out[mode] = sample_generate(bmodel, ids, samples=S, max_new_tokens=n, keep_weights=True, **{mode: True})
        assert ops.DECODE_CALLS == d0 and ops.GQA_CALLS == g0
        assert ops.SOFTCAP_CALLS["fwd"] - c0["fwd"] >= 2  # the prefill: both layers
        if mode == "static_cache":
            assert ops.SOFTCAP_CALLS["decode_len"] - c0["decode_len"] == 2 * (n - 1)
        else:  # enqueued under capture (and its warm-up), replayed after that
            assert ops.SOFTCAP_CALLS["decode_len"] - c0["decode_len"] >= 2
    assert all(torch.equal(getattr(out["graph"], f.name), getattr(out["static_cache"], f.name)) for f in fields(out["graph"]))
    gen = out["graph"]
    bf.manual_seed(SEED)
    with torch.no_grad():
        raw, _, _, _ = sample_bayesian(bmodel, {"input_ids": gen.sequences[:, :-1], "use_cache": False}, S)
    pred = mc_predictive(raw[0][:, :, T0 - 1:])
    assert torch.equal(pred.prediction, gen.sequences[:, T0:])
