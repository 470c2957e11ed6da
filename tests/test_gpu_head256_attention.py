"""Head size 256 (Gemma 1/2/3, Qwen3-Next) on the causal grouped-query kernels and the KV-cache decode kernel: against the
float64 restatements of tests/test_gpu_causal_attention.py and tests/test_gpu_sliding_window.py, the tail forms bitwise
against the zero-padded launch, "nothing at or past row T", the decode entries, the refusals and two Gemma decoders.

The bound on a kernel's error is not taken from the kernels: on the same inputs the model's own unfused arithmetic
(transformers' eager_attention_forward chain: repeat_kv, q @ k^T * scaling in the 16-bit type, the additive mask, an fp32
softmax cast back, @ v; autograd for the gradients) is evaluated in the tested type, and each of out, dq, dk, dv must be
within 2x that chain's error against float64 (both round P to 16 bits and accumulate in fp32 in another order; 2 is the
factor of test_sliding_decoder_logits_match_sdpa and of TOL).  Two places where that rule has no meaning, decided from the
arithmetic and not from a result:
  * W = 1: a query sees itself only, so the exact dq and dk are identically 0 and the chain's are too (its softmax
    backward computes 1 * (g - g)); the kernel's dS = P (dP - delta) keeps the 16-bit rounding of `out` inside delta.  There
    the error is taken relative to a gradient's noise floor, 1e-3 max |dO|, and held to the existing TOL entry — the rule
    tests/test_gpu_sliding_window.py and tests/test_gpu_ragged_attention.py apply to W = 1 and T = 1;
  * a row with no visible key (left padding): the contract is out = 0 and zero gradients, while a softmax over a row of
    finfo.min is uniform; the chain's output is multiplied by the rows' liveness, so both compute the same function.
Largest errors measured on the MI355X: profiles/head256_attention.md."""
import ctypes

import pytest
import torch

from test_gpu_causal_attention import TOL, make_inputs, make_mask, reference, rel_err
from test_gpu_ragged_attention import _go, _guards_intact, _interior, _lib_bwd, _lib_fwd, _run, _zero_extend
from test_gpu_sliding_window import DEC_TOL, decode_inputs, visible
from test_gpu_sliding_window import reference as window_reference

pytestmark = pytest.mark.gpu

D = 256
SEED = 0x5EED
SCALE = D ** -0.5
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])


def eager_chain(q, k, v, allowed, scale, go=None):
    """transformers' eager attention in q's dtype: q [B, H, Tq, D], k / v [B, Hkv, Tk, D], allowed bool [B, 1, Tq, Tk].
    Returns out [B, Tq, H, D] (rows with no allowed key: 0) and, given go, dq [B, Tq, H, D], dk / dv [B, Tk, Hkv, D]."""
    B, H, Tq, _ = q.shape
    Hkv, Tk = k.shape[1], k.shape[2]
    G = H // Hkv
    qr, kr, vr = (t.detach().clone().requires_grad_(go is not None) for t in (q, k, v))
    kk = kr[:, :, None].expand(B, Hkv, G, Tk, D).reshape(B, H, Tk, D)  # repeat_kv
    vv = vr[:, :, None].expand(B, Hkv, G, Tk, D).reshape(B, H, Tk, D)
    add = torch.zeros(allowed.shape, dtype=q.dtype, device=q.device).masked_fill(~allowed, torch.finfo(q.dtype).min)
    w = torch.matmul(qr, kk.transpose(2, 3)) * scale + add
    w = torch.nn.functional.softmax(w, dim=-1, dtype=torch.float32).to(q.dtype)
    live = allowed.any(-1)[:, 0]  # [B, Tq]
    out = torch.matmul(w, vv).transpose(1, 2).contiguous() * live[:, :, None, None].to(q.dtype)
    if go is None:
        return (out.detach(),)
    out.backward(go)
    return out.detach(), qr.grad.transpose(1, 2), kr.grad.transpose(1, 2), vr.grad.transpose(1, 2)


def _allowed(B, Tq, Tk, causal, W, key_mask):
    a = torch.ones(Tq, Tk, dtype=torch.bool, device="cuda")
    if causal:
        a = visible(Tq, Tk, W if W is not None else Tk + Tq, "cuda")
    a = a[None, None].expand(B, 1, Tq, Tk)
    if key_mask is not None:
        a = a & torch.isfinite(key_mask)[:, None, None, :]
    return a


WORST = {}  # (dtype, quantity) -> (kernel error, chain error, kernel error / existing TOL entry), printed as it grows


def _hold(name, dtype, got, chain, ref, go, zero_ref=()):
    """each of out, dq, dk, dv: the kernel's rel_err against float64 <= 2x the eager chain's (zero_ref: see the module's
    docstring); both errors and the ratio to the existing TOL entry are printed before anything is asserted"""
    names = ("out", "dq", "dk", "dv")[:len(got)]
    floor = 1e-3 * go.abs().max().item() if go is not None else 0.0
    lines, bad = [], []
    for n, a, c, r in zip(names, got, chain, ref):
        assert torch.isfinite(a).all(), n
        if n in zero_ref:
            assert r.abs().max().item() < 1e-9 * floor  # (float64's own rounding of dP - delta)
            ek = (a.double() - r).abs().max().item() / floor
            lines.append(f"{n}: kernel {ek:.2e} of the noise floor (float64 is 0), / TOL {ek / TOL[dtype][n]:.2f}")
            if ek > TOL[dtype][n]:
                bad.append((n, ek))
            continue
        ek, ec = rel_err(a, r), rel_err(c, r)
        tol = TOL[dtype][n] if go is not None else DEC_TOL[dtype]
        lines.append(f"{n}: kernel {ek:.2e} chain {ec:.2e} ratio {ek / max(ec, 1e-30):.2f}, / TOL {ek / tol:.2f}")
        key = (str(dtype)[6:], n if go is not None else "decode")
        if ek > WORST.get(key, (0.0,))[0]:
            WORST[key] = (ek, ec, ek / tol)
        if ek > 2 * ec:
            bad.append((n, ek, ec))
    print(f"{name}: " + "; ".join(lines))
    print("  worst so far: " + ", ".join(f"{k[0]} {k[1]} {v[0]:.2e} (chain {v[1]:.2e}, / TOL {v[2]:.2f})"
                                         for k, v in sorted(WORST.items())))
    assert not bad, bad


def _case(dtype, H, Hkv, T, mask, layout, causal=True, W=None):
    from bayeformers_amd import ops

    B = 2
    q, k, v = make_inputs(dtype, B, T, H, Hkv, D, layout, seed=T * 31 + H * 7 + Hkv + D + (W or 0))
    assert ops.attention_supported(q, k, v, causal=causal, kv_heads=Hkv)
    key_mask, mask_off, keep = make_mask(mask, B, T)
    go = _go(dtype, B, T, H, D, T + D)
    qr, kr, vr = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    c0 = dict(ops.GQA_CALLS)
    out = ops.AttentionGqaFn.apply(qr, kr, vr, key_mask, mask_off, SCALE, causal, *(() if W is None else (W,)))
    out.backward(go)
    tag = "_window" if W is not None else ""
    assert ops.GQA_CALLS["fwd" + tag] - c0["fwd" + tag] == 1 and ops.GQA_CALLS["bwd" + tag] - c0["bwd" + tag] == 1
    out2, lse = ops.attention_forward_gqa(q, k, v, key_mask, SCALE, causal, mask_off, want_lse=True, window=W)
    assert torch.equal(out, out2)
    dq, dk, dv = qr.grad.transpose(1, 2), kr.grad.transpose(1, 2), vr.grad.transpose(1, 2)
    if W is None:
        r_out, r_lse, r_dq, r_dk, r_dv = reference(q, k, v, key_mask, SCALE, causal, go)
    else:
        r_out, r_lse, r_dq, r_dk, r_dv = window_reference(q, k, v, key_mask, SCALE, W, go)
    chain = eager_chain(q, k, v, _allowed(B, T, T, causal, W, key_mask), SCALE, go)
    fin = torch.isfinite(r_lse)
    assert lse.isnan().sum().item() == 0 and torch.equal(torch.isfinite(lse), fin)
    assert (lse[~fin] == float("inf")).all()
    lse_err = (lse[fin].double() - r_lse[fin]).abs().max().item()
    name = f"head256 {str(dtype)[6:]} H={H} Hkv={Hkv} T={T} mask={mask} {layout} causal={causal} W={W} lse={lse_err:.2e}"
    _hold(name, dtype, (out, dq, dk, dv), chain, (r_out, r_dq, r_dk, r_dv), go, zero_ref=("dq", "dk") if W == 1 else ())
    assert lse_err < 2e-2
    if mask == "left" and causal:  # rows of the padding that see no key at all: exactly 0, gradients 0
        dead = ~keep[1].cuda() & (torch.arange(T, device="cuda") < (~keep[1]).sum().item())
        assert dead.any()
        assert (out[1][dead] == 0).all() and (dq[1][dead] == 0).all()
        assert (dk[1][dead] == 0).all() and (dv[1][dead] == 0).all()
        assert (lse[1][:, dead] == float("inf")).all()


# ---------------------------------------------------------------------------------------------------- 1. the kernel grid
@DTYPES
@pytest.mark.parametrize("H,Hkv", [(4, 4), (4, 2), (4, 1)])
@pytest.mark.parametrize("T", [128, 384, 100, 333])
@pytest.mark.parametrize("mask", ["none", "right", "left"])
@pytest.mark.parametrize("layout", ["view", "cache"])
def test_head256_causal_matches_float64_within_twice_the_eager_chain(dtype, H, Hkv, T, mask, layout):
    _case(dtype, H, Hkv, T, mask, layout)


@DTYPES
@pytest.mark.parametrize("H,Hkv", [(4, 4), (4, 2), (4, 1)])
@pytest.mark.parametrize("T", [384, 100])
def test_head256_non_causal_matches_float64_within_twice_the_eager_chain(dtype, H, Hkv, T):
    _case(dtype, H, Hkv, T, "right", "cache", causal=False)


@DTYPES
@pytest.mark.parametrize("H,Hkv", [(4, 4), (4, 2), (4, 1)])
@pytest.mark.parametrize("T,W", [(333, 1), (333, 48), (333, 200), (128, 48)])
@pytest.mark.parametrize("mask,layout", [("none", "view"), ("left", "cache"), ("right", "view")])
def test_head256_window_matches_float64_within_twice_the_eager_chain(dtype, H, Hkv, T, W, mask, layout):
    _case(dtype, H, Hkv, T, mask, layout, W=W)


# ---------------------------------------------------------------------------------------------------- 2. tails
@DTYPES
@pytest.mark.parametrize("T", [100, 333])
@pytest.mark.parametrize("W", [None, 48, 200])
def test_head256_tail_is_bitwise_the_padded_launch(dtype, T, W):
    """Rows < T of out, lse, dq, dk, dv equal a launch zero-padded to the next multiple of 128 (dO = 0 on the added rows)."""
    B, H, Hkv = 2, 4, 2
    Tp = (T + 127) // 128 * 128
    q, k, v = make_inputs(dtype, B, T, H, Hkv, D, "cache", seed=T + D)
    go = _go(dtype, B, T, H, D, 7)
    got = _run(q, k, v, None, None, go, SCALE, True, W)
    qp, kp, vp = (_zero_extend(t, 2, Tp) for t in (q, k, v))
    pad = _run(qp, kp, vp, None, None, _zero_extend(go, 1, Tp), SCALE, True, W)
    for n, a, b in zip(("out", "lse", "dq", "dk", "dv"), got, pad):
        b = b[:, :, :T] if n == "lse" else b[:, :T]
        assert a.shape == b.shape
        assert torch.equal(a, b), (n, (a.double() - b.double()).abs().max().item())


@pytest.mark.parametrize("T", [100, 333])
@pytest.mark.parametrize("W", [None, 48])
@pytest.mark.parametrize("layout", ["view", "cache"])
def test_head256_nothing_at_or_past_T_is_read_or_written(T, W, layout):
    """Through the C ABI: q, k, v are the first T tokens of buffers whose other tokens are NaN, dO / out / lse of the
    backward sit between NaNs, every output is the interior of a sentinel-filled buffer (with B = 2 a store past row T - 1 of
    sequence 0 would land in sequence 1).  The results are finite, the bits of the run on compact copies, no sentinel moved."""
    dtype, B, H, Hkv, Tbuf, nan = torch.bfloat16, 2, 4, 2, T + 60, float("nan")
    g = torch.Generator().manual_seed(T + D)
    qbuf = torch.full((B, Tbuf, H, D), nan, dtype=dtype, device="cuda")
    qbuf[:, :T] = torch.randn(B, T, H, D, generator=g).to("cuda", dtype)
    q = qbuf[:, :T].transpose(1, 2)
    if layout == "view":
        kbuf, vbuf = (torch.full((B, Tbuf, Hkv, D), nan, dtype=dtype, device="cuda") for _ in range(2))
        for t in (kbuf, vbuf):
            t[:, :T] = torch.randn(B, T, Hkv, D, generator=g).to("cuda", dtype)
        k, v = kbuf[:, :T].transpose(1, 2), vbuf[:, :T].transpose(1, 2)
    else:
        kbuf, vbuf = (torch.full((B, Hkv, Tbuf, D), nan, dtype=dtype, device="cuda") for _ in range(2))
        for t in (kbuf, vbuf):
            t[:, :, :T] = torch.randn(B, Hkv, T, D, generator=g).to("cuda", dtype)
        k, v = kbuf[:, :, :T], vbuf[:, :, :T]
    key_mask, mask_off, _ = make_mask("right", B, T)
    go_buf, go = _interior((B, T, H, D), dtype, nan)
    go.copy_(_go(dtype, B, T, H, D, 3))
    want = _run(q.contiguous(), k.contiguous(), v.contiguous(), key_mask, mask_off, go.clone(), SCALE, True, W)
    for n, t in zip(("out", "lse", "dq", "dk", "dv"), want):  # (lse: +inf where a window holds padding only)
        assert t.isnan().sum().item() == 0 and (n == "lse" or torch.isfinite(t).all()), n

    out_buf, out = _interior((B, T, H, D), dtype, 7.0)
    lse_buf, lse = _interior((B, H, T), torch.float32, 7.0)
    assert _lib_fwd(q, k, v, key_mask, mask_off, out, lse, True, W, SCALE) == 0
    assert torch.equal(out, want[0]) and torch.equal(lse, want[1])
    assert _guards_intact(out_buf, 7.0) and _guards_intact(lse_buf, 7.0)
    o_buf, o_in = _interior((B, T, H, D), dtype, nan)
    o_in.copy_(out)
    l_buf, l_in = _interior((B, H, T), torch.float32, nan)
    l_in.copy_(lse)
    del_buf, delta = _interior((B, H, T), torch.float32, 7.0)
    dq_buf, dq = _interior((B, T, H, D), dtype, 7.0)
    dk_buf, dk = _interior((B, T, Hkv, D), dtype, 7.0)
    dv_buf, dv = _interior((B, T, Hkv, D), dtype, 7.0)
    assert _lib_bwd(q, k, v, key_mask, mask_off, o_in, go, l_in, delta, dq, dk, dv, True, W, SCALE) == 0
    assert torch.equal(dq, want[2]) and torch.equal(dk, want[3]) and torch.equal(dv, want[4])
    assert torch.isfinite(delta).all()
    for buf in (del_buf, dq_buf, dk_buf, dv_buf):
        assert _guards_intact(buf, 7.0)


# ---------------------------------------------------------------------------------------------------- 3. decode
def _decode_mask(kind, N, Tk):
    """row 1 right-padded / left-padded by Tk // 3 keys (a left-padded row of Tk = Tq has queries with no visible key)"""
    if kind == "none":
        return None
    m = torch.zeros(N, Tk)
    pad = Tk // 3
    if pad:
        if kind == "right":
            m[1, Tk - pad:] = float("-inf")
        else:
            m[1, :pad] = float("-inf")
    return m.cuda()


def _decode_case(dtype, H, Hkv, Tq, Tk, mask, W):
    from bayeformers_amd import ops

    N = 3
    q, k, v = decode_inputs(dtype, N, H, Hkv, Tq, Tk, D, seed=Tk * 13 + Tq + H + Hkv)
    assert ops.attention_decode_supported(q, k, v)
    key_mask = _decode_mask(mask, N, Tk)
    ref = window_reference(q, k, v, key_mask, SCALE, W if W is not None else Tk + Tq)[0]
    chain = eager_chain(q, k, v, _allowed(N, Tq, Tk, True, W, key_mask), SCALE)
    # exactly the reported workspace, then a guard
    nbytes = ops.attention_decode_workspace_bytes(q, k, v)
    assert nbytes >= 0 and nbytes % 16 == 0
    buf = torch.full((nbytes + 256,), 0x5A, dtype=torch.uint8, device="cuda")
    ws = buf[:nbytes] if nbytes else None
    c0 = dict(ops.DECODE_CALLS)
    out = ops.attention_forward_decode(q, k, v, key_mask, SCALE, workspace=ws, window=W)
    again = ops.attention_forward_decode(q, k, v, key_mask, SCALE, workspace=ws, window=W)
    key = "fwd" if W is None else "window"
    assert ops.DECODE_CALLS[key] - c0[key] == 2
    assert (buf[nbytes:] == 0x5A).all()
    assert out.shape == (N, Tq, H, D) and torch.equal(out, again)
    _hold(f"head256 decode {str(dtype)[6:]} H={H} Hkv={Hkv} Tq={Tq} Tk={Tk} mask={mask} W={W} ws={nbytes}", dtype,
          (out,), chain, (ref,), None)


@DTYPES
@pytest.mark.parametrize("H,Hkv", [(8, 8), (8, 2), (4, 1)])
@pytest.mark.parametrize("Tq", [1, 5, 16])
@pytest.mark.parametrize("Tk", ["Tq", 64, 65, 1000])
@pytest.mark.parametrize("mask", ["none", "right", "left"])
def test_head256_decode_matches_float64_within_twice_the_eager_chain(dtype, H, Hkv, Tq, Tk, mask):
    _decode_case(dtype, H, Hkv, Tq, Tq if Tk == "Tq" else Tk, mask, None)


@DTYPES
@pytest.mark.parametrize("H,Hkv", [(8, 8), (8, 2), (4, 1)])
@pytest.mark.parametrize("Tq", [1, 5, 16])
@pytest.mark.parametrize("Tk", [1000, 30])
@pytest.mark.parametrize("mask", ["none", "left"])
def test_head256_window_decode_matches_float64_within_twice_the_eager_chain(dtype, H, Hkv, Tq, Tk, mask):
    _decode_case(dtype, H, Hkv, Tq, Tk, mask, 48)


@DTYPES
@pytest.mark.parametrize("H,Hkv", [(8, 8), (8, 2), (4, 1)])
@pytest.mark.parametrize("Tq", [1, 5, 16])
@pytest.mark.parametrize("W", [None, 48])
def test_head256_decode_len_is_the_plain_entry_on_the_first_L_keys(dtype, H, Hkv, Tq, W):
    """A cache of capacity 1024 filled to L: bitwise the plain entry at L = 1024; at L < 1024 the keys past L are NaN (never
    read) and the result is the plain entry's on the first L keys bit for bit, and held like it to float64."""
    from bayeformers_amd import ops

    N, cap = 3, 1024
    q, k, v = decode_inputs(dtype, N, H, Hkv, Tq, cap, D, seed=cap + Tq + H + Hkv)
    key_mask = _decode_mask("left", N, cap)
    ws = torch.empty(max(ops.attention_decode_workspace_bytes(q, k, v), 16), dtype=torch.uint8, device="cuda")
    c0 = dict(ops.DECODE_CALLS)
    for L in (Tq, 65, cap):
        kc, vc = k.clone(), v.clone()
        kc[:, :, L:] = float("nan")
        vc[:, :, L:] = float("nan")
        mc = key_mask.clone()
        mc[:, L:] = float("nan")
        Lt = torch.tensor([L], device="cuda")
        got = ops.attention_forward_decode_len(q, kc, vc, Lt, mc, SCALE, workspace=ws, window=W)
        assert torch.equal(got, ops.attention_forward_decode_len(q, kc, vc, Lt, mc, SCALE, workspace=ws, window=W))
        plain = ops.attention_forward_decode(q, k[:, :, :L], v[:, :, :L], key_mask[:, :L].contiguous(), SCALE, window=W)
        assert torch.isfinite(got).all()
        assert torch.equal(got, plain), L  # the split rule applied to L gives the plain entry's splits on L keys
        if L < cap:
            ref = window_reference(q, k[:, :, :L], v[:, :, :L], key_mask[:, :L], SCALE, W if W is not None else cap + Tq)[0]
            chain = eager_chain(q, k[:, :, :L], v[:, :, :L], _allowed(N, Tq, L, True, W, key_mask[:, :L]), SCALE)
            _hold(f"head256 decode_len {str(dtype)[6:]} H={H} Hkv={Hkv} Tq={Tq} L={L} W={W}", dtype, (got,), chain, (ref,),
                  None)
    key = "len" if W is None else "len_window"
    assert ops.DECODE_CALLS[key] - c0[key] == 6


# ---------------------------------------------------------------------------------------------------- 4. refusals
@pytest.mark.parametrize("bad", [96, 512])
def test_head256_entries_still_refuse_other_head_sizes_and_fp32(bad):
    from bayeformers_amd import _C, ops

    lib = _C.lib()
    q, k, v = make_inputs(torch.bfloat16, 1, 128, 4, 2, D, "view", seed=0)
    out = torch.empty(1, 128, 4, D, dtype=torch.bfloat16, device="cuda")
    lse = torch.empty(1, 4, 128, device="cuda")
    grads = [torch.empty(1, 128, h, D, dtype=torch.bfloat16, device="cuda") for h in (4, 2, 2)]
    delta = torch.empty(1, 4, 128, device="cuda")

    def fwd(shape, dt, window=None):
        args = (q.data_ptr(), k.data_ptr(), v.data_ptr(), None, None, out.data_ptr(), lse.data_ptr(), dt, ctypes.byref(shape))
        if window is None:
            return lib.bf_attention_fwd_gqa(*args, SCALE, None)
        return lib.bf_attention_fwd_gqa_window(*args, window, SCALE, None)

    def bwd(shape, dt, window=None):
        args = (q.data_ptr(), k.data_ptr(), v.data_ptr(), None, None, out.data_ptr(), out.data_ptr(), lse.data_ptr(),
                delta.data_ptr(), grads[0].data_ptr(), grads[1].data_ptr(), grads[2].data_ptr(), dt, ctypes.byref(shape))
        if window is None:
            return lib.bf_attention_bwd_gqa(*args, SCALE, None)
        return lib.bf_attention_bwd_gqa_window(*args, window, SCALE, None)

    for call in (fwd, bwd):
        for window in (None, 48):
            shape = ops._gqa_shape(q, k, v, True)
            assert call(shape, _C.BF_DT_F32, window) != 0 and b"bf16 or fp16" in lib.bf_last_error()
            shape.head_dim = bad
            assert call(shape, _C.BF_DT_BF16, window) != 0 and b"head size" in lib.bf_last_error()

    qd, kd, vd = decode_inputs(torch.bfloat16, 1, 4, 2, 1, 64, D, seed=0)
    od = torch.empty(1, 1, 4, D, dtype=torch.bfloat16, device="cuda")
    L = torch.tensor([64], device="cuda")
    for name in ("bf_attention_decode_gqa", "bf_attention_decode_gqa_window", "bf_attention_decode_gqa_len",
                 "bf_attention_decode_gqa_len_window"):
        for dt, hd, text in ((_C.BF_DT_F32, D, b"bf16 or fp16"), (_C.BF_DT_BF16, bad, b"head size")):
            shape = ops._decode_shape(qd, kd, vd)
            shape.head_dim = hd
            args = [qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), None, None, od.data_ptr(), None, dt, ctypes.byref(shape)]
            if "_len" in name:
                args.insert(5, L.data_ptr())
            if name.endswith("_window"):
                args.append(48)
            assert getattr(lib, name)(*args, SCALE, None) != 0 and text in lib.bf_last_error(), name
    shape = ops._decode_shape(qd, kd, vd)
    shape.head_dim = bad
    assert lib.bf_attention_decode_workspace_bytes(ctypes.byref(shape)) < 0 and b"head size" in lib.bf_last_error()
    assert not ops.attention_supported(q.float(), k.float(), v.float(), causal=True)


# ---------------------------------------------------------------------------------------------------- 5. whole models
def _gemma(kind, dtype, fuse=True, **kw):
    """test_gpu_sliding_window._decoder's recipe for a Gemma config with head size 256"""
    from transformers import AutoConfig, AutoModelForCausalLM

    import bayeformers_amd as bf

    cfg = AutoConfig.for_model(kind, hidden_size=256, num_attention_heads=4, num_key_value_heads=2, head_dim=D,
                               num_hidden_layers=2, intermediate_size=512, vocab_size=512, max_position_embeddings=1024,
                               tie_word_embeddings=False, attention_dropout=0.0, attn_implementation="sdpa", **kw)
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


GEMMA3 = dict(sliding_window=100, layer_types=["sliding_attention", "full_attention"])
MODES = (("ref", torch.float32, False), ("sdpa16", torch.bfloat16, False), ("fused", torch.bfloat16, True))


def _prompt(B=2, T=256, pad=37):
    ids = torch.randint(0, 512, (B, T), generator=torch.Generator().manual_seed(11)).cuda()
    mask = torch.ones_like(ids)
    mask[B - 1, T - pad:] = 0  # right padding: no query row without a visible key
    return ids, mask


def test_gemma3_head256_logits_match_the_framework_model():
    """test_sliding_decoder_logits_match_sdpa's criterion on a Gemma 3 decoder with one sliding (W = 100) and one full
    layer of head size 256: the fused bf16 logits against the fp32 framework model, ef <= 2 e16 + 2e-3.  The batch is
    padded, so the framework's side would run its dense-mask form and both layers run the kernels
    (ops.prefill_kernel_wins, profiles/head256_attention.md)."""
    import bayeformers_amd as bf
    from bayeformers_amd import ops
    from bayeformers_amd.sampling import sample_bayesian

    ids, mask = _prompt()
    S, outs = 2, {}
    for name, dtype, fuse in MODES:
        model = _gemma("gemma3_text", dtype, fuse, **GEMMA3)
        assert model.model.model.layers[0].self_attn.head_dim == D
        c0 = dict(ops.GQA_CALLS)
        bf.manual_seed(SEED)
        with torch.no_grad():
            raw, _, _, _ = sample_bayesian(model, {"input_ids": ids, "attention_mask": mask, "use_cache": False}, S)
        outs[name] = raw[0].float().view(S, *ids.shape, -1)
        moved = {k: ops.GQA_CALLS[k] - c0[k] for k in c0}
        assert moved == ({"fwd": 1, "fwd_window": 1, "bwd": 0, "bwd_window": 0} if fuse else dict.fromkeys(c0, 0)), moved
    valid = mask.bool()[None, :, :, None].expand_as(outs["ref"])
    ref = outs["ref"][valid]
    e16 = (outs["sdpa16"][valid] - ref).abs().max().item() / ref.abs().max().item()
    ef = (outs["fused"][valid] - ref).abs().max().item() / ref.abs().max().item()
    print(f"[gemma3 D=256] fused bf16 {ef:.3e}, framework bf16 {e16:.3e} (max |logit - fp32| / max |fp32|)")
    assert ef <= 2 * e16 + 2e-3


def test_gemma3_head256_training_step_runs_the_backward_kernels():
    """One training step (the ELBO of test_recorded_gradients_run_the_plain_forwards): both backward entries run, every
    gradient is finite and the q / k / v projections' mu-gradients are within 2x the bf16 framework model's error against
    the fp32 framework model."""
    from test_gpu_causal_attention import _token_nll

    import bayeformers_amd as bf
    from bayeformers_amd import ops
    from bayeformers_amd.sampling import elbo, sample_bayesian

    ids, mask = _prompt()
    grads = {}
    for name, dtype, fuse in MODES:
        model = _gemma("gemma3_text", dtype, fuse, **GEMMA3)
        for p in model.parameters():
            p.requires_grad_(p.dtype.is_floating_point)
        c0 = dict(ops.GQA_CALLS)
        bf.manual_seed(SEED)
        _, mean, lp, lq = sample_bayesian(model, {"input_ids": ids, "attention_mask": mask, "use_cache": False}, 2)
        loss = elbo(lp, lq, _token_nll(mean[0].float(), ids, mask).double(), 4)
        loss.backward()
        moved = {k: ops.GQA_CALLS[k] - c0[k] for k in c0}
        if fuse:
            assert moved["bwd"] >= 1 and moved["bwd_window"] >= 1 and moved["fwd"] >= 1 and moved["fwd_window"] >= 1, moved
        else:
            assert moved == dict.fromkeys(c0, 0)
        grads[name] = {n: p.grad.double().clone() for n, p in model.named_parameters() if p.grad is not None}
        assert all(torch.isfinite(g).all() for g in grads[name].values())
    assert grads["fused"].keys() == grads["ref"].keys()
    proj = [n for n in grads["ref"] if any(n.endswith(f"{p}_proj.weight.mu") for p in "qkv")]
    assert len(proj) >= 6, sorted(grads["ref"])[:20]
    bad = []
    for n in proj:
        g = grads["ref"][n]
        e16 = rel_err(grads["sdpa16"][n], g)
        ef = rel_err(grads["fused"][n], g)
        print(f"[gemma3 D=256] {n}: fused {ef:.3e}, framework bf16 {e16:.3e}, ratio {ef / max(e16, 1e-30):.2f}")
        if ef > 2 * e16:
            bad.append((n, ef, e16))
    assert not bad, bad


def test_gemma_head256_graph_generation_is_static_and_matches_teacher_forcing():
    """A Gemma decoder, every layer full attention at head size 256, bf16 with kept weights: graph=True returns the
    static_cache=True Generation field for field, bit for bit, the decode steps run bf_attention_decode_gqa_len (the
    prefill carries no mask: its forward stays on SDPA's is_causal form, ops.prefill_kernel_wins), and the greedy tokens are teacher forcing's on the same model."""
    from dataclasses import fields

    import bayeformers_amd as bf
    from bayeformers_amd import ops
    from bayeformers_amd.sampling import mc_predictive, sample_bayesian, sample_generate

    bmodel = _gemma("gemma", torch.bfloat16)
    bf.set_compute_dtype("bf16")
    ids = torch.randint(0, 512, (2, 128), generator=torch.Generator().manual_seed(11)).cuda()
    S, n, T0 = 3, 8, ids.shape[1]
    out = {}
    for mode in ("static_cache", "graph"):
        bf.manual_seed(SEED)
        c0, g0 = dict(ops.DECODE_CALLS), dict(ops.GQA_CALLS)
        with torch.no_grad():
            out[mode] = sample_generate(bmodel, ids, samples=S, max_new_tokens=n, keep_weights=True, **{mode: True})
        assert ops.GQA_CALLS["fwd"] == g0["fwd"]
        if mode == "static_cache":
            assert ops.DECODE_CALLS["len"] - c0["len"] == 2 * (n - 1)
        else:  # enqueued under capture (and its warm-up), replayed after that
            assert ops.DECODE_CALLS["len"] - c0["len"] >= 2
    assert all(torch.equal(getattr(out["graph"], f.name), getattr(out["static_cache"], f.name)) for f in fields(out["graph"]))
    gen = out["graph"]
    bf.manual_seed(SEED)
    with torch.no_grad():
        raw, _, _, _ = sample_bayesian(bmodel, {"input_ids": gen.sequences[:, :-1], "use_cache": False}, S)
    pred = mc_predictive(raw[0][:, :, T0 - 1:])
    assert torch.equal(pred.prediction, gen.sequences[:, T0:])
