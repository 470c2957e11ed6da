"""The causal / grouped-query attention kernels at sequence lengths that are no multiple of 128 (the tail forms of
bf_attention_fwd_gqa / bf_attention_bwd_gqa and their window siblings): against the float64 restatement of
tests/test_gpu_causal_attention.py with that file's bounds, bitwise against the same inputs zero-padded to the next multiple
of 128, "nothing at or past row T is read or written", and the decoders routed through fuse_attention."""
import ctypes

import pytest
import torch

from test_gpu_causal_attention import TOL, make_inputs, make_mask, reference, rel_err
from test_gpu_sliding_window import reference as window_reference

pytestmark = pytest.mark.gpu

SEED = 0x5EED


def _go(dtype, B, T, H, D, seed):
    return torch.randn(B, T, H, D, generator=torch.Generator().manual_seed(seed)).to("cuda", dtype)


def _run(q, k, v, key_mask, mask_off, go, scale, causal=True, window=None):
    """(out, lse, dq, dk, dv) of one forward + backward through the entries; dq [B, T, H, D], dk / dv [B, T, Hkv, D]"""
    from bayeformers_amd import ops

    out, lse = ops.attention_forward_gqa(q, k, v, key_mask, scale, causal, mask_off, want_lse=True, window=window)
    dq, dk, dv = ops.attention_backward_gqa(q, k, v, key_mask, mask_off, out, go, lse, scale, causal, window=window)
    return out, lse, dq, dk, dv


def _check(name, got, ref, dtype, go, finite_lse=True):
    """the comparison of tests/test_gpu_causal_attention.py (its TOL, its lse bound), printed before it is asserted.  Where a
    gradient's reference is exactly zero (T = 1: one key, so dS = P (dP - delta) = 0) the denominator is bounded from below
    by a gradient's noise floor, as tests/test_gpu_sliding_window.py does for W = 1."""
    out, lse, dq, dk, dv = got
    r_out, r_lse, r_dq, r_dk, r_dv = ref
    for t in (out, dq, dk, dv):
        assert torch.isfinite(t).all()
    assert lse.isnan().sum().item() == 0
    fin = torch.isfinite(r_lse)
    assert torch.equal(torch.isfinite(lse), fin)
    lse_err = (lse[fin].double() - r_lse[fin]).abs().max().item() if fin.any() else 0.0
    floor = 1e-3 * go.abs().max().item()
    errs = {"out": rel_err(out, r_out), "dq": _rel(dq, r_dq, floor), "dk": _rel(dk, r_dk, floor), "dv": _rel(dv, r_dv, floor)}
    print(f"{name}: " + " ".join(f"{n}={e:.2e}" for n, e in errs.items()) + f" lse={lse_err:.2e}")
    assert lse_err < 2e-2
    for n, e in errs.items():
        assert e <= TOL[dtype][n], (n, e)


def _rel(a, r, floor):
    return (a.double() - r).abs().max().item() / max(r.abs().max().item(), floor)


# ---------------------------------------------------------------------------------------------------- 1. float64
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("H,Hkv", [(4, 4), (8, 2), (4, 1)])
@pytest.mark.parametrize("T", [1, 15, 17, 100, 127, 129, 200, 257, 385])
@pytest.mark.parametrize("mask", ["none", "right", "left"])
@pytest.mark.parametrize("layout", ["view", "cache"])
def test_ragged_causal_gqa_matches_float64(dtype, D, H, Hkv, T, mask, layout):
    from bayeformers_amd import ops

    if mask != "none" and T < 9:
        pytest.skip("make_mask's padding formula needs T >= 9")
    B = 2
    q, k, v = make_inputs(dtype, B, T, H, Hkv, D, layout, seed=T * 31 + H * 7 + Hkv + D)
    assert ops.attention_supported(q, k, v, causal=True, kv_heads=Hkv)
    key_mask, mask_off, keep = make_mask(mask, B, T)
    scale = D ** -0.5
    go = _go(dtype, B, T, H, D, T + D)
    qr, kr, vr = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    out = ops.AttentionGqaFn.apply(qr, kr, vr, key_mask, mask_off, scale, True)
    out.backward(go)
    out2, lse = ops.attention_forward_gqa(q, k, v, key_mask, scale, True, mask_off, want_lse=True)
    assert torch.equal(out, out2)
    dq, dk, dv = qr.grad.transpose(1, 2), kr.grad.transpose(1, 2), vr.grad.transpose(1, 2)
    _check(f"ragged causal gqa {str(dtype)[6:]} D={D} H={H} Hkv={Hkv} T={T} mask={mask} layout={layout}",
           (out, lse, dq, dk, dv), reference(q, k, v, key_mask, scale, True, go), dtype, go)
    if mask == "left":  # rows of the padding that see no key at all: exactly 0, gradients 0, lse = +inf
        dead = ~keep[1].cuda() & (torch.arange(T, device="cuda") < (~keep[1]).sum().item())
        assert dead.any()
        assert (out[1][dead] == 0).all() and (dq[1][dead] == 0).all()
        assert (dk[1][dead] == 0).all() and (dv[1][dead] == 0).all()
        assert (lse[1][:, dead] == float("inf")).all()


# ---------------------------------------------------------------------------------------------------- 2. the padded launch
def _zero_extend(t, dim, Tp):
    shape = list(t.shape)
    shape[dim] = Tp - t.shape[dim]
    return torch.cat([t, torch.zeros(shape, dtype=t.dtype, device=t.device)], dim)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("T", [100, 200, 300])
@pytest.mark.parametrize("mode", ["causal", "W1", "W50", "W129", "non_causal"])
def test_ragged_is_bitwise_the_padded_launch(dtype, D, T, mode):
    """The same inputs zero-extended to the next multiple of 128 (dO = 0 on the added rows; non-causal: the added keys
    masked with -inf) run the instantiations the project always had; rows < T of every result are the same bits."""
    B, H, Hkv = 2, 8, 2
    Tp = (T + 127) // 128 * 128
    causal = mode != "non_causal"
    window = int(mode[1:]) if mode.startswith("W") else None
    q, k, v = make_inputs(dtype, B, T, H, Hkv, D, "cache", seed=T + D)
    go = _go(dtype, B, T, H, D, 7)
    scale = D ** -0.5
    got = _run(q, k, v, None, None, go, scale, causal, window)
    qp, kp, vp = (_zero_extend(t, 2, Tp) for t in (q, k, v))
    key_mask = mask_off = None
    if not causal:
        key_mask = torch.zeros(B, Tp, device="cuda")
        key_mask[:, T:] = float("-inf")
        mask_off = torch.zeros(1, dtype=torch.bool, device="cuda")
    pad = _run(qp, kp, vp, key_mask, mask_off, _zero_extend(go, 1, Tp), scale, causal, window)
    names = ("out", "lse", "dq", "dk", "dv")
    for n, a, b in zip(names, got, pad):
        b = b[:, :, :T] if n == "lse" else b[:, :T]
        assert a.shape == b.shape
        assert torch.equal(a, b), (n, (a.double() - b.double()).abs().max().item())


# ---------------------------------------------------------------------------------------------------- 3. nothing past T
def _lib_fwd(q, k, v, mask, mask_off, out, lse, causal, window, scale):
    from bayeformers_amd import _C, ops

    shape = ops._gqa_shape(q, k, v, causal)
    ptr = lambda t: t.data_ptr() if t is not None else None
    args = (q.data_ptr(), k.data_ptr(), v.data_ptr(), ptr(mask), ptr(mask_off), out.data_ptr(), ptr(lse),
            ops._TORCH2BF[q.dtype], ctypes.byref(shape))
    stream = ops._stream_ptr()
    if window is None:
        return _C.lib().bf_attention_fwd_gqa(*args, float(scale), stream)
    return _C.lib().bf_attention_fwd_gqa_window(*args, int(window), float(scale), stream)


def _lib_bwd(q, k, v, mask, mask_off, out, go, lse, delta, dq, dk, dv, causal, window, scale):
    from bayeformers_amd import _C, ops

    shape = ops._gqa_shape(q, k, v, causal)
    ptr = lambda t: t.data_ptr() if t is not None else None
    args = (q.data_ptr(), k.data_ptr(), v.data_ptr(), ptr(mask), ptr(mask_off), out.data_ptr(), go.data_ptr(),
            lse.data_ptr(), delta.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), ops._TORCH2BF[q.dtype],
            ctypes.byref(shape))
    stream = ops._stream_ptr()
    if window is None:
        return _C.lib().bf_attention_bwd_gqa(*args, float(scale), stream)
    return _C.lib().bf_attention_bwd_gqa_window(*args, int(window), float(scale), stream)


GUARD = 64  # elements on either side of an interior: 128 / 256 bytes, so the interior keeps the 16-byte alignment


def _interior(shape, dtype, fill):
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((GUARD + n + GUARD,), fill, dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + n].view(shape)


def _guards_intact(buf, fill):
    return bool((buf[:GUARD] == fill).all() and (buf[-GUARD:] == fill).all())


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("T", [100, 130])
@pytest.mark.parametrize("mode", ["causal", "W50", "non_causal"])
@pytest.mark.parametrize("layout", ["view", "cache"])
def test_nothing_at_or_past_T_is_read_or_written(D, T, mode, layout):
    """q, k, v: the first T tokens of buffers whose other tokens are NaN (a read of token >= T would poison the result);
    every output: the interior of a sentinel-filled buffer.  The results are the bits of the run on compact copies and no
    sentinel moved; with B = 2 a store past row T - 1 of sequence 0 would land in sequence 1 and break the equality."""
    dtype, B, H, Hkv, Tbuf = torch.bfloat16, 2, 4, 2, T + 60
    causal = mode != "non_causal"
    window = int(mode[1:]) if mode.startswith("W") else None
    scale = D ** -0.5
    g = torch.Generator().manual_seed(T + D)
    nan = float("nan")
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

    want = _run(q.contiguous(), k.contiguous(), v.contiguous(), key_mask, mask_off, go.clone(), scale, causal, window)

    out_buf, out = _interior((B, T, H, D), dtype, 7.0)
    lse_buf, lse = _interior((B, H, T), torch.float32, 7.0)
    assert _lib_fwd(q, k, v, key_mask, mask_off, out, lse, causal, window, scale) == 0
    assert torch.equal(out, want[0]) and torch.equal(lse, want[1])
    assert _guards_intact(out_buf, 7.0) and _guards_intact(lse_buf, 7.0)
    # the backward reads the output between NaNs
    o_buf, o_in = _interior((B, T, H, D), dtype, nan)
    o_in.copy_(out)
    l_buf, l_in = _interior((B, H, T), torch.float32, nan)
    l_in.copy_(lse)
    del_buf, delta = _interior((B, H, T), torch.float32, 7.0)
    dq_buf, dq = _interior((B, T, H, D), dtype, 7.0)
    dk_buf, dk = _interior((B, T, Hkv, D), dtype, 7.0)
    dv_buf, dv = _interior((B, T, Hkv, D), dtype, 7.0)
    assert _lib_bwd(q, k, v, key_mask, mask_off, o_in, go, l_in, delta, dq, dk, dv, causal, window, scale) == 0
    assert torch.equal(dq, want[2]) and torch.equal(dk, want[3]) and torch.equal(dv, want[4])
    assert torch.isfinite(delta).all()
    for buf in (del_buf, dq_buf, dk_buf, dv_buf):
        assert _guards_intact(buf, 7.0)


# ---------------------------------------------------------------------------------------------------- 4. window
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("D,H,Hkv", [(64, 8, 2), (128, 4, 1), (128, 4, 4)])
@pytest.mark.parametrize("W", [1, 50, 128, 129, 4096])
def test_ragged_window_matches_float64(dtype, D, H, Hkv, W):
    B, T = 2, 200
    q, k, v = make_inputs(dtype, B, T, H, Hkv, D, "view", seed=W + D + H)
    key_mask, mask_off, _ = make_mask("left", B, T)
    scale = D ** -0.5
    go = _go(dtype, B, T, H, D, W)
    got = _run(q, k, v, key_mask, mask_off, go, scale, True, W)
    _check(f"ragged window gqa {str(dtype)[6:]} D={D} H={H} Hkv={Hkv} T={T} W={W}", got,
           window_reference(q, k, v, key_mask, scale, W, go), dtype, go)
    if W >= T:  # a window that hides nothing: the plain entries' bits
        for a, b in zip(got, _run(q, k, v, key_mask, mask_off, go, scale, True, None)):
            assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------- 5. entries
def test_entry_refuses_T_0_and_a_misaligned_mask():
    from bayeformers_amd import _C, ops

    q, k, v = make_inputs(torch.bfloat16, 2, 100, 4, 2, 64, "view", seed=0)
    out = torch.empty(2, 100, 4, 64, dtype=torch.bfloat16, device="cuda")
    shape = ops._gqa_shape(q, k, v, True)
    shape.T = 0
    rc = _C.lib().bf_attention_fwd_gqa(q.data_ptr(), k.data_ptr(), v.data_ptr(), None, None, out.data_ptr(), None,
                                       _C.BF_DT_BF16, ctypes.byref(shape), 0.125, None)
    assert rc != 0 and b"T=0" in _C.lib().bf_last_error()
    mask = torch.zeros(2 * 100 + 1, device="cuda")[1:].view(2, 100)
    assert mask.data_ptr() % 16 == 4
    assert _lib_fwd(q, k, v, mask, None, out, None, True, None, 0.125) != 0
    assert b"aligned" in _C.lib().bf_last_error()
    assert _lib_fwd(q, k, v, mask, None, out, None, True, 50, 0.125) != 0
    assert b"aligned" in _C.lib().bf_last_error()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("D,H,Hkv,layout", [(64, 4, 4, "view"), (64, 8, 2, "cache"), (128, 4, 1, "view")])
def test_ragged_non_causal_matches_float64(dtype, D, H, Hkv, layout):
    """causal = 0 at T = 100.  (64, 4, 4, "view") is the BERT kernels' case (one K/V head per query head, head size 64,
    packed strides) at a length they do not take: it runs the generic non-causal kernel."""
    B, T = 2, 100
    q, k, v = make_inputs(dtype, B, T, H, Hkv, D, layout, seed=5 + D + Hkv)
    key_mask, mask_off, _ = make_mask("right", B, T)
    scale = D ** -0.5
    go = _go(dtype, B, T, H, D, 3)
    got = _run(q, k, v, key_mask, mask_off, go, scale, False)
    _check(f"ragged non-causal gqa {str(dtype)[6:]} D={D} H={H} Hkv={Hkv}", got, reference(q, k, v, key_mask, scale, False, go),
           dtype, go)


# ---------------------------------------------------------------------------------------------------- 6. capture
@pytest.mark.parametrize("D,window", [(64, None), (128, 70)])
def test_captured_ragged_forward_backward_replays_bitwise(D, window):
    """No allocation of the library's and no synchronisation in the entries: a ragged forward + backward is captured on a
    side stream and every replay gives the eager bits."""
    dtype, B, T, H, Hkv = torch.bfloat16, 2, 201, 8, 2
    q, k, v = make_inputs(dtype, B, T, H, Hkv, D, "view", seed=D)
    key_mask, mask_off, _ = make_mask("right", B, T)
    go = _go(dtype, B, T, H, D, 1)
    scale = D ** -0.5
    eager = [t.clone() for t in _run(q, k, v, key_mask, mask_off, go, scale, True, window)]
    static = [torch.zeros_like(t) for t in eager]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _run(q, k, v, key_mask, mask_off, go, scale, True, window)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for dst, src in zip(static, _run(q, k, v, key_mask, mask_off, go, scale, True, window)):
            dst.copy_(src)
    for _ in range(3):
        for t in static:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(static, eager):
            assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------- 7. models
FAMILIES = {"llama": {}, "mistral": dict(sliding_window=64)}
LAYERS = 2


def _decoder(kind, dtype, fuse):
    """as tests/test_gpu_sliding_window.py builds its decoders"""
    from transformers import AutoConfig, AutoModelForCausalLM

    import bayeformers_amd as bf

    cfg = AutoConfig.for_model(kind, hidden_size=256, num_attention_heads=4, num_key_value_heads=2, head_dim=64,
                               num_hidden_layers=LAYERS, intermediate_size=512, vocab_size=512, max_position_embeddings=1024,
                               tie_word_embeddings=False, attention_dropout=0.0, attn_implementation="sdpa", **FAMILIES[kind])
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


def _batch(T, pad):
    ids = torch.randint(0, 512, (2, T), generator=torch.Generator().manual_seed(11)).cuda()
    mask = torch.ones_like(ids)
    mask[1, T - pad:] = 0  # right padding: no query row without a visible key
    return ids, mask


@pytest.mark.parametrize("kind", list(FAMILIES))
@pytest.mark.parametrize("T", [100, 130])
def test_ragged_decoder_logits_and_gradients_match_sdpa(kind, T):
    """One Monte-Carlo training loss at a ragged length: the fused bf16 model against the same Bayesian model on the
    framework's attention in fp32, held to tests/test_gpu_sliding_window.py's criteria (twice the bf16 framework model's own
    error, plus 2e-3 for the logits and 1e-2 for each parameter's gradient); every layer ran the kernels, both ways."""
    import bayeformers_amd as bf
    from bayeformers_amd import ops
    from bayeformers_amd.sampling import sample_bayesian

    ids, mask = _batch(T, pad=21)
    S = 2
    logits, grads = {}, {}
    key = "_window" if kind == "mistral" else ""
    for name, dtype, fuse in (("ref", torch.float32, False), ("sdpa16", torch.bfloat16, False), ("fused", torch.bfloat16, True)):
        model = _decoder(kind, dtype, fuse)
        for p in model.parameters():
            p.requires_grad_(p.dtype.is_floating_point)
        c0 = dict(ops.GQA_CALLS)
        bf.manual_seed(SEED)
        raw, mean, _, _ = sample_bayesian(model, {"input_ids": ids, "attention_mask": mask, "use_cache": False}, S)
        if fuse:
            assert ops.GQA_CALLS["fwd" + key] - c0["fwd" + key] == LAYERS
        loss = torch.nn.functional.cross_entropy(mean[0].float()[:, :-1].reshape(-1, 512), ids[:, 1:].reshape(-1))
        loss.backward()
        if fuse:
            assert ops.GQA_CALLS["bwd" + key] - c0["bwd" + key] == LAYERS
        logits[name] = raw[0].detach().float().view(S, *ids.shape, -1)
        grads[name] = {n: p.grad.double().clone() for n, p in model.named_parameters() if p.grad is not None}
    valid = mask.bool()[None, :, :, None].expand_as(logits["ref"])
    ref = logits["ref"][valid]
    e16 = (logits["sdpa16"][valid] - ref).abs().max().item() / ref.abs().max().item()
    ef = (logits["fused"][valid] - ref).abs().max().item() / ref.abs().max().item()
    print(f"[{kind} T={T}] fused bf16 {ef:.3e}, framework bf16 {e16:.3e} (max |logit - fp32| / max |fp32|)")
    assert ef <= 2 * e16 + 2e-3
    assert grads["fused"].keys() == grads["ref"].keys() and grads["ref"]
    worst = 0.0
    for n, g in grads["ref"].items():
        scale = max(g.norm().item(), 1e-30)
        g16 = (grads["sdpa16"][n] - g).norm().item() / scale
        gf = (grads["fused"][n] - g).norm().item() / scale
        worst = max(worst, gf - 2 * g16)
        assert gf <= 2 * g16 + 1e-2, (n, gf, g16)
    print(f"[{kind} T={T}] gradients: max(fused - 2 x framework bf16) = {worst:.3e}")


@pytest.mark.parametrize("kind", list(FAMILIES))
def test_switch_off_sends_ragged_lengths_to_the_framework(kind, monkeypatch):
    import bayeformers_amd as bf
    from bayeformers_amd import ops
    from bayeformers_amd.sampling import sample_bayesian

    monkeypatch.delenv("BF_NO_RAGGED_ATTENTION", raising=False)
    model = _decoder(kind, torch.bfloat16, True)
    ids, mask = _batch(100, pad=21)
    inputs = {"input_ids": ids, "attention_mask": mask, "use_cache": False}
    key = "fwd_window" if kind == "mistral" else "fwd"
    try:
        for on in (False, True):
            bf.ragged_attention(on)
            c0 = dict(ops.GQA_CALLS)
            bf.manual_seed(SEED)
            with torch.no_grad():
                sample_bayesian(model, inputs, 2)
            moved = {n: ops.GQA_CALLS[n] - c0[n] for n in c0}
            assert moved == ({n: (LAYERS if n == key else 0) for n in c0} if on else {n: 0 for n in c0}), (on, moved)
        monkeypatch.setenv("BF_NO_RAGGED_ATTENTION", "1")  # the environment switches it off too
        c0 = dict(ops.GQA_CALLS)
        with torch.no_grad():
            sample_bayesian(model, inputs, 2)
        assert ops.GQA_CALLS == c0
    finally:
        bf.ragged_attention(True)


# ---------------------------------------------------------------------------------------------------- 8. generation
def test_generation_prefill_of_a_ragged_prompt_runs_the_kernels():
    """sample_generate on a 37-token bf16 prompt with a left-padded row: the prefill is one causal launch per layer, and
    the graph-replayed generation is bitwise the static-cache one."""
    from bayeformers_amd import ops
    from test_gpu_generate_graph import _equal, _gen, _llama, _prompt, _settle

    bmodel = _llama(torch.bfloat16)
    layers = 2
    ids, mask = _prompt(T=37, pad=5)
    c0 = ops.GQA_CALLS["fwd"]
    _settle(bmodel, ids, mask)
    assert ops.GQA_CALLS["fwd"] - c0 == layers
    c1 = ops.GQA_CALLS["fwd"]
    static = _gen(bmodel, ids, mask, static_cache=True, max_new_tokens=12)
    assert ops.GQA_CALLS["fwd"] - c1 == layers
    c2 = ops.GQA_CALLS["fwd"]
    graph = _gen(bmodel, ids, mask, graph=True, max_new_tokens=12)
    assert ops.GQA_CALLS["fwd"] - c2 == layers
    assert _equal(static, graph)
    assert (graph.token_prob > 0).all()
