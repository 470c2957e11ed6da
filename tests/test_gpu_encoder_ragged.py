"""The any-length encoder attention entries (include/bayeformers_amd_encoder_any.h: the tail forms of the kernels of
csrc/bf_attention.hip and csrc/bf_attention_bwd.hip) against the float64 restatement of tests/attention_ref.py, bitwise
against the existing entries on padded sequences and at a multiple of 128, with dropout against the oracle's mask
(tests/encoder_any_ref.py), for reads outside the tensors, and through the model-level route under
bayeformers_amd.encoder_ragged_attention().

Launched through ctypes with guarded buffers, as tests/test_gpu_encoder_attention.py does; B = 2 on purpose: a store past
one sequence's end lands in the next one's rows."""
import types

import numpy as np
import pytest
import torch

import bayeformers_amd as bf
from attention_ref import attention_ref
from encoder_any_ref import attention_keep_mask_any, keep_words_any, padded_length
from oracle import bayes_oracle as bo
from test_gpu_encoder_attention import (HD, LSE_ABS, SEED, TOL, Guarded, bf_dtype, compare, flag, make_inputs, make_mask,
                                        name_of, ptr, rel_err, run_packed)

pytestmark = pytest.mark.gpu

DT = [torch.bfloat16, torch.float16]
DT_IDS = ["bf16", "fp16"]
LENGTHS = [1, 17, 127, 129, 200, 300]
B, H = 2, 2
SCALE = 0.125
NAN_PAD = 4096  # elements of NaN on either side of an operand (a multiple of 8: the operand stays 16-byte aligned)


def nan_wrapped(t):
    """A copy of the contiguous tensor t in the middle of a buffer whose other words are NaN."""
    buf = torch.full((t.numel() + 2 * NAN_PAD,), float("nan"), dtype=t.dtype, device=t.device)
    buf[NAN_PAD:NAN_PAD + t.numel()] = t.reshape(-1)
    out = buf[NAN_PAD:NAN_PAD + t.numel()].view(t.shape)
    assert out.data_ptr() % 16 == 0
    return out


def launch_any(dtype, q, k, v, mask, mask_off, scale, go=None, drop=None, first_group=0, wrap=False):
    """bf_attention_fwd_any[_dropout] and, given go, bf_attention_bwd_any[_dropout] through ctypes on [B, H, T, 64] views of
    packed [B, T, H*64] operands; drop = (p, seed, call, site); wrap: q, k, v and go are copied into NaN-surrounded
    buffers first.  Every output sits between guard bands (which are NaN patterns: the forward's out, an operand of the
    backward, is NaN-surrounded as well)."""
    from bayeformers_amd import _C, ops

    lib, st = _C.lib(), ops._stream_ptr()
    Bq, Hq, T, _ = q.shape
    qp, kp, vp = (t.transpose(1, 2).contiguous() for t in (q, k, v))  # packed [B, T, H, 64]
    if wrap:
        qp, kp, vp = (nan_wrapped(t) for t in (qp, kp, vp))
        go = None if go is None else nan_wrapped(go)
    n, words = Bq * T * Hq * HD, padded_length(T) // 32
    g = {"out": Guarded(n, dtype), "lse": Guarded(Bq * Hq * T, torch.float32)}
    r = types.SimpleNamespace(keep=None, delta=None, dq=None, dk=None, dv=None)
    common = (bf_dtype(dtype), Bq, T, Hq, HD, Hq * HD, float(scale))
    if drop is not None:
        p, seed, call, site = drop
        g["keep"] = Guarded(Bq * Hq * T * words, torch.int32)
        rc = lib.bf_attention_fwd_any_dropout(ptr(qp), ptr(kp), ptr(vp), ptr(mask), ptr(mask_off), ptr(g["out"].t),
                                              ptr(g["lse"].t), *common, p, seed, call, site, first_group, ptr(g["keep"].t),
                                              None, st)
        r.keep = g["keep"].t.view(Bq, Hq, T, words)
    else:
        rc = lib.bf_attention_fwd_any(ptr(qp), ptr(kp), ptr(vp), ptr(mask), ptr(mask_off), ptr(g["out"].t), ptr(g["lse"].t),
                                      *common, st)
    assert rc == 0, lib.bf_last_error()
    r.out, r.lse = g["out"].t.view(Bq, T, Hq, HD), g["lse"].t.view(Bq, Hq, T)
    if go is not None:
        assert go.is_contiguous() and go.dtype == dtype and go.numel() == n
        g["delta"] = Guarded(Bq * Hq * T, torch.float32)
        for name in ("dq", "dk", "dv"):
            g[name] = Guarded(n, dtype)
        head = (ptr(qp), ptr(kp), ptr(vp), ptr(mask), ptr(mask_off), ptr(r.out), ptr(go), ptr(r.lse), ptr(g["delta"].t),
                ptr(g["dq"].t), ptr(g["dk"].t), ptr(g["dv"].t)) + common
        if drop is not None:
            rc = lib.bf_attention_bwd_any_dropout(*head, drop[0], ptr(r.keep), st)
        else:
            rc = lib.bf_attention_bwd_any(*head, st)
        assert rc == 0, lib.bf_last_error()
        r.delta = g["delta"].t.view(Bq, Hq, T)
        r.dq, r.dk, r.dv = (g[x].t.view(Bq, T, Hq, HD) for x in ("dq", "dk", "dv"))
    torch.cuda.synchronize()
    for name, gd in g.items():
        assert gd.intact(), f"the guard bands around {name} were written"
    return r


def inputs(dtype, T, seed, nb=B, nh=H):
    return make_inputs(dtype, nb, T, nh, seed=seed)


NAMES = ("out", "lse", "delta", "dq", "dk", "dv")


def check(r, ref, dtype, label, q, k, v, go):
    """compare() of tests/test_gpu_encoder_attention.py, its bounds unchanged.  T = 1 alone needs a word: the one
    probability is 1, so dS = P (dP - delta) = go.v - go.out is 0 in exact arithmetic and the float64 dq and dk are
    identically zero — "relative to max |reference|" has no denominator.  There the two are held to the same TOL relative
    to the size of the one term that cancels, scale * max |go.v| * max |k| (dq) or max |q| (dk); every other quantity, and
    every other length, goes through compare() as it stands."""
    if q.shape[2] > 1 or not torch.isfinite(ref.lse).any():  # (T = 1 with its key hidden: exact zeros, compare() as it is)
        return compare(r, ref, dtype, label)
    assert torch.isfinite(ref.lse).all()
    assert ref.dq.abs().max().item() == 0 and ref.dk.abs().max().item() == 0
    tol = TOL[dtype]
    for name in NAMES:
        assert torch.isfinite(getattr(r, name)).all(), name
    errs = {"out": rel_err(r.out, ref.out), "delta": rel_err(r.delta, ref.delta), "dv": rel_err(r.dv, ref.dv)}
    lse_err = (r.lse.double() - ref.lse).abs().max().item()
    dp = torch.einsum("bthd,bhtd->bht", go.double(), v.double()).abs().max().item()
    zero = {"dq": r.dq.double().abs().max().item() / (SCALE * dp * k.double().abs().max().item()),
            "dk": r.dk.double().abs().max().item() / (SCALE * dp * q.double().abs().max().item())}
    tols = dict(tol, delta=tol["dq"])
    print(f"[enc-any] {label} " + " ".join(f"{n}={e:.3e}/{e / tols[n]:.2f}" for n, e in {**errs, **zero}.items())
          + f" lse={lse_err:.3e}/{lse_err / LSE_ABS:.2f}")
    assert lse_err <= LSE_ABS
    for n, e in {**errs, **zero}.items():
        assert e <= tols[n], (n, e, tols[n])


# ------------------------------------------------------------------------------------------------- 1. float64 agreement
@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("kind", ["none", "right", "left", "holes"])
@pytest.mark.parametrize("T", LENGTHS)
def test_every_length_matches_float64(dtype, kind, T):
    """out, lse, delta, dq, dk, dv at every length and mask kind, in the bounds of tests/test_gpu_encoder_attention.py (the
    same kernels, the same quantities).  `left` hides every key of the short lengths: empty rows, out = 0 and lse = +inf."""
    q, k, v, go = inputs(dtype, T, seed=T * 31 + 5)
    mask = make_mask(kind, B, T)
    r = launch_any(dtype, q, k, v, mask, None, SCALE, go)
    ref = attention_ref(q, k, v, mask, SCALE, go=go)
    check(r, ref, dtype, f"any-length dtype={name_of(dtype)} T={T} mask={kind}:", q, k, v, go)


# ------------------------------------------------------------------------------------------ 2. bitwise vs the padded run
@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("kind", ["none", "right"])
@pytest.mark.parametrize("T", LENGTHS)
def test_forward_is_bitwise_the_existing_kernel_on_the_padded_sequence(dtype, kind, T):
    """Rows < T of out and lse: bit for bit bf_attention_fwd at Tp on operands padded with arbitrary finite rows and -inf on
    the pad keys.  The backward (dO padded with zeros) is printed, and asserted against float64 only."""
    Tp = padded_length(T)
    q, k, v, go = inputs(dtype, T, seed=T * 17 + 3)
    mask = make_mask(kind, B, T)
    r = launch_any(dtype, q, k, v, mask, None, SCALE, go)
    qp, kp, vp, gop = inputs(dtype, Tp, seed=T + 1000)           # arbitrary finite pad rows
    for dst, src in ((qp, q), (kp, k), (vp, v)):
        dst[:, :, :T] = src                                      # (views of the packed tensors: written in place)
    gop[:, :T] = go
    gop[:, T:] = 0
    mp = torch.full((B, Tp), float("-inf"), device="cuda")
    mp[:, :T] = 0.0 if mask is None else mask
    rp = run_packed(qp, kp, vp, mp, None, SCALE, gop)
    assert torch.equal(r.out, rp.out[:, :T]) and torch.equal(r.lse, rp.lse[:, :, :T])
    same = {n: torch.equal(getattr(r, n), getattr(rp, n)[:, :T]) for n in ("dq", "dk", "dv")}
    same["delta"] = torch.equal(r.delta, rp.delta[:, :, :T])
    print(f"[enc-any] padded-run backward bitwise dtype={name_of(dtype)} T={T} mask={kind}: {same}")
    check(r, attention_ref(q, k, v, mask, SCALE, go=go), dtype, f"any-length (padded-run case) dtype={name_of(dtype)} T={T}:",
          q, k, v, go)


# --------------------------------------------------------------------------------------- 3. T = 256 through the new entries
@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_a_multiple_of_128_gives_the_existing_entries_bits(dtype, p):
    T = 256
    q, k, v, go = inputs(dtype, T, seed=99)
    mask = make_mask("holes", B, T)
    drop = (p, SEED, 3, 4) if p else None
    a = launch_any(dtype, q, k, v, mask, None, SCALE, go, drop=drop)
    b = run_packed(q, k, v, mask, None, SCALE, go, drop=drop)
    for n in NAMES + (("keep",) if p else ()):
        assert torch.equal(getattr(a, n), getattr(b, n)), n


# ------------------------------------------------------------------------------------------------------------ 4. dropout
@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("p", [0.1, 0.25])
@pytest.mark.parametrize("T", [100, 300])
def test_dropout_matches_float64_with_the_oracles_mask(dtype, p, T):
    """The DROP tail forms: the keep words of the keys < T against the oracle's mask, the results against float64 with that
    mask in the bounds of tests/test_gpu_dropout.py, and a second call number far away."""
    call, site = 5, 9
    q, k, v, go = inputs(dtype, T, seed=T + int(p * 100))
    mask = make_mask("right", B, T) if T == 300 else None
    full = torch.from_numpy(attention_keep_mask_any(B, H, T, p, SEED, call, site, with_pad_keys=True)).cuda()
    keep = full[..., :T].contiguous()
    assert torch.equal(keep.cpu(), torch.from_numpy(attention_keep_mask_any(B, H, T, p, SEED, call, site)))
    assert abs(float(keep.double().mean()) - (1 - p)) < 0.01
    r = launch_any(dtype, q, k, v, mask, None, SCALE, go, drop=(p, SEED, call, site))
    valid = torch.zeros_like(full)
    valid[..., :T] = 1
    assert torch.equal(r.keep & keep_words_any(valid), keep_words_any(full * valid))  # (bits of keys >= T: meaningless)
    ref = attention_ref(q, k, v, mask, SCALE, keep=keep, p=p, go=go)
    bf16 = dtype == torch.bfloat16
    tol_o, tol_g = (2.0 ** -7, 2.0 ** -6) if bf16 else (2.0 ** -10, 2.0 ** -9)
    ref_max = ref.out.abs().max().item()
    e_out = (r.out.double() - ref.out).abs().max().item()
    errs = {n: rel_err(getattr(r, n), getattr(ref, n)) for n in ("dq", "dk", "dv", "delta")}
    lse_err = (r.lse.double() - ref.lse).abs().max().item()
    other = launch_any(dtype, q, k, v, mask, None, SCALE, drop=(p, SEED, call + 1, site))
    e_other = (other.out.double() - ref.out).abs().max().item()
    print(f"[enc-any] dropout dtype={name_of(dtype)} T={T} p={p}: out={e_out:.3e}/{e_out / (tol_o * ref_max + 1e-3):.2f} "
          + " ".join(f"{n}={e:.3e}/{e / tol_g:.2f}" for n, e in errs.items())
          + f" lse={lse_err:.3e}/{lse_err / LSE_ABS:.2f} other-call={e_other / (tol_o * ref_max):.1f}x")
    assert e_out <= tol_o * ref_max + 1e-3
    for n, e in errs.items():
        assert e <= tol_g, (n, e)
    assert lse_err <= LSE_ABS
    assert e_other > 20 * tol_o * ref_max


# ---------------------------------------------------------------------------------------------- 5. reads outside the tensors
@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("T", [1, 129, 300])
def test_nothing_outside_the_tensors_is_read_or_written(dtype, p, T):
    """Q, K, V, O and dO lie between NaN words: a row read past the end would reach an accumulator as 0 * NaN.  Every output
    is finite and the guard bands around every output are intact (asserted in launch_any)."""
    q, k, v, go = inputs(dtype, T, seed=T + 7)
    mask = make_mask("holes", B, T) if T == 300 else None
    drop = (p, SEED, 2, 3) if p else None
    r = launch_any(dtype, q, k, v, mask, None, SCALE, go, drop=drop, wrap=True)
    for n in NAMES:
        assert torch.isfinite(getattr(r, n)).all(), n
    plain = launch_any(dtype, q, k, v, mask, None, SCALE, go, drop=drop)
    for n in NAMES:
        assert torch.equal(getattr(r, n), getattr(plain, n)), n


# ------------------------------------------------------------------------------------------------------------ 6. rows entry
@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("q_rows", [1, 16])
@pytest.mark.parametrize("T", [100, 300])
def test_rows_entry_is_bitwise_the_full_kernels_first_rows(dtype, q_rows, T):
    from bayeformers_amd import _C, ops

    q, k, v, _ = inputs(dtype, T, seed=T + q_rows)
    mask = make_mask("right", B, T)
    off = flag(0)
    full = launch_any(dtype, q, k, v, mask, off, SCALE)
    out = Guarded(B * q_rows * H * HD, dtype)
    qp, kp, vp = (nan_wrapped(t.transpose(1, 2).contiguous()) for t in (q, k, v))
    rc = _C.lib().bf_attention_fwd_any_rows(ptr(qp), ptr(kp), ptr(vp), ptr(mask), ptr(off), ptr(out.t), bf_dtype(dtype), B, T,
                                            H, HD, H * HD, q_rows, SCALE, ops._stream_ptr())
    assert rc == 0, _C.lib().bf_last_error()
    torch.cuda.synchronize()
    assert out.intact()
    assert torch.equal(out.t.view(B, q_rows, H, HD), full.out[:, :q_rows])
    calls = ops.ENCODER_ANY_CALLS["rows"]
    got = ops.attention_forward_rows_any(q, k, v, mask, SCALE, off, q_rows=q_rows)
    assert torch.equal(got, full.out[:, :q_rows]) and ops.ENCODER_ANY_CALLS["rows"] == calls + 1


# -------------------------------------------------------------------------------------------------------- 7. edge semantics
@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("T", [17, 200])
def test_a_fully_masked_sequence_is_exact_zeros_and_a_batch_is_its_sequences(dtype, T):
    nb = 3
    q, k, v, go = inputs(dtype, T, seed=T + 1, nb=nb)
    mask = torch.zeros(nb, T, device="cuda")
    mask[1] = float("-inf")
    mask[2, T - 5:] = float("-inf")
    a = launch_any(dtype, q, k, v, mask, flag(0), SCALE, go)
    for n in ("out", "dq", "dk", "dv", "delta"):
        assert (getattr(a, n)[1] == 0).all(), n
    assert (a.lse[1] == float("inf")).all() and torch.isfinite(a.lse[[0, 2]]).all()
    b = launch_any(dtype, q, k, v, mask, flag(0), SCALE, go)
    for n in NAMES:
        assert torch.equal(getattr(a, n), getattr(b, n)), n
    for i in range(nb):  # (sequence 1 alone: the neighbours' rows do not depend on it, nor it on them)
        one = launch_any(dtype, q[i:i + 1], k[i:i + 1], v[i:i + 1], mask[i:i + 1].contiguous(), flag(0), SCALE,
                         go[i:i + 1].contiguous())
        for n in NAMES:
            assert torch.equal(getattr(a, n)[i:i + 1], getattr(one, n)), (n, i)


# ------------------------------------------------------------------------------------------------------------ 8. shard origin
@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
def test_a_shard_draws_the_masks_of_its_global_samples(dtype):
    from bayeformers_amd import ops

    T, p = 100, 0.2
    q, k, v, go = inputs(dtype, T, seed=41, nb=4)
    whole, shard = ops.Dropout(p, SEED, 7, 3), ops.Dropout(p, SEED, 7, 3, origin=(1, 1))
    o_full, l_full, keep_full = ops.attention_forward_any(q, k, v, None, SCALE, None, want_lse=True, drop=whole, want_keep=True)
    o_half, l_half, keep_half = ops.attention_forward_any(q[2:], k[2:], v[2:], None, SCALE, None, want_lse=True, drop=shard,
                                                          want_keep=True)
    assert keep_full.shape == (4, H, T, 4)
    assert torch.equal(o_full[2:], o_half) and torch.equal(keep_full[2:], keep_half) and not torch.equal(o_full[:2], o_half)
    g_full = ops.attention_backward_any(q, k, v, None, None, o_full, go, l_full, SCALE, p, keep_full)
    g_half = ops.attention_backward_any(q[2:], k[2:], v[2:], None, None, o_half, go[2:].contiguous(), l_half, SCALE, p, keep_half)
    for x, y in zip(g_full, g_half):
        assert torch.equal(x[2:], y)


# ------------------------------------------------------------------------------------------------------------ 9. model level
def _tiny_bert(pooled=True):
    from transformers import BertConfig, BertForSequenceClassification

    cfg = BertConfig(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, vocab_size=100,
                     max_position_embeddings=128)
    torch.manual_seed(0)
    model = bf.to_bayesian(BertForSequenceClassification(cfg).eval(), delta=0.05, freeze=True).eval().cuda()
    bf.fuse_activations(model), bf.fuse_residual_layernorm(model), bf.fuse_shared_inputs(model)
    assert bf.fuse_attention(model)
    bf.fuse_embeddings(model)
    model = model.to(torch.bfloat16)
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(0, 100, (4, 100), generator=g).cuda()
    pad = torch.ones(4, 100, dtype=torch.long, device="cuda")
    pad[1, 70:] = 0
    pad[3, 33:] = 0
    return model, {"input_ids": ids, "attention_mask": pad}


def _delta(before):
    from bayeformers_amd import ops

    return {n: ops.ENCODER_ANY_CALLS[n] - before[n] for n in before}


def test_model_route_in_eval_counts_the_layers_and_keeps_the_logits():
    from bayeformers_amd import ops
    from bayeformers_amd.sampling import sample_bayesian

    model, batch = _tiny_bert()
    bf.set_compute_dtype("bf16")

    def run():
        bf.manual_seed(SEED)
        with torch.no_grad():
            return sample_bayesian(model, batch, 2)[0][0].float()

    try:
        run()  # (the head's layers settle on their kernels in a first forward)
        bf.pooled_last_layer(False)
        before = dict(ops.ENCODER_ANY_CALLS)
        off = run()
        assert _delta(before) == {"fwd": 0, "bwd": 0, "rows": 0}  # off by default: the framework's attention
        bf.encoder_ragged_attention()
        on = run()
        assert _delta(before) == {"fwd": 2, "bwd": 0, "rows": 0}, _delta(before)  # both layers
        err = (on - off).abs().max().item()
        print(f"[enc-any] tiny BERT T=100, kernels vs the framework's attention: max |logit difference| = {err:.3e}")
        assert err < 2e-2  # tests/test_gpu_models.py, test_fused_attention_in_bert_matches_framework_attention
        bf.pooled_last_layer(True)
        before = dict(ops.ENCODER_ANY_CALLS)
        narrow = run()
        assert _delta(before) == {"fwd": 1, "bwd": 0, "rows": 1}, _delta(before)  # the last layer: the [CLS] rows alone
        assert (narrow - off).abs().max().item() < 2e-2
    finally:
        bf.encoder_ragged_attention(False)
        bf.pooled_last_layer(True)


def test_model_route_in_training_repeats_its_masks_and_differentiates():
    from bayeformers_amd import ops
    from bayeformers_amd.sampling import sample_bayesian

    model, batch = _tiny_bert()
    model.train()
    bf.set_compute_dtype("bf16")
    dropped = []
    orig = ops.AttentionAnyFn.forward

    def count(ctx, *a):
        dropped.append(a[6] is not None and a[6].p > 0)
        return orig(ctx, *a)

    def run():
        bf.manual_seed(SEED)
        torch.manual_seed(1)  # the embedding block's dropout is the framework's
        return sample_bayesian(model, batch, 3)[1][0]

    ops.AttentionAnyFn.forward = staticmethod(count)
    try:
        bf.encoder_ragged_attention()
        before = dict(ops.ENCODER_ANY_CALLS)
        a = run()
        assert dropped == [True, True] and _delta(before) == {"fwd": 2, "bwd": 0, "rows": 0}  # the dropout entry, both layers
        b = run()
        assert torch.equal(a, b)
        c = sample_bayesian(model, batch, 3)[1][0]  # the next sample indices and the next dropout call
        assert not torch.equal(a, c)
        before = dict(ops.ENCODER_ANY_CALLS)
        a.float().sum().backward()
        assert _delta(before)["bwd"] == 2
        grads = [p.grad for p in model.parameters() if p.requires_grad and p.grad is not None]
        assert grads and all(torch.isfinite(g).all() for g in grads)
    finally:
        ops.AttentionAnyFn.forward = orig
        bf.encoder_ragged_attention(False)


def test_graphed_sampler_replays_the_eager_bits():
    from bayeformers_amd import ops
    from bayeformers_amd.sampling import GraphedSampler, sample_bayesian

    model, batch = _tiny_bert()
    bf.set_compute_dtype("bf16")
    sampler = None
    try:
        bf.encoder_ragged_attention()
        with torch.no_grad():
            sample_bayesian(model, batch, 2)
        bf.manual_seed(SEED)
        before = dict(ops.ENCODER_ANY_CALLS)
        with torch.no_grad():
            eager = [sample_bayesian(model, batch, 2)[0][0].clone() for _ in range(3)]
        assert _delta(before) == {"fwd": 3, "bwd": 0, "rows": 3}
        sampler = GraphedSampler(model, batch, 2)
        bf.manual_seed(SEED)
        for want in eager:
            assert torch.equal(sampler()[0][0], want)
    finally:
        if sampler is not None:
            sampler.close()
        bf.encoder_ragged_attention(False)
