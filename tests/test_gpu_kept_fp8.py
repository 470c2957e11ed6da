"""pinned_samples(keep_weights="fp8"): the centred FP8 row kernels (bf_fp8_rows_quantize / _dequantize, bf_gemm_nt_skinny_fp8)
against tests/fp8_rows_ref.py and float64, and the block and generation on them."""
import numpy as np
import pytest
import torch

from bayeformers_amd import _C, ops
from fp8_rows_ref import dequantize_rows, quantize_rows

pytestmark = pytest.mark.gpu

SEED = 0x5EED


# ---------------------------------------------------------------------------------------------------- quantise, dequantise
def _rows(S, N, K, seed):
    """Draws and their centre with the rows the format can go wrong on: w == centre, an amax of exactly 448 * 2^j,
    deviations from 1 down to 2^-20 of the row's largest (past 2^-12: fp8 subnormals and zeros), -0 on a +0 centre."""
    g = torch.Generator().manual_seed(seed)
    mu = torch.randn(N, K, generator=g) * 0.05
    c = mu.to(torch.bfloat16)
    w = (mu[None] + 0.05 * mu.abs()[None] * torch.randn(S, N, K, generator=g)).to(torch.bfloat16)
    w[0, 0] = c[0]                                              # an all-zero deviation row
    c[1 % N] = 0.0
    spread = 2.0 ** -torch.randint(0, 21, (K,), generator=g).float() * torch.randn(K, generator=g).sign()
    # 0.4375 = 448 * 2^-10 exactly: amax = 448 * 2^j, and 448 * 2^-15 .. 2^-20 are e4m3 subnormals and zeros
    w[0, 1 % N] = (spread * 0.4375).to(torch.bfloat16)
    w[0, 1 % N, 0], w[0, 1 % N, 1] = 0.4375, -0.0
    if S > 1:
        w[1, 1 % N] = (spread * 0.4375 * torch.rand(K, generator=g)).to(torch.bfloat16)  # the same spread, dense mantissas
        w[1, 1 % N, 0] = 0.45                                    # just above 448 * 2^-10: the next exponent
    return w, c


@pytest.mark.parametrize("S,N,K", [(3, 37, 96), (1, 16, 32), (2, 5, 4128), (2, 3, 8200), (2, 9, 44)])
def test_quantize_and_dequantize_are_bitwise_the_reference(S, N, K):
    """The issue's shapes, a row longer than a workgroup holds in registers (8200) and one that is no multiple of 8 (44: the
    element-wise path)."""
    w, c = _rows(S, N, K, seed=S * 1000 + K)
    q_ref, scale_ref = quantize_rows(w, c)
    w_ref = dequantize_rows(q_ref, scale_ref, c)
    assert bool((q_ref == 0).any()) and bool(((q_ref & 0x78) == 0).any())  # zeros and subnormals occur
    q, scale = ops.quantize_rows_fp8(w.cuda(), c.cuda())
    assert torch.equal(scale.cpu(), scale_ref)
    assert torch.equal(q.cpu(), q_ref), int((q.cpu() != q_ref).sum())
    assert torch.equal(ops.dequantize_rows_fp8(q, scale, c.cuda()).cpu().view(torch.int16), w_ref.view(torch.int16))


def test_every_fp8_byte_dequantises_as_the_reference():
    """All 254 finite e4m3fn bytes (0x7F / 0xFF are NaN: never written) on centres of both signs and several scales."""
    codes = torch.tensor([b for b in range(256) if b & 0x7F != 0x7F], dtype=torch.uint8)
    K = 256
    q = torch.zeros(3, 4, K, dtype=torch.uint8)
    q[..., :codes.numel()] = codes
    scale = torch.tensor([[1.0, 2.0 ** -20, 2.0 ** 7, 2.0 ** -64]]).repeat(3, 1).contiguous()
    c = torch.tensor([0.0, 0.37, -1e-3, 3.0], dtype=torch.bfloat16)[:, None].repeat(1, K).contiguous()
    ref = dequantize_rows(q, scale, c)
    got = ops.dequantize_rows_fp8(q.cuda(), scale.cuda(), c.cuda()).cpu()
    assert torch.equal(got.view(torch.int16), ref.view(torch.int16))


def test_rows_entries_refuse_other_dtypes():
    w = torch.zeros(2, 16, 32, dtype=torch.float16, device="cuda")
    c = torch.zeros(16, 32, dtype=torch.float16, device="cuda")
    with pytest.raises(_C.BayeFormersAMDError, match="fp16"):
        ops.quantize_rows_fp8(w, c)


# ---------------------------------------------------------------------------------------------------- the skinny GEMM
def _gelu64(v):
    return 0.5 * v * (1.0 + torch.erf(v / np.sqrt(2.0)))


_OPERANDS = {}


def _operands(N, K):
    """(q, scale, c, W^ float64, x buffer, bias) on the device for S = 4, quantised by the reference; computed once per shape."""
    if (N, K) not in _OPERANDS:
        g = torch.Generator().manual_seed(N * 7919 + K)
        S, Mmax = 4, 64
        mu = torch.randn(N, K, generator=g)
        c = mu.to(torch.bfloat16)
        w = (mu[None] + 0.05 * mu.abs()[None] * torch.randn(S, N, K, generator=g)).to(torch.bfloat16)
        q, scale = quantize_rows(w, c)
        w_hat = dequantize_rows(q, scale, c)
        # rows of x live in a [S, Mmax + 3, K] buffer: the sample stride is larger than M * K
        xbuf = torch.randn(S, Mmax + 3, K, generator=g).to(torch.bfloat16)
        bias = torch.randn(S, N, generator=g)
        _OPERANDS[(N, K)] = tuple(t.cuda() for t in (q, scale, c, w_hat.double(), xbuf, bias))
    return _OPERANDS[(N, K)]


def _skinny(x, q, scale, c, b, S, N, K, act, stride=None):
    return ops.skinny_linear_forward_fp8(x, q, scale, c, b, S, N, K, act, x_sample_stride=stride)


# (200, 4128) is split over K, unevenly; (100, 96) ends on an odd 32-deep slice
@pytest.mark.parametrize("N,K", [(16, 32), (100, 64), (100, 96), (1024, 1024), (200, 4128)])
def test_skinny_fp8_against_float64(N, K):
    q, scale, c, w64, xbuf, bias = _operands(N, K)
    Mmax = 64
    tol = 2.0 ** -8  # test_skinny_against_float64's, relative to max |ref|: the arithmetic is the same
    for S in (1, 4):
        for i, M in enumerate((1, 4, 16, 17, 64)):
            x = xbuf[:S, :M]
            ref = torch.einsum("smk,snk->smn", x.double(), w64[:S])
            for with_bias, act in ((True, 0), (False, 1)) if i % 2 == 0 else ((False, 0), (True, 1)):
                r = ref + bias[:S, None, :].double() if with_bias else ref
                r = _gelu64(r) if act else r
                b = bias[:S].contiguous() if with_bias else None
                y = _skinny(x, q[:S], scale[:S], c, b, S, N, K, act, stride=(Mmax + 3) * K).view(S, M, N)
                err = (y.double() - r).abs().max().item()
                assert err <= tol * r.abs().max().item() + 1e-5 * np.sqrt(K), (S, M, with_bias, act, err)
            # contiguous x (sample stride M * K) and a second call: bitwise equal
            xc = x.contiguous().view(S * M, K)
            y1 = _skinny(xc, q[:S], scale[:S], c, bias[:S].contiguous(), S, N, K, 0)
            y2 = _skinny(xc, q[:S], scale[:S], c, bias[:S].contiguous(), S, N, K, 0)
            assert torch.equal(y1, y2)


@pytest.mark.parametrize("N,K", [(100, 96), (200, 4128)])
def test_skinny_fp8_multiplies_by_the_dequantise_kernels_weights(N, K):
    """W^ formed in registers is W^ as bf_fp8_rows_dequantize writes it: x = one-hot rows read single weights out."""
    q, scale, c, w64, _, _ = _operands(N, K)
    S, M = 4, 16
    w_hat = ops.dequantize_rows_fp8(q, scale, c)
    assert torch.equal(w_hat.double(), w64)
    for k0 in (0, K - M):
        x = torch.zeros(S, M, K, dtype=torch.bfloat16, device="cuda")
        for m in range(M):
            x[:, m, k0 + m] = 1.0
        y = _skinny(x.view(S * M, K), q, scale, c, None, S, N, K, 0).view(S, M, N)
        assert torch.equal(y, w_hat[:, :, k0:k0 + M].transpose(1, 2))


@pytest.mark.parametrize("S,M,N,K", [(4, 4, 1024, 1024), (4, 4, 200, 4128)])
def test_skinny_fp8_graph_replay_is_bitwise_eager(S, M, N, K):
    q, scale, c, _, xbuf, b = _operands(N, K)
    x = xbuf[:S, :M].contiguous().view(S * M, K)
    eager = _skinny(x, q, scale, c, b, S, N, K, 1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _skinny(x, q, scale, c, b, S, N, K, 1)  # this stream's workspace exists before capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = _skinny(x, q, scale, c, b, S, N, K, 1)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_skinny_fp8_refuses_bad_arguments():
    dev = "cuda"
    q = torch.zeros(2, 64, 48, dtype=torch.uint8, device=dev)
    scale = torch.ones(2, 64, device=dev)
    c = torch.zeros(64, 48, dtype=torch.bfloat16, device=dev)
    x = torch.zeros(2, 48, dtype=torch.bfloat16, device=dev)
    with pytest.raises(_C.BayeFormersAMDError, match="K % 32"):
        _skinny(x, q, scale, c, None, 2, 64, 48, 0)
    q = torch.zeros(2, 64, 64, dtype=torch.uint8, device=dev)
    c = torch.zeros(64, 64, dtype=torch.bfloat16, device=dev)
    x = torch.zeros(2 * 65, 64, dtype=torch.bfloat16, device=dev)
    with pytest.raises(_C.BayeFormersAMDError, match="M <= 64"):
        _skinny(x, q, scale, c, None, 2, 64, 64, 0)
    with pytest.raises(_C.BayeFormersAMDError, match="bf16"):
        _skinny(x[:2].half(), q, scale, c, None, 2, 64, 64, 0)
    assert not ops.skinny_fp8_supported(x, q, c, 2, 64) and not ops.skinny_fp8_supported(x[:2].half(), q, c, 2, 64)
    assert ops.skinny_fp8_supported(x[:2 * ops.SKINNY_ROWS], q, c, 2, 64)


# ---------------------------------------------------------------------------------------------------- the block
def _llama(heads=8, kv_heads=2, layers=2, hidden=512, vocab=512):
    from transformers import LlamaConfig, LlamaForCausalLM

    import bayeformers_amd as bf

    cfg = LlamaConfig(hidden_size=hidden, num_attention_heads=heads, num_key_value_heads=kv_heads, num_hidden_layers=layers,
                      intermediate_size=2 * hidden, vocab_size=vocab, max_position_embeddings=512, tie_word_embeddings=False,
                      attention_dropout=0.0, attn_implementation="sdpa")
    torch.manual_seed(0)
    bmodel = bf.to_bayesian(LlamaForCausalLM(cfg).eval(), delta=0.05, freeze=True).eval().cuda()
    freqs = {n: b.detach().clone() for n, b in bmodel.named_buffers() if "inv_freq" in n}
    bmodel = bmodel.to(torch.bfloat16)
    for n, b in freqs.items():
        setattr(bmodel.get_submodule(n.rsplit(".", 1)[0]), n.rsplit(".", 1)[1], b)
    assert bf.fuse_attention(bmodel)
    bf.set_compute_dtype("bf16")
    return bmodel


def _prompt(B=2, T=128, vocab=512):
    g = torch.Generator().manual_seed(11)
    return torch.randint(0, vocab, (B, T), generator=g).cuda()


def _count_launches(monkeypatch):
    lib = _C.lib()
    counts = {"bf_sample_logprob_table": 0, "bf_linear_fwd": 0, "bf_sample_logprob": 0, "bf_gemm_nt_skinny": 0}
    for name in counts:
        real = getattr(lib, name)

        def wrapper(*a, _real=real, _name=name):
            counts[_name] += 1
            return _real(*a)

        monkeypatch.setattr(lib, name, wrapper)
    return counts


def test_fp8_store_is_the_reference_quantisation_of_the_kept_draws():
    import bayeformers_amd as bf
    from bayeformers_amd.nn.layers.linear import Linear
    from bayeformers_amd.plan import kept_weight_bytes

    bmodel = _llama()
    ids = _prompt(T=32)
    S = 3
    linears = [l for l in bmodel.fused_children() if isinstance(l, Linear)]
    picked = (linears[0], linears[5], linears[-1])
    bf.manual_seed(SEED)
    with torch.no_grad(), bmodel.monte_carlo(S), bmodel.pinned_samples(keep_weights=True):
        bmodel(input_ids=ids.repeat(S, 1), use_cache=False)
        lp_ref = bmodel.log_prob_samples().clone()
        draws = [bmodel._kept.plan.views[id(l)][0].cpu() for l in picked]
    bf.manual_seed(SEED)
    with torch.no_grad(), bmodel.monte_carlo(S), bmodel.pinned_samples(keep_weights="fp8"):
        bmodel(input_ids=ids.repeat(S, 1), use_cache=False)
        lp = bmodel.log_prob_samples().clone()
        kept = bmodel._kept
        assert len(kept.store) == len(linears)
        for layer, w16 in zip(picked, draws):
            center, q, scale, bias = kept.store[id(layer)]
            c_ref = layer.weight.mu.detach().cpu().to(torch.bfloat16)
            q_ref, scale_ref = quantize_rows(w16, c_ref)
            assert torch.equal(center.cpu().view(torch.int16), c_ref.view(torch.int16)) and bias is None
            assert torch.equal(q.cpu(), q_ref) and torch.equal(scale.cpu(), scale_ref)
        assert kept.store_bytes() == kept_weight_bytes(bmodel, S, torch.bfloat16, fp8=True)
        assert kept.store_bytes() < 0.84 * kept_weight_bytes(bmodel, S, torch.bfloat16)  # (2 + S) / 2S = 0.833 at S = 3
        bmodel(input_ids=ids.repeat(S, 1), use_cache=False)
        assert torch.equal(bmodel.log_prob_samples(), lp)
    assert torch.equal(lp, lp_ref)
    assert bmodel.__dict__.get("_kept") is None


def _last_logits_both_ways(bmodel, ids, S, keep):
    """Last-position logits of a forward over all T tokens (tiled GEMMs) and of a forward over T - 1 tokens plus one cached
    decode step (skinny GEMMs), inside one block."""
    import bayeformers_amd as bf
    from transformers import DynamicCache

    bf.manual_seed(SEED)
    rep = ids.repeat(S, 1)
    with torch.no_grad(), bmodel.monte_carlo(S), bmodel.pinned_samples(keep_weights=keep):
        full = bmodel(input_ids=rep, use_cache=False).logits[:, -1].float()
        cache = DynamicCache(config=bmodel.model.config)
        bmodel(input_ids=rep[:, :-1], past_key_values=cache, use_cache=True)
        k0 = (ops.SKINNY_FP8_CALLS if keep == "fp8" else ops.SKINNY_CALLS)[0]
        step = bmodel(input_ids=rep[:, -1:], past_key_values=cache, use_cache=True).logits[:, -1].float()
        assert (ops.SKINNY_FP8_CALLS if keep == "fp8" else ops.SKINNY_CALLS)[0] - k0 == 15
    return full, step


def test_prefill_and_decode_multiply_by_the_same_weights():
    """fp8: |full - (prefill + decode step)| at most 2x what keep_weights=True shows between the same two paths — there the
    weights are identical bits and only the kernels' summation orders differ.  Measured on an MI355X: 0.0098 for
    keep_weights=True, 0.0039 for fp8 (max |logit difference|)."""
    bmodel = _llama()
    ids = _prompt(T=33)
    S = 3
    full16, step16 = _last_logits_both_ways(bmodel, ids, S, True)
    full8, step8 = _last_logits_both_ways(bmodel, ids, S, "fp8")
    d16 = (full16 - step16).abs().max().item()
    d8 = (full8 - step8).abs().max().item()
    print(f"prefill vs decode, max |logit difference|: keep_weights=True {d16:.6g}, fp8 {d8:.6g}; "
          f"fp8 vs True on the full forward {(full8 - full16).abs().max().item():.6g}")
    assert d16 > 0.0
    assert d8 <= 2.0 * d16


def test_fp8_fidelity_of_the_predictive_statistics():
    """Teacher-forced, same seed: entropies and mutual information of mc_predictive within the project's bf16 bound 0.05.
    Measured on an MI355X: 0.0006 / 0.0012 / 0.0006."""
    import bayeformers_amd as bf
    from bayeformers_amd.sampling import mc_predictive

    bmodel = _llama()
    ids = _prompt(T=64)
    S, B = 4, ids.shape[0]
    preds = {}
    for keep in (True, "fp8"):
        bf.manual_seed(SEED)
        with torch.no_grad(), bmodel.monte_carlo(S), bmodel.pinned_samples(keep_weights=keep):
            logits = bmodel(input_ids=ids.repeat(S, 1), use_cache=False).logits
            preds[keep] = mc_predictive(logits.view(S, B, *logits.shape[1:]))
    for name in ("predictive_entropy", "expected_entropy", "mutual_information"):
        a, b = getattr(preds[True], name), getattr(preds["fp8"], name)
        shift = (a - b).abs().max().item()
        print(f"{name}: max |fp8 - bf16 keep| {shift:.6g} (mean {a.mean().item():.6g})")
        assert shift < 0.05  # the project's bf16 bound (test_generate_keep_weights_bf16_matches_teacher_forcing)


# ---------------------------------------------------------------------------------------------------- generation
def _gen(bmodel, ids, mask=None, **kw):
    import bayeformers_amd as bf
    from bayeformers_amd.sampling import sample_generate

    bf.manual_seed(SEED)
    with torch.no_grad():
        return sample_generate(bmodel, ids, attention_mask=mask, **kw)


def _equal(a, b):
    from dataclasses import fields

    return all(torch.equal(getattr(a, f.name), getattr(b, f.name)) for f in fields(a))


def test_generate_fp8_launches_and_log_probs(monkeypatch):
    bmodel = _llama()
    ids = _prompt()
    S, n = 3, 8
    ref = _gen(bmodel, ids, samples=S, max_new_tokens=n, keep_weights=True)
    counts = _count_launches(monkeypatch)
    k0, d0 = ops.SKINNY_FP8_CALLS[0], ops.DECODE_CALLS["fwd"]
    gen = _gen(bmodel, ids, samples=S, max_new_tokens=n, keep_weights="fp8")
    # one sampling launch for the whole generation, no per-layer forward, no bf16 skinny launch
    assert counts == {"bf_sample_logprob_table": 1, "bf_linear_fwd": 0, "bf_sample_logprob": 0, "bf_gemm_nt_skinny": 0}, counts
    assert ops.SKINNY_FP8_CALLS[0] - k0 == 15 * (n - 1)  # 7 Linear layers per decoder layer and the head, every decode step
    assert ops.DECODE_CALLS["fwd"] - d0 == 2 * (n - 1)
    monkeypatch.undo()
    assert torch.equal(gen.log_prior, ref.log_prior) and torch.equal(gen.log_variational_posterior, ref.log_variational_posterior)
    assert gen.sequences.shape == ref.sequences.shape and (gen.token_prob > 0).all()
    for name in ("predictive_entropy", "expected_entropy", "mutual_information"):
        same = gen.sequences[:, 128:] == ref.sequences[:, 128:]
        first = same.long().cummin(1).values.bool()  # steps before the texts part ways see the same context
        assert ((getattr(gen, name) - getattr(ref, name)).abs() * first).max().item() < 0.05


def test_generate_fp8_graph_is_bitwise_static():
    bmodel = _llama()
    ids = _prompt(T=64)
    mask = torch.ones_like(ids)
    mask[1, :9] = 0
    kw = dict(samples=3, max_new_tokens=12, keep_weights="fp8")
    _gen(bmodel, ids, mask, samples=3, max_new_tokens=2)
    static = _gen(bmodel, ids, mask, static_cache=True, **kw)
    graph = _gen(bmodel, ids, mask, graph=True, **kw)
    assert _equal(static, graph)
    assert torch.equal(graph.lengths, torch.full((2,), 12, device="cuda")) and (graph.token_prob > 0).all()


def test_generate_fp8_padding_and_eos():
    """As test_generate_keep_weights_device_counter_padding_and_eos."""
    import bayeformers_amd as bf
    from bayeformers_amd.sampling import sample_generate

    bmodel = _llama()
    ids = _prompt()
    mask = torch.ones_like(ids)
    mask[1, :7] = 0
    S, n = 2, 6
    host = _gen(bmodel, ids, mask, samples=S, max_new_tokens=n, keep_weights="fp8")
    alone = _gen(bmodel, ids[1:, 7:], samples=S, max_new_tokens=n, keep_weights="fp8")
    assert torch.equal(host.sequences[1, 128:], alone.sequences[0, 121:])
    bf.manual_seed(SEED)
    bf.use_device_counter(True)
    try:
        with torch.no_grad():
            dev = sample_generate(bmodel, ids, attention_mask=mask, samples=S, max_new_tokens=n, keep_weights="fp8")
        assert int(bf.random.STATE.device_counter.item()) == S  # committed once
    finally:
        bf.use_device_counter(False)
    assert torch.equal(host.sequences, dev.sequences) and torch.equal(host.log_prior, dev.log_prior)
    # EOS: row 0 ends at the token it emits at step 2
    eos = int(host.sequences[0, 128 + 2])
    first = (host.sequences[0, 128:] == eos).nonzero()[0].item()
    g = _gen(bmodel, ids, mask, samples=S, max_new_tokens=n, eos_token_id=eos, pad_token_id=7, keep_weights="fp8")
    assert int(g.lengths[0]) == first + 1
    assert torch.equal(g.sequences[0, 128:129 + first], host.sequences[0, 128:129 + first])
    assert (g.sequences[0, 129 + first:] == 7).all() and (g.token_prob[0, first + 1:] == 0).all()


def test_fp8_block_refusals(monkeypatch):
    import bayeformers_amd as bf
    from bayeformers_amd.plan import kept_weight_bytes

    bmodel = _llama()
    ids = _prompt(T=16)
    S = 2
    need = kept_weight_bytes(bmodel, S, torch.bfloat16, fp8=True)
    counts = _count_launches(monkeypatch)
    bf.manual_seed(SEED)
    with torch.no_grad(), bmodel.monte_carlo(S), pytest.raises(ValueError, match=str(need)):
        with bmodel.pinned_samples(keep_weights="fp8", max_bytes=need - 1):
            bmodel(input_ids=ids.repeat(S, 1), use_cache=False)
    assert sum(counts.values()) == 0 and bf.random.STATE.next_sample == 0
    # parameters are read once: an in-place edit of mu inside the block makes the next forward raise
    layer = bmodel.model.model.layers[0].mlp.up_proj
    with torch.no_grad(), bmodel.monte_carlo(S), bmodel.pinned_samples(keep_weights="fp8", max_bytes=need):
        bmodel(input_ids=ids.repeat(S, 1), use_cache=False)
        layer.weight.mu.mul_(1.0)
        with pytest.raises(RuntimeError, match="changed inside the block"):
            bmodel(input_ids=ids.repeat(S, 1), use_cache=False)
    with torch.no_grad(), bmodel.monte_carlo(S), bmodel.pinned_samples(keep_weights="fp8"):
        with torch.enable_grad(), pytest.raises(RuntimeError, match="without gradients"):
            bmodel(input_ids=ids.repeat(S, 1), use_cache=False)
