"""The FP8 KV cache on the GPU: bf_kv8_append / bf_kv8_dequantize bitwise against tests/kv8_ref.py, bf_attention_decode_gqa_kv8
bitwise against the bf16 decode kernel on the dequantised cache (and both against float64), capture, the cache layer, and
sample_generate(kv_cache="fp8") against an oracle that shares everything with it but the layer and the decode entry."""
import functools
from dataclasses import fields

import pytest
import torch

from kv8_ref import append as ref_append
from kv8_ref import decode_reference, dequantize, quantize, special_rows

pytestmark = pytest.mark.gpu

TOL = 9.1e-3  # tests/test_gpu_decode_attention.py's bf16 bound for this kernel: max |out - ref| / max |ref|
SEED = 1234


def _empty_cache(N, Hkv, cap, D, device="cuda"):
    return (torch.zeros(N, Hkv, cap, D, dtype=torch.uint8, device=device), torch.zeros(N, Hkv, cap, D, dtype=torch.uint8, device=device),
            torch.zeros(N, Hkv, cap, dtype=torch.float32, device=device), torch.zeros(N, Hkv, cap, dtype=torch.float32, device=device))


def _rows(layout, N, Hkv, Tq, D, gen):
    """New K / V rows [N, Hkv, Tq, D] bf16 on the CPU: contiguous, or HF's [B, T, H * D] projection viewed as [B, H, T, D]"""
    if layout == "contiguous":
        return torch.randn(N, Hkv, Tq, D, generator=gen).to(torch.bfloat16)
    return torch.randn(N, Tq, Hkv * D, generator=gen).to(torch.bfloat16).view(N, Tq, Hkv, D).transpose(1, 2)


# ---------------------------------------------------------------------------------------------------- 1. append, dequantise
@pytest.mark.parametrize("layout", ["contiguous", "hf"])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_append_is_bitwise_the_reference(D, layout):
    from bayeformers_amd import ops

    N, Hkv, cap = 3, 2, 70
    gen = torch.Generator().manual_seed(D)
    dev = _empty_cache(N, Hkv, cap, D)
    for t in dev:  # a pattern in the unwritten slots
        t.fill_(3)
    ref = tuple(t.cpu() for t in dev)
    fill = torch.zeros(1, dtype=torch.int64, device="cuda")
    c0 = ops.KV8_CALLS["append"]
    for pos, Tq in ((0, 5), (5, 1), (6, 16)):
        k, v = _rows(layout, N, Hkv, Tq, D, gen), _rows(layout, N, Hkv, Tq, D, gen)
        if Tq >= 4:  # the special rows, as K rows of one head and V rows of another
            k[1, 0, :4], v[2, 1, :4] = special_rows(D), special_rows(D)
        fill.fill_(pos)
        kd, vd = k.cuda(), v.cuda()  # (.cuda() keeps the strides of the transposed view)
        assert kd.stride() == k.stride()
        ops.kv8_append(kd, vd, *dev, fill)
        ref_append(*ref, k, v, pos)
    assert ops.KV8_CALLS["append"] - c0 == 3
    for name, got, want in zip(("kq", "vq", "k_scale", "v_scale"), dev, ref):
        assert torch.equal(got.cpu(), want), name  # the written slots and the untouched ones (22 .. 69 still hold the pattern)
    assert bool((dev[0][:, :, 22:] == 3).all()) and bool((dev[3][:, :, 22:] == 3.0).all())
    back = ops.kv8_dequantize(dev[0][:, :, :22].contiguous(), dev[2][:, :, :22].contiguous())
    assert back.dtype == torch.bfloat16 and torch.equal(back.cpu(), dequantize(ref[0][:, :, :22], ref[2][:, :, :22]))


def test_dequantize_of_every_byte_at_three_scales():
    from bayeformers_amd import ops

    finite = [b for b in range(256) if b & 0x7F != 0x7F]  # (0x7f / 0xff are e4m3fn's NaN: inputs are finite)
    row = torch.tensor(finite + [0] * (256 - len(finite)), dtype=torch.uint8)
    q = row[None].repeat(3, 1)
    scale = torch.tensor([1.0, 2.0 ** -13, 2.0 ** 40])
    c0 = ops.KV8_CALLS["dequantize"]
    got = ops.kv8_dequantize(q.cuda(), scale.cuda())
    assert ops.KV8_CALLS["dequantize"] - c0 == 1
    want = dequantize(q, scale)
    assert torch.equal(got.cpu(), want)
    assert bool((got.cpu().view(torch.int16)[:, finite.index(0x80)] == -0x8000).all())  # the byte -0 stays -0
    assert torch.equal(want.float(), q.view(torch.float8_e4m3fn).float() * scale[:, None])


@pytest.mark.parametrize("D", [64, 256])
def test_append_at_the_boundary_writes_inside_the_cache_only(D):
    """Fill capacity - 2 with four new rows writes two; a negative fill writes the rows that land at slots >= 0.  The cache
    tensors are views inside larger tensors full of a sentinel, all of which must survive."""
    from bayeformers_amd import ops

    N, Hkv, cap, Tq = 3, 2, 10, 4
    gen = torch.Generator().manual_seed(D + 1)
    rows, guard = N * Hkv * cap, 4096
    big_q = torch.full((2, guard + rows * D + guard), 0xA5, dtype=torch.uint8, device="cuda")
    big_s = torch.full((2, guard + rows + guard), -7.0, dtype=torch.float32, device="cuda")
    kq, vq = (big_q[i, guard:guard + rows * D].view(N, Hkv, cap, D) for i in range(2))
    ks, vs = (big_s[i, guard:guard + rows].view(N, Hkv, cap) for i in range(2))
    assert kq.data_ptr() % 16 == 0 and vq.data_ptr() % 16 == 0
    ref = tuple(t.cpu().clone() for t in (kq, vq, ks, vs))
    fill = torch.zeros(1, dtype=torch.int64, device="cuda")
    for pos in (cap - 2, -3, cap, -Tq, 2 ** 40, -2 ** 40):
        k, v = _rows("hf", N, Hkv, Tq, D, gen), _rows("hf", N, Hkv, Tq, D, gen)
        fill.fill_(pos)
        ops.kv8_append(k.cuda(), v.cuda(), kq, vq, ks, vs, fill)
        ref_append(*ref, k, v, pos)
    torch.cuda.synchronize()
    for got, want in zip((kq, vq, ks, vs), ref):
        assert torch.equal(got.cpu(), want)
    assert bool((ref[0][:, :, 1:cap - 2] == 0xA5).all())  # slots 1 .. capacity - 3 were never written
    for big, sentinel in ((big_q, 0xA5), (big_s, -7.0)):
        assert bool((big[:, :guard] == sentinel).all()) and bool((big[:, -guard:] == sentinel).all())


# ---------------------------------------------------------------------------------------------------- 2. decode
CAP = 320


@functools.lru_cache(maxsize=None)
def _cache(D, Hkv, N=3):
    """A full FP8 cache of CAP slots (quantised by the reference) and its dequantised bf16 twin, on the device"""
    gen = torch.Generator().manual_seed(100 * D + Hkv)
    out = []
    for _ in range(2):
        q, s = quantize(torch.randn(N, Hkv, CAP, D, generator=gen).to(torch.bfloat16))
        out += [q.cuda(), s.cuda(), dequantize(q, s).cuda()]
    kq, ks, k16, vq, vs, v16 = out
    return kq, vq, ks, vs, k16, v16


def _key_mask(kind, N, cap):
    if kind == "none":
        return None
    m = torch.zeros(N, cap, device="cuda")
    for n in range(N):  # left padding of different lengths
        m[n, : 5 * n] = float("-inf")
    if kind == "hidden_row":
        m[N - 1] = float("-inf")
    return m


@pytest.mark.parametrize("Tq", [1, 3, 16])
@pytest.mark.parametrize("H,Hkv", [(4, 2), (8, 1), (4, 4)])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_decode_is_bitwise_the_bf16_kernel_on_the_dequantised_cache(D, H, Hkv, Tq):
    from bayeformers_amd import ops

    N, scale = 3, D ** -0.5
    kq, vq, ks, vs, k16, v16 = _cache(D, Hkv)
    gen = torch.Generator().manual_seed(1000 * Tq + 10 * H + D)
    q = torch.randn(N, Tq, H, D, generator=gen).to(torch.bfloat16).cuda().transpose(1, 2)  # HF's layout
    assert ops.attention_decode_kv8_supported(q, kq, vq)
    d0, s0, k0 = dict(ops.DECODE_CALLS), dict(ops.SOFTCAP_CALLS), ops.KV8_CALLS["decode"]
    calls, worst = 0, 0.0
    for L in sorted({Tq, 63, 64, 65, 129, 300, CAP}):  # 129 and up: 2 .. 3 key splits; 64 +- 1: the tile edges
        kv_len = torch.tensor([L], dtype=torch.int64, device="cuda")
        for kind in ("none", "padded", "hidden_row"):
            m = _key_mask(kind, N, CAP)
            for window in (None, 50):
                for softcap in (None, 30.0):
                    d1, s1 = dict(ops.DECODE_CALLS), dict(ops.SOFTCAP_CALLS)
                    out = ops.attention_forward_decode_kv8(q, kq, vq, ks, vs, kv_len, m, scale, window=window, softcap=softcap)
                    assert ops.DECODE_CALLS == d1 and ops.SOFTCAP_CALLS == s1  # the kv8 entry counts on KV8_CALLS alone
                    calls += 1
                    want = ops.attention_forward_decode_len(q, k16, v16, kv_len, m, scale, window=window, softcap=softcap)
                    assert out.shape == (N, Tq, H, D) and out.is_contiguous() and out.dtype == torch.bfloat16
                    assert torch.equal(out, want), (L, kind, window, softcap)
                    if L == CAP:  # the fill at the capacity is the call without a fill
                        no_len = ops.attention_forward_decode_kv8(q, kq, vq, ks, vs, None, m, scale, window=window, softcap=softcap)
                        calls += 1
                        assert torch.equal(no_len, ops.attention_forward_decode(q, k16, v16, m, scale, window=window, softcap=softcap))
                        assert torch.equal(no_len, out)
                    if kind == "hidden_row":
                        assert torch.equal(out[N - 1], torch.zeros_like(out[N - 1]))  # no visible key: exactly 0
                    ref = decode_reference(q, k16, v16, scale, kv_len=L, key_mask=m, window=window, softcap=softcap)
                    err = (out.double() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)
                    worst = max(worst, err)
                    assert err < TOL, (L, kind, window, softcap, err)
    assert ops.KV8_CALLS["decode"] - k0 == calls
    print(f"[kv8 decode D={D} H={H} Hkv={Hkv} Tq={Tq}] max |out - float64| / max |float64| = {worst:.3e}")


def test_decode_wrapper_refusals():
    from bayeformers_amd import _C, ops

    kq, vq, ks, vs, k16, _ = _cache(64, 2)
    q = torch.zeros(3, 4, 1, 64, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(_C.BayeFormersAMDError, match="bfloat16"):
        ops.attention_forward_decode_kv8(q.half(), kq, vq, ks, vs, None, None, 0.125)
    with pytest.raises(_C.BayeFormersAMDError, match="uint8"):
        ops.attention_forward_decode_kv8(q, k16, k16, ks, vs, None, None, 0.125)
    with pytest.raises(_C.BayeFormersAMDError, match="k_scale"):
        ops.attention_forward_decode_kv8(q, kq, vq, ks[:, :, :5], vs, None, None, 0.125)
    with pytest.raises(_C.BayeFormersAMDError, match="Tq=17"):
        ops.attention_forward_decode_kv8(torch.zeros(3, 4, 17, 64, dtype=torch.bfloat16, device="cuda"), kq, vq, ks, vs, None,
                                         None, 0.125)
    with pytest.raises(_C.BayeFormersAMDError, match="bfloat16"):
        ops.kv8_append(k16.half()[:, :, :1], k16.half()[:, :, :1], kq, vq, ks, vs, torch.zeros(1, dtype=torch.int64, device="cuda"))


# ---------------------------------------------------------------------------------------------------- 3. capture
def test_captured_append_and_decode_replay_while_the_fill_advances():
    from bayeformers_amd import ops

    N, H, Hkv, D, cap, fill0, steps = 8, 32, 8, 128, 400, 100, 5
    gen = torch.Generator().manual_seed(9)
    start = _empty_cache(N, Hkv, cap, D, device="cpu")
    ref_append(*start, torch.randn(N, Hkv, fill0, D, generator=gen).to(torch.bfloat16),
               torch.randn(N, Hkv, fill0, D, generator=gen).to(torch.bfloat16), 0)
    qs = [torch.randn(N, 1, H, D, generator=gen).to(torch.bfloat16).cuda().transpose(1, 2) for _ in range(steps)]
    kvs = [(_rows("hf", N, Hkv, 1, D, gen).cuda(), _rows("hf", N, Hkv, 1, D, gen).cuda()) for _ in range(steps)]
    mask = _key_mask("padded", N, cap)

    def step(q, k, v, cache, fill):
        ops.kv8_append(k, v, *cache, fill)
        fill.add_(1)
        return ops.attention_forward_decode_kv8(q, cache[0], cache[1], cache[2], cache[3], fill, mask, 0.125)

    eager = tuple(t.cuda() for t in start)
    fill = torch.tensor([fill0], dtype=torch.int64, device="cuda")
    want = [step(q, k, v, eager, fill) for q, (k, v) in zip(qs, kvs)]

    replayed = tuple(t.cuda() for t in start)
    fill_g = torch.tensor([fill0], dtype=torch.int64, device="cuda")
    q_in, k_in, v_in = torch.empty_like(qs[0]), torch.empty_like(kvs[0][0]), torch.empty_like(kvs[0][1])
    assert q_in.stride() == qs[0].stride() and k_in.stride() == kvs[0][0].stride()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up off the capture, on a cache of its own
        step(qs[0], *kvs[0], tuple(t.cuda() for t in start), torch.tensor([fill0], dtype=torch.int64, device="cuda"))
    torch.cuda.current_stream().wait_stream(s)
    q_in.copy_(qs[0]), k_in.copy_(kvs[0][0]), v_in.copy_(kvs[0][1])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = step(q_in, k_in, v_in, replayed, fill_g)
    fill_g.fill_(fill0)  # (capture ran nothing: the cache and the fill are as they were)
    got = []
    for q, (k, v) in zip(qs, kvs):
        q_in.copy_(q), k_in.copy_(k), v_in.copy_(v)
        g.replay()
        got.append(out.clone())
    torch.cuda.synchronize()
    assert int(fill_g) == int(fill) == fill0 + steps
    for t, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), t
    for a, b in zip(replayed, eager):
        assert torch.equal(a, b)
    assert not torch.equal(eager[0].cpu(), start[0])  # (the steps did write)


# ---------------------------------------------------------------------------------------------------- models
def _tiny_llama():
    from test_gpu_decode_attention import _tiny_llama as build

    import bayeformers_amd as bf

    bf.set_compute_dtype("bf16")
    model = build()  # 8 heads, 2 K/V heads, head size 64, 2 layers
    assert bf.fuse_attention(model)
    return model


def _tiny_mistral(window=4):
    from transformers import AutoConfig, AutoModelForCausalLM

    import bayeformers_amd as bf

    bf.set_compute_dtype("bf16")
    cfg = AutoConfig.for_model("mistral", hidden_size=256, num_attention_heads=4, num_key_value_heads=2, head_dim=64,
                               num_hidden_layers=2, intermediate_size=512, vocab_size=512, max_position_embeddings=1024,
                               tie_word_embeddings=False, attention_dropout=0.0, attn_implementation="sdpa",
                               sliding_window=window)
    torch.manual_seed(0)
    bmodel = bf.to_bayesian(AutoModelForCausalLM.from_config(cfg).eval(), delta=0.05, freeze=True).eval().cuda()
    freqs = {n: b.detach().clone() for n, b in bmodel.named_buffers() if "inv_freq" in n}
    bmodel = bmodel.to(torch.bfloat16)
    for n, b in freqs.items():
        setattr(bmodel.get_submodule(n.rsplit(".", 1)[0]), n.rsplit(".", 1)[1], b)
    assert bf.fuse_attention(bmodel)
    return bmodel


def _tiny_gemma2():
    from test_gpu_softcap_attention import _gemma2

    import bayeformers_amd as bf

    bf.set_compute_dtype("bf16")
    return _gemma2(torch.bfloat16, True)  # head size 256, sliding W = 100 then full, attn_logit_softcapping 1.0


def _oracle_layer():
    """A bf16 StaticLayer that stores what the FP8 layer would give back: kv8_dequantize(kv8_append(...))"""
    from transformers.cache_utils import StaticLayer

    from bayeformers_amd import ops

    class OracleLayer(StaticLayer):
        def update(self, key_states, value_states, *args, **kwargs):
            if not self.is_initialized:
                self.lazy_initialization(key_states, value_states)
                self.rows = _empty_cache(*self.keys.shape, device=self.keys.device)
            ops.kv8_append(key_states, value_states, *self.rows, self.cumulative_length)
            self.cumulative_length.add_(key_states.shape[-2])
            ops.kv8_dequantize(self.rows[0], self.rows[2], out=self.keys)
            ops.kv8_dequantize(self.rows[1], self.rows[3], out=self.values)
            return self.keys, self.values

    return OracleLayer


def _prompt(B=2, T=8, pad=3, vocab=512):
    ids = torch.randint(0, vocab, (B, T), generator=torch.Generator().manual_seed(11)).cuda()
    mask = torch.ones_like(ids)
    mask[B - 1, :pad] = 0  # one left-padded row
    return ids, mask


def _generate(model, ids, mask, n=6, sample=False, **kw):
    import bayeformers_amd as bf
    from bayeformers_amd.sampling import sample_generate

    bf.manual_seed(SEED)
    if sample:
        kw.update(do_sample=True, top_k=5, generator=torch.Generator(device="cuda").manual_seed(5))
    with torch.no_grad():
        return sample_generate(model, ids, attention_mask=mask, samples=3, max_new_tokens=n, **kw)


def _same(a, b):
    return all(torch.equal(getattr(a, f.name), getattr(b, f.name)) for f in fields(a))


# ---------------------------------------------------------------------------------------------------- 4. the layer
def test_the_fp8_layer_appends_at_its_fill_and_counts_its_bytes():
    import bayeformers_amd as bf
    from bayeformers_amd.kv_cache import Fp8StaticLayer
    from bayeformers_amd.sampling import _static_cache

    model = _tiny_llama()
    S, B, cap, Hkv, D = 3, 2, 24, 2, 64
    cache = _static_cache(model, cap, kv_cache="fp8")
    assert [type(layer) for layer in cache.layers] == [Fp8StaticLayer] * 2
    gen = torch.Generator().manual_seed(4)
    ref = [_empty_cache(S * B, Hkv, cap, D, device="cpu") for _ in cache.layers]
    fill = 0
    for Tq in (5, 1):
        for i, layer in enumerate(cache.layers):
            k, v = _rows("hf", S * B, Hkv, Tq, D, gen), _rows("hf", S * B, Hkv, Tq, D, gen)
            keys, values = cache.update(k.cuda(), v.cuda(), i)
            ref_append(*ref[i], k, v, fill)
            assert keys is layer.keys and values is layer.values and keys.dtype == torch.uint8
            assert keys._bf_kv8_scale is layer.key_scales and values._bf_kv8_scale is layer.value_scales
            assert int(layer.cumulative_length) == fill + Tq and int(layer.get_seq_length()) == fill + Tq
            assert layer.get_mask_sizes(Tq) == (cap, 0)
        fill += Tq
    for layer, want in zip(cache.layers, ref):
        for got, w in zip((layer.keys, layer.values, layer.key_scales, layer.value_scales), want):
            assert torch.equal(got.cpu(), w)
    assert sum(layer.store_bytes() for layer in cache.layers) == bf.kv_cache_bytes(model, S, B, cap, fp8=True)
    assert bf.kv_cache_bytes(model, S, B, cap, fp8=True) / bf.kv_cache_bytes(model, S, B, cap) == (2 * D + 8) / (4 * D)


# ---------------------------------------------------------------------------------------------------- 5. generation
@pytest.fixture
def softcap_switch():
    import bayeformers_amd as bf

    yield bf.softcap_attention
    bf.softcap_attention(False)


VARIANTS = {
    "plain": (_tiny_llama, {}),
    "graph": (_tiny_llama, dict(graph=True)),
    "keep_weights": (_tiny_llama, dict(keep_weights=True)),
    "keep_weights_fp8": (_tiny_llama, dict(keep_weights="fp8")),
    "top_k": (_tiny_llama, dict(sample=True)),
    "mistral_window_4": (_tiny_mistral, {}),
    "gemma2_softcap": (_tiny_gemma2, {}),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_generation_is_bitwise_the_oracle_on_a_dequantised_cache(variant, monkeypatch, softcap_switch):
    """sample_generate(kv_cache="fp8") against the same call on a bf16 static cache whose layers store
    kv8_dequantize(kv8_append(...)): the two runs share everything but the layer and the decode entry, so every field of the
    Generation is equal bit for bit."""
    from bayeformers_amd import ops, sampling

    build, kw = VARIANTS[variant]
    if variant == "gemma2_softcap":
        softcap_switch()
    model = build()
    layers, n = 2, 6
    ids, mask = _prompt()  # 8 prompt tokens: longer than Mistral's window of 4
    with monkeypatch.context() as mp:
        mp.setattr(sampling, "_STATIC_LAYER_HOOK", _oracle_layer())
        oracle = _generate(model, ids, mask, n, **{**kw, "static_cache": True})
    k0, d0, s0 = dict(ops.KV8_CALLS), dict(ops.DECODE_CALLS), dict(ops.SOFTCAP_CALLS)
    got = _generate(model, ids, mask, n, kv_cache="fp8", **kw)
    moved = {name: ops.KV8_CALLS[name] - k0[name] for name in k0}
    # the decode entries of the bf16 caches did not move (the soft-cap prefill of Gemma 2 is a forward, not a decode)
    assert ops.DECODE_CALLS == d0
    assert all(ops.SOFTCAP_CALLS[name] == s0[name] for name in ("decode", "decode_len"))
    if kw.get("graph"):  # one eager step and the captured one enqueue from Python; the replays do not
        assert moved == {"append": layers * 3, "decode": layers * 2, "dequantize": 0}, moved
        assert _same(got, _generate(model, ids, mask, n, kv_cache="fp8"))  # bitwise the eager static run
    else:
        assert moved == {"append": layers * n, "decode": layers * (n - 1), "dequantize": 0}, moved
    assert got.sequences.shape == (2, 8 + n) and bool((got.lengths == n).all())
    for f in fields(got):
        assert torch.equal(getattr(got, f.name), getattr(oracle, f.name)), (variant, f.name)


# ---------------------------------------------------------------------------------------------------- 6. fidelity
def test_fidelity_against_the_bf16_cache():
    """Greedy, 16 new tokens, the same seed: kv_cache="fp8" against static_cache=True over the steps before the first token
    on which the two texts differ (at least 4).  The statistics differ by e4m3's rounding of the cached rows.  Measured on
    the MI355X (profiles/kv_cache_fp8.md): the texts first differ at step 6 of 16, and over the steps before it the
    predictive entropy moves by at most 4.8e-4, the expected entropy by 3.7e-4, the mutual information by 1.1e-4 and
    token_prob by 1.7e-4.  That is under 0.025, so the bound asserted is the project's statistics bound 0.05
    (tests/test_gpu_kept_fp8.py)."""
    model = _tiny_llama()
    ids, mask = _prompt()
    n = 16
    ref = _generate(model, ids, mask, n, static_cache=True)
    got = _generate(model, ids, mask, n, kv_cache="fp8")
    assert bool((ref.lengths == n).all())  # no eos_token_id: the bf16 run does not end early
    differ = (ref.sequences[:, 8:] != got.sequences[:, 8:]).any(0)
    first = int(differ.nonzero()[0]) if bool(differ.any()) else n
    worst = {}
    for name in ("predictive_entropy", "expected_entropy", "mutual_information", "token_prob"):
        a, b = getattr(ref, name)[:, :max(first, 1)], getattr(got, name)[:, :max(first, 1)]
        worst[name] = (a - b).abs().max().item()
    print(f"[kv8 fidelity] first differing step {first} of {n}; max |fp8 - bf16| over the steps before it: "
          + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    assert first >= 4, first
    assert max(worst.values()) < 0.05, worst


# ---------------------------------------------------------------------------------------------------- 7. fallback
def test_a_17_token_chunk_against_an_fp8_cache_dequantises_and_matches_the_bf16_path():
    import bayeformers_amd as bf
    from bayeformers_amd import ops
    from bayeformers_amd.sampling import _static_cache
    from transformers import StaticCache

    model = _tiny_llama()
    S, B, cap = 2, 2, 64
    gen = torch.Generator().manual_seed(3)
    first = torch.randint(0, 512, (B, 8), generator=gen).cuda().repeat(S, 1)
    chunk = torch.randint(0, 512, (B, 17), generator=gen).cuda().repeat(S, 1)

    def run(cache):
        bf.manual_seed(SEED)
        with torch.no_grad(), model.monte_carlo(S), model.pinned_samples():
            model(input_ids=first, position_ids=torch.arange(8, device="cuda")[None].expand(S * B, 8), past_key_values=cache,
                  use_cache=True)
            c0 = dict(ops.KV8_CALLS)
            out = model(input_ids=chunk, position_ids=torch.arange(8, 25, device="cuda")[None].expand(S * B, 17),
                        past_key_values=cache, use_cache=True)
            return out.logits.clone(), {k: ops.KV8_CALLS[k] - c0[k] for k in c0}

    got, moved = run(_static_cache(model, cap, kv_cache="fp8"))
    assert moved == {"append": 2, "decode": 0, "dequantize": 4}, moved  # per layer: one append, K and V dequantised
    oracle = StaticCache(config=model.model.config, max_cache_len=cap)
    oracle.layers = [_oracle_layer()(max_cache_len=cap) for _ in oracle.layers]
    want, _ = run(oracle)
    assert torch.equal(got, want)
