"""The ring-buffer KV cache of sample_generate(sliding_cache="ring") on the GPU.  The criterion is bitwise equality with
what the project already trusts: the ring appends against the pure-Python placement (and bf_kv8_append's bytes), the ring
decode against the window decode on the same keys in a linear cache, a captured append + decode step against the eager
linear-cache result while the fill wraps the ring twice, and sample_generate with the ring against the same call without
it, on every sliding-window family.  One case per head size is also held to the float64 reference of
tests/test_gpu_sliding_window.py at its DEC_TOL."""
from dataclasses import fields
from functools import lru_cache

import pytest
import torch

from ring_cache_ref import live_keys, placement
from test_gpu_sliding_window import DEC_TOL, SEED, _prompt, reference, rel_err

pytestmark = pytest.mark.gpu

HEADS = [(64, 8, 2), (128, 4, 4), (256, 8, 4)]  # (D, H, Hkv); the D 128 one is the class decode_kernel_wins sends to SDPA
N = 2


def _strided_rows(T, Hkv, D, dtype, seed):
    """k, v [N, Hkv, T, D] as a decoder's projections hand them over: transposed views of [N, T, Hkv * D]."""
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(N, T, Hkv * D, generator=g).to("cuda", dtype).view(N, T, Hkv, D).transpose(1, 2)
                 for _ in range(2))


# ---------------------------------------------------------------------------------------------------- append
@pytest.mark.parametrize("D", [64, 128, 256])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_ring_append_places_the_rows_and_touches_nothing_else(D, dtype):
    from bayeformers_amd import ops

    Hkv, C = 2, 22
    c0 = ops.RING_CALLS["append"]
    calls = 0
    for T in (1, 5, 16, C + 9):
        k, v = _strided_rows(T, Hkv, D, dtype, seed=D + T)
        for fill in (0, C - 3, 2 * C + 1):
            kc, vc = (torch.full((N, Hkv, C, D), s, dtype=dtype, device="cuda") for s in (-7.0, 9.0))
            ops.kv_ring_append(k, v, kc, vc, torch.tensor([fill], device="cuda"))
            calls += 1
            slots = placement(fill, T, C)
            for got, src, sentinel in ((kc, k, -7.0), (vc, v, 9.0)):
                want = torch.full_like(got, sentinel)
                for slot, row in slots.items():
                    want[:, :, slot] = src[:, :, row]
                assert torch.equal(got, want), (T, fill)
    assert ops.RING_CALLS["append"] - c0 == calls
    # a negative fill writes nothing
    kc, vc = (torch.full((N, Hkv, C, D), -7.0, dtype=dtype, device="cuda") for _ in range(2))
    ops.kv_ring_append(k, v, kc, vc, torch.tensor([-5], device="cuda"))
    assert (kc == -7.0).all() and (vc == -7.0).all()


@pytest.mark.parametrize("D", [64, 128, 256])
def test_fp8_ring_append_is_kv8_append_gathered_at_the_slots(D):
    from bayeformers_amd import ops

    Hkv, C = 2, 22
    for T in (1, 5, 16, C + 9):
        k, v = _strided_rows(T, Hkv, D, torch.bfloat16, seed=3 * D + T)
        for fill in (0, C - 3, 2 * C + 1):
            cap = fill + T
            lin = [torch.zeros(N, Hkv, cap, D, dtype=torch.uint8, device="cuda") for _ in range(2)]
            lin_s = [torch.zeros(N, Hkv, cap, device="cuda") for _ in range(2)]
            pos = torch.tensor([fill], device="cuda")
            ops.kv8_append(k, v, lin[0], lin[1], lin_s[0], lin_s[1], pos)
            ring = [torch.full((N, Hkv, C, D), 0xAB, dtype=torch.uint8, device="cuda") for _ in range(2)]
            ring_s = [torch.full((N, Hkv, C), -1.0, device="cuda") for _ in range(2)]
            ops.kv8_ring_append(k, v, ring[0], ring[1], ring_s[0], ring_s[1], pos)
            slots = placement(fill, T, C)
            for i in range(2):
                want, want_s = torch.full_like(ring[i], 0xAB), torch.full_like(ring_s[i], -1.0)
                for slot, row in slots.items():
                    want[:, :, slot], want_s[:, :, slot] = lin[i][:, :, fill + row], lin_s[i][:, :, fill + row]
                assert torch.equal(ring[i], want) and torch.equal(ring_s[i], want_s), (T, fill, i)


# ---------------------------------------------------------------------------------------------------- decode
GRID = [(40, 7, (1, 7, 22, 23, 40)),  # one split
        (1000, 129, (100, 144, 145, 700, 1000)),  # several tiles
        (4100, 1000, (4100,))]  # several splits plus the merge


def _ring_of(lin, L, C, fill_value):
    """The ring holding the keys [max(0, L - C), L) of the linear cache `lin` [N, Hkv, capacity, ...] at j % C; the slots
    never written hold `fill_value`."""
    ring = torch.full((lin.shape[0], lin.shape[1], C) + tuple(lin.shape[3:]), fill_value, dtype=lin.dtype, device=lin.device)
    held = live_keys(L, C)
    if held:
        keys = torch.tensor(list(held), device=lin.device)
        ring[:, :, torch.tensor(list(held.values()), device=lin.device)] = lin[:, :, keys]
    return ring


def _left_padded(capacity):
    mask = torch.zeros(N, capacity, device="cuda")
    mask[1, :max(1, capacity // 5)] = float("-inf")
    return mask


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("D,H,Hkv", HEADS)
@pytest.mark.parametrize("Tq", [1, 5, 16])
@pytest.mark.parametrize("capacity,W,fills", GRID, ids=["one-split", "tiles", "splits"])
def test_ring_decode_is_bitwise_the_window_decode_on_the_linear_cache(dtype, D, H, Hkv, Tq, capacity, W, fills):
    from bayeformers_amd import ops

    C = ops.ring_slots(W, capacity)
    assert C == W + 15 and C < capacity
    g = torch.Generator().manual_seed(capacity + W + Tq + D)
    q = torch.randn(N, Tq, H, D, generator=g).to("cuda", dtype).transpose(1, 2)
    k, v = (torch.randn(N, Hkv, capacity, D, generator=g).to("cuda", dtype) for _ in range(2))
    scale = D ** -0.5
    c0, d0 = ops.RING_CALLS["decode"], dict(ops.DECODE_CALLS)
    runs = 0
    for L in fills:
        kv_len = torch.tensor([L], device="cuda")
        kr, vr = _ring_of(k, L, C, float("nan")), _ring_of(v, L, C, float("nan"))
        for key_mask in (None, _left_padded(capacity)):
            for softcap in (None, 30.0):
                want = ops.attention_forward_decode_len(q, k, v, kv_len, key_mask, scale, window=W, softcap=softcap)
                got = ops.attention_forward_decode_ring(q, kr, vr, kv_len, key_mask, scale, None, None, W, C, capacity,
                                                        softcap=softcap)
                runs += 1
                assert torch.equal(got, want), (L, key_mask is not None, softcap)
                assert not torch.isnan(got).any()
    assert ops.RING_CALLS["decode"] - c0 == runs
    assert ops.DECODE_CALLS["len_window"] - d0["len_window"] == runs // 2  # (the references; the capped ones count elsewhere)


@pytest.mark.parametrize("D,H,Hkv", HEADS)
@pytest.mark.parametrize("Tq,capacity,W,fills", [(1, 40, 7, (7, 23, 40)), (16, 40, 7, (22, 40)), (5, 1000, 129, (145, 1000)),
                                                 (1, 4100, 1000, (4100,))])
def test_fp8_ring_decode_is_bitwise_the_kv8_decode_on_the_linear_cache(D, H, Hkv, Tq, capacity, W, fills):
    from bayeformers_amd import ops

    C = ops.ring_slots(W, capacity)
    g = torch.Generator().manual_seed(capacity + W + Tq + D)
    q = torch.randn(N, Tq, H, D, generator=g).to("cuda", torch.bfloat16).transpose(1, 2)
    k, v = (torch.randn(N, Hkv, capacity, D, generator=g).to("cuda", torch.bfloat16) for _ in range(2))
    kq, vq = (torch.zeros(N, Hkv, capacity, D, dtype=torch.uint8, device="cuda") for _ in range(2))
    ks, vs = (torch.zeros(N, Hkv, capacity, device="cuda") for _ in range(2))
    ops.kv8_append(k, v, kq, vq, ks, vs, torch.tensor([0], device="cuda"))
    scale = D ** -0.5
    c0, k0 = ops.RING_CALLS["kv8_decode"], ops.KV8_CALLS["decode"]
    runs = 0
    for L in fills:
        kv_len = torch.tensor([L], device="cuda")
        # the slots never written: e4m3 NaN bytes under NaN scales
        rq, rv = _ring_of(kq, L, C, 0x7F), _ring_of(vq, L, C, 0x7F)
        rks, rvs = _ring_of(ks, L, C, float("nan")), _ring_of(vs, L, C, float("nan"))
        for key_mask in (None, _left_padded(capacity)):
            for softcap in (None, 30.0):
                want = ops.attention_forward_decode_kv8(q, kq, vq, ks, vs, kv_len, key_mask, scale, window=W, softcap=softcap)
                got = ops.attention_forward_decode_ring_kv8(q, rq, rv, rks, rvs, kv_len, key_mask, scale, None, None, W, C,
                                                            capacity, softcap=softcap)
                runs += 1
                assert torch.equal(got, want), (L, key_mask is not None, softcap)
                assert not torch.isnan(got).any()
    assert ops.RING_CALLS["kv8_decode"] - c0 == runs and ops.KV8_CALLS["decode"] - k0 == runs


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("D,H,Hkv", HEADS)
def test_ring_decode_matches_float64(dtype, D, H, Hkv):
    from bayeformers_amd import ops

    capacity, W, L, Tq = 1000, 129, 700, 5
    C = ops.ring_slots(W, capacity)
    g = torch.Generator().manual_seed(D)
    q = torch.randn(N, Tq, H, D, generator=g).to("cuda", dtype).transpose(1, 2)
    k, v = (torch.randn(N, Hkv, capacity, D, generator=g).to("cuda", dtype) for _ in range(2))
    key_mask = _left_padded(capacity)
    got = ops.attention_forward_decode_ring(q, _ring_of(k, L, C, float("nan")), _ring_of(v, L, C, float("nan")),
                                            torch.tensor([L], device="cuda"), key_mask, D ** -0.5, None, None, W, C, capacity)
    r = reference(q, k[:, :, :L], v[:, :, :L], key_mask[:, :L], D ** -0.5, W)[0]
    err = rel_err(got, r)
    print(f"ring decode {str(dtype)[6:]} D={D} H={H} Hkv={Hkv}: {err:.2e}")
    assert torch.isfinite(got).all() and err <= DEC_TOL[dtype], err


# ---------------------------------------------------------------------------------------------------- capture
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_a_captured_ring_step_replays_while_the_fill_wraps_the_ring_twice(fp8):
    from bayeformers_amd import ops

    D, H, Hkv, W, capacity, start = 64, 8, 2, 25, 128, 5
    C = ops.ring_slots(W, capacity)
    assert C == 40
    g = torch.Generator().manual_seed(17)
    qs = torch.randn(capacity, N, 1, H, D, generator=g).to("cuda", torch.bfloat16)
    k, v = (torch.randn(N, Hkv, capacity, D, generator=g).to("cuda", torch.bfloat16) for _ in range(2))
    scale = D ** -0.5
    if fp8:  # the linear FP8 cache the eager reference reads
        kq, vq = (torch.zeros(N, Hkv, capacity, D, dtype=torch.uint8, device="cuda") for _ in range(2))
        ks, vs = (torch.zeros(N, Hkv, capacity, device="cuda") for _ in range(2))
        ops.kv8_append(k, v, kq, vq, ks, vs, torch.tensor([0], device="cuda"))
        ring = [torch.zeros(N, Hkv, C, D, dtype=torch.uint8, device="cuda") for _ in range(2)]
        ring += [torch.zeros(N, Hkv, C, device="cuda") for _ in range(2)]
        append, decode = ops.kv8_ring_append, ops.attention_forward_decode_ring_kv8
    else:
        ring = [torch.zeros(N, Hkv, C, D, dtype=torch.bfloat16, device="cuda") for _ in range(2)]
        append, decode = ops.kv_ring_append, ops.attention_forward_decode_ring
    fill = torch.tensor([0], device="cuda")  # the device fill pointer: counts every row, never wraps
    append(k[:, :, :start], v[:, :, :start], *ring, fill)
    fill.add_(start)
    q = qs[0].transpose(1, 2).clone()
    k_new, v_new = k[:, :, :1].clone(), v[:, :, :1].clone()
    out = torch.empty(N, 1, H, D, dtype=torch.bfloat16, device="cuda")

    def step():
        append(k_new, v_new, *ring, fill)
        fill.add_(1)
        out.copy_(decode(q, *ring, fill, None, scale, None, None, W, C, capacity))

    def load(t):
        q.copy_(qs[t].transpose(1, 2))
        k_new.copy_(k[:, :, t:t + 1])
        v_new.copy_(v[:, :, t:t + 1])

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        load(start)
        step()  # eagerly once (the key at `start`), outside the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    load(start + 1)
    with torch.cuda.graph(graph):
        step()
    fill.fill_(start + 1)  # (the capture launched nothing: the fill is where the eager step left it)
    for t in range(start + 1, 2 * C + 12):  # from below W past 2 C
        load(t)
        graph.replay()
        L = torch.tensor([t + 1], device="cuda")
        assert int(fill) == t + 1
        if fp8:
            want = ops.attention_forward_decode_kv8(q, kq, vq, ks, vs, L, None, scale, window=W)
        else:
            want = ops.attention_forward_decode_len(q, k, v, L, None, scale, window=W)
        assert torch.equal(out, want), t


# ---------------------------------------------------------------------------------------------------- models
W_MODEL = 20  # C = 35: the prompt of 96 has wrapped the ring twice at the hand-over, the 23 decode steps wrap it again
FAMILIES = {
    "mistral": dict(sliding_window=W_MODEL),
    "qwen2": dict(sliding_window=W_MODEL, use_sliding_window=True, max_window_layers=1,
                  layer_types=["full_attention", "sliding_attention"]),
    "qwen3": dict(sliding_window=W_MODEL, use_sliding_window=True, max_window_layers=0,
                  layer_types=["sliding_attention", "sliding_attention"]),
    "gemma2": dict(sliding_window=W_MODEL, layer_types=["sliding_attention", "full_attention"], attn_logit_softcapping=1.0,
                   final_logit_softcapping=None, query_pre_attn_scalar=1),
}


def _sliding_layers(kind):
    return FAMILIES[kind].get("layer_types", ["sliding_attention"] * 2).count("sliding_attention")


@lru_cache(maxsize=None)
def _decoder(kind):
    """tests/test_gpu_sliding_window.py's _decoder at sliding_window = 20, in bf16, routed by fuse_attention (Gemma 2 on its
    eager attention, the framework's only one that applies the cap)."""
    from transformers import AutoConfig, AutoModelForCausalLM

    import bayeformers_amd as bf

    cfg = AutoConfig.for_model(kind, hidden_size=256, num_attention_heads=4, num_key_value_heads=2, head_dim=64,
                               num_hidden_layers=2, intermediate_size=512, vocab_size=512, max_position_embeddings=1024,
                               tie_word_embeddings=False, attention_dropout=0.0,
                               attn_implementation="eager" if kind == "gemma2" else "sdpa", **FAMILIES[kind])
    torch.manual_seed(0)
    bmodel = bf.to_bayesian(AutoModelForCausalLM.from_config(cfg).eval(), delta=0.05, freeze=True).eval().cuda()
    freqs = {n: b.detach().clone() for n, b in bmodel.named_buffers() if "inv_freq" in n}
    bmodel = bmodel.to(torch.bfloat16)
    for n, b in freqs.items():
        setattr(bmodel.get_submodule(n.rsplit(".", 1)[0]), n.rsplit(".", 1)[1], b)
    assert bf.fuse_attention(bmodel)
    return bmodel


@pytest.fixture
def softcap_on():
    import bayeformers_amd as bf

    bf.softcap_attention()
    yield
    bf.softcap_attention(False)


@pytest.fixture
def caches(monkeypatch):
    """The static caches sample_generate builds, in call order."""
    from bayeformers_amd import sampling

    built, real = [], sampling._static_cache

    def record(*a, **k):
        built.append(real(*a, **k))
        return built[-1]

    monkeypatch.setattr(sampling, "_static_cache", record)
    return built


def _generate(model, ids, mask, **kw):
    import bayeformers_amd as bf
    from bayeformers_amd.sampling import sample_generate

    bf.manual_seed(SEED)
    with torch.no_grad():
        return sample_generate(model, ids, attention_mask=mask, samples=3, max_new_tokens=24, **kw)


def _store_bytes(cache):
    return sum(layer.store_bytes() if hasattr(layer, "store_bytes")
               else sum(t.numel() * t.element_size() for t in (layer.keys, layer.values)) for layer in cache.layers)


def _same(a, b):
    return all(torch.equal(getattr(a, f.name), getattr(b, f.name)) for f in fields(a))


@pytest.mark.parametrize("fp8", [None, "fp8"], ids=["bf16", "fp8"])
@pytest.mark.parametrize("kind", list(FAMILIES))
def test_ring_generation_is_bitwise_the_static_generation(kind, fp8, softcap_on, caches):
    from bayeformers_amd import ops
    from bayeformers_amd.kv_cache import Fp8RingStaticLayer, RingStaticLayer
    from bayeformers_amd.plan import kv_cache_bytes

    model = _decoder(kind)
    ids, mask = _prompt(T=96, pad=5)
    sliding, steps = _sliding_layers(kind), 23
    append, decode = ("kv8_append", "kv8_decode") if fp8 else ("append", "decode")
    base = dict(kv_cache=fp8) if fp8 else dict(static_cache=True)
    plain = _generate(model, ids, mask, **base)
    r0, d0, s0, k0 = dict(ops.RING_CALLS), dict(ops.DECODE_CALLS), dict(ops.SOFTCAP_CALLS), dict(ops.KV8_CALLS)
    ring = _generate(model, ids, mask, sliding_cache="ring", **({"kv_cache": fp8} if fp8 else {}))
    assert _same(ring, plain)
    # every sliding layer: the hand-over's append and one per step; one ring decode per step; nothing on the window entries
    assert ops.RING_CALLS[decode] - r0[decode] == sliding * steps
    assert ops.RING_CALLS[append] - r0[append] == sliding * (steps + 1)
    assert {k: ops.RING_CALLS[k] - r0[k] for k in r0 if k not in (append, decode)} == {
        k: 0 for k in r0 if k not in (append, decode)}
    assert ops.DECODE_CALLS["len_window"] == d0["len_window"]
    full = (2 - sliding) * steps  # the full-attention layers decode where they did
    if fp8:
        assert ops.KV8_CALLS["decode"] - k0["decode"] == full
    elif kind == "gemma2":
        assert ops.SOFTCAP_CALLS["decode_len"] - s0["decode_len"] == full
    else:
        assert ops.DECODE_CALLS["len"] - d0["len"] == full
    r1 = dict(ops.RING_CALLS)
    graph = _generate(model, ids, mask, sliding_cache="ring", graph=True, **({"kv_cache": fp8} if fp8 else {}))
    assert _same(graph, plain)
    # eager step 1 + the captured step 2: the replays enqueue nothing from Python
    assert ops.RING_CALLS[decode] - r1[decode] == sliding * 2
    assert ops.RING_CALLS[append] - r1[append] == sliding * 3

    # the memory: what the caches hold is what the plan counts
    S, B, capacity = 3, ids.shape[0], 96 + 24 - 1
    assert len(caches) == 3
    want_ring = kv_cache_bytes(model, S, B, capacity, fp8=bool(fp8), ring=True)
    want_full = kv_cache_bytes(model, S, B, capacity, fp8=bool(fp8))
    assert _store_bytes(caches[0]) == want_full
    assert _store_bytes(caches[1]) == _store_bytes(caches[2]) == want_ring < want_full
    cls = Fp8RingStaticLayer if fp8 else RingStaticLayer
    assert sum(type(layer) is cls for layer in caches[1].layers) == sliding
    for layer in caches[1].layers:
        assert int(layer.cumulative_length) == capacity and layer.max_cache_len == capacity
        if type(layer) is cls:
            assert layer.ring_slots == 35 and layer.keys.shape[2] == 35


def test_seventeen_queries_against_a_ring_raise_and_do_not_return():
    from bayeformers_amd.sampling import _static_cache

    model = _decoder("mistral")
    ids, _ = _prompt(T=17)
    cache = _static_cache(model, 119, sliding_cache="ring")
    with torch.no_grad(), model.monte_carlo(1), model.pinned_samples():
        with pytest.raises(RuntimeError, match="ring-buffer cache.*17 queries"):
            model(input_ids=ids, past_key_values=cache, use_cache=True)
