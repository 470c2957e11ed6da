"""The causal / grouped-query attention kernels take any sequence length: the host predicate, the switch that restores the
multiples-of-128 dispatch, and the C boundary the feature must not move (no GPU needed)."""
import pytest
import torch


def _qkv(T, D, H=8, Hkv=2, B=2, dtype=torch.bfloat16):
    q = torch.zeros(B, T, H * D, dtype=dtype).view(B, T, H, D).transpose(1, 2)
    k, v = (torch.zeros(B, T, Hkv * D, dtype=dtype).view(B, T, Hkv, D).transpose(1, 2) for _ in range(2))
    return q, k, v


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("T", [1, 100, 129, 1000])
def test_gqa_predicate_takes_any_length(T, D):
    from bayeformers_amd import ops

    q, k, v = _qkv(T, D)
    assert ops._gqa_supported(q, k, v, 2)
    assert ops._gqa_supported(q, k, v, None)  # the K/V head count read off k


def test_gqa_predicate_still_refuses_what_the_kernels_do_not_take():
    from bayeformers_amd import ops

    assert not ops._gqa_supported(*_qkv(100, 96), 2)                  # head size
    assert not ops._gqa_supported(*_qkv(100, 64, H=6, Hkv=4), 4)      # 4 K/V heads do not divide 6 query heads
    assert not ops._gqa_supported(*_qkv(0, 64), 2)                    # no token at all
    q, k, v = _qkv(100, 64)
    odd = torch.zeros(2, 100, 2 * 64 + 4, dtype=torch.bfloat16)[:, :, :128].view(2, 100, 2, 64).transpose(1, 2)
    assert odd.shape == k.shape and odd.stride(2) % 8 == 4
    assert not ops._gqa_supported(q, odd, v, 2)                       # a token stride that is no multiple of 8 elements
    assert not ops._gqa_supported(q, k, odd, 2)


def test_bidirectional_predicate_keeps_its_limit():
    """The encoder kernels (bf_attention_fwd, with dropout) still want T % 128 == 0: the shape part of the predicate,
    looked at on its own (attention_supported also asks for a device tensor)."""
    from bayeformers_amd import ops

    B, H, D = 2, 4, 64
    for T, want in ((100, False), (128, True), (200, False)):
        q, k, v = (torch.zeros(B, T, H * D, dtype=torch.bfloat16).view(B, T, H, D).transpose(1, 2) for _ in range(3))
        assert not ops.attention_supported(q, k, v)  # a CPU tensor never runs the kernels
        fake = [_AsDevice(t) for t in (q, k, v)]
        assert ops.attention_supported(*fake) is want, T


class _AsDevice:
    """a CPU tensor that says is_cuda: the shape / stride / alignment part of attention_supported without a GPU"""

    def __init__(self, t):
        self._t = t

    is_cuda = True

    def __getattr__(self, name):
        return getattr(self._t, name)


def test_switch_exists_flips_and_is_baked(monkeypatch):
    import bayeformers_amd as bf
    from bayeformers_amd import graphs

    monkeypatch.delenv("BF_NO_RAGGED_ATTENTION", raising=False)
    model = torch.nn.Linear(2, 2)
    assert bf.ragged_attention_enabled()  # on by default (every test that flips it flips it back)
    try:
        on = graphs.baked_state(model)
        assert graphs.still_valid(model, on)
        bf.ragged_attention(False)
        assert not bf.ragged_attention_enabled()
        off = graphs.baked_state(model)
        assert on != off and not graphs.still_valid(model, on) and graphs.still_valid(model, off)
        bf.ragged_attention(True)
        assert graphs.still_valid(model, on)
        monkeypatch.setenv("BF_NO_RAGGED_ATTENTION", "1")
        assert not bf.ragged_attention_enabled()
        assert graphs.baked_state(model) == off
    finally:
        bf.ragged_attention(True)


def test_c_boundary_did_not_move():
    """The feature adds no entry and changes no prototype: the six causal entries stop refusing ragged T, nothing else."""
    from bayeformers_amd import _C

    assert _C.ABI_VERSION == 6
    assert len(_C.SYMBOLS) == 90
