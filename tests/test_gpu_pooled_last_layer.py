"""The narrow last encoder layer of a pooled-head model (bayeformers_amd._pooled_last_layer_forward, installed by
fuse_attention): the same logits and log-probs as the full layer on the benchmarked BERT-base, and every case that must
keep the full layer keeps it — proven by the FLOP count of the tiled-GEMM launches (bf_profile_read), not by timing."""
import ctypes

import numpy as np
import pytest
import torch

import bayeformers_amd as bf
from bayeformers_amd import _C, ops
from bayeformers_amd import random as bfr
from bayeformers_amd.sampling import sample_bayesian

SEED = 0x5EED
S = 10


def _tiny(cls_name="BertForSequenceClassification"):
    import transformers

    cfg = transformers.BertConfig(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
                                  vocab_size=100, max_position_embeddings=128)
    torch.manual_seed(0)
    return getattr(transformers, cls_name)(cfg).eval()


def _fuse(model):
    b = bf.to_bayesian(model, delta=0.05, freeze=True).eval()
    bf.fuse_activations(b)
    bf.fuse_residual_layernorm(b)
    bf.fuse_shared_inputs(b)
    assert bf.fuse_attention(b) is True
    return b


# ------------------------------------------------------------------------------------------ the dispatch predicate (CPU)
def test_rewrite_is_installed_on_the_pooled_head_only():
    b = _fuse(_tiny())
    head = b.model
    last = head.bert.encoder.layer[-1]
    assert head.forward.__func__ is bf._pooled_head_forward and last.forward.__func__ is bf._pooled_last_layer_forward
    assert "forward" not in head.bert.encoder.layer[0].__dict__
    assert bf._pooled_fusions_installed(last) and not bf._pooled_active(last)
    qa = _fuse(_tiny("BertForQuestionAnswering"))
    assert all("_bf_plain_layer_forward" not in m.__dict__ and "_bf_plain_forward" not in m.__dict__ for m in qa.modules()
               if type(m).__name__ in ("BertLayer", "BertForQuestionAnswering", "BertModel"))


def test_missing_fusions_keep_the_full_layer():
    model = _tiny()
    b = bf.to_bayesian(model, delta=0.05, freeze=True).eval()
    bf.fuse_activations(b)
    assert bf.fuse_attention(b) is True          # installed, but residual+LayerNorm and Q/K/V fusions are not
    assert not bf._pooled_fusions_installed(b.model.bert.encoder.layer[-1])
    bf.fuse_residual_layernorm(b)
    assert not bf._pooled_fusions_installed(b.model.bert.encoder.layer[-1])
    bf.fuse_shared_inputs(b)
    assert bf._pooled_fusions_installed(b.model.bert.encoder.layer[-1])


def test_head_forward_flags_the_layer_only_when_every_condition_holds(monkeypatch):
    b = _fuse(_tiny())
    head = b.model
    last = head.bert.encoder.layer[-1]
    seen = []
    monkeypatch.setattr(head, "_bf_plain_forward", lambda *a, **k: seen.append(bf._pooled_active(last)))

    def flagged(**kw):
        seen.clear()
        head.forward(**kw)
        assert not bf._pooled_active(last)   # never left set
        return seen[0]

    with torch.no_grad():
        assert flagged() is True
        assert flagged(output_hidden_states=True) is False
        assert flagged(output_attentions=True) is False
        from transformers.utils.output_capturing import install_output_capuring_hook

        install_output_capuring_hook(last, "hidden_states", 0)   # what one output_hidden_states=True call leaves behind
        assert flagged() is True
        h = last.output.register_forward_hook(lambda *a: None)
        assert flagged() is False
        h.remove()
        h = head.bert.pooler.register_forward_pre_hook(lambda *a: None)
        assert flagged() is False
        h.remove()
        assert flagged() is True
        head.config.output_hidden_states = True
        assert flagged() is False
        head.config.output_hidden_states = False
        head.train()
        assert flagged() is False
        head.eval()
        # Monte-Carlo dropout: an eval() model whose Dropout modules alone are switched back on — each of the last layer's
        for drop in (last.output.dropout, last.attention.output.dropout, last.attention.self.dropout):
            drop.train()
            assert not last.training and flagged() is False
            drop.eval()
        assert flagged() is True
        bf.pooled_last_layer(False)
        try:
            assert flagged() is False
        finally:
            bf.pooled_last_layer(True)
        monkeypatch.setenv("BF_NO_POOLED_LAST_LAYER", "1")
        assert flagged() is False
        monkeypatch.delenv("BF_NO_POOLED_LAST_LAYER")
        assert flagged() is True
    assert flagged() is False                     # grad mode


# ------------------------------------------------------------------------------------------------------------ on the GPU
def _gemm_profile(fn):
    """(tiled-GEMM launches, their FLOP, whatever fn returned) of one call of fn."""
    lib = _C.lib()
    lib.bf_profile_reset()
    lib.bf_profile_enable(1)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        lib.bf_profile_enable(0)
    n, ms, work = ctypes.c_uint64(), ctypes.c_double(), ctypes.c_double()
    _C.check(lib.bf_profile_read(_C.BF_PROF_GEMM, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(work)), "bf_profile_read")
    lib.bf_profile_reset()
    return n.value, work.value, out


def _flop(S_, rows, narrow_rows, layers=12, H=768, F=3072):
    """FLOP of the tiled launches of a BERT forward: `layers - 1` full layers and one whose three dense layers behind the
    query / key / value launch run on narrow_rows rows per sample."""
    per_row_qkv, per_row_rest = 2.0 * 3 * H * H, 2.0 * (H * H + 2 * H * F)
    return S_ * ((layers - 1) * rows * (per_row_qkv + per_row_rest) + rows * per_row_qkv + narrow_rows * per_row_rest)


@pytest.fixture(scope="module")
def bert():
    import bench

    bf.set_compute_dtype("bf16")
    bmodel, _, inputs, ids, labels, info = bench.build_bert(torch.device("cuda"), "bf16")
    # one forward first: the pooler and the classifier find out in their first forward that they run the single small-M
    # kernel and leave the sampling plan, which moves their log-prob sums to another (equally valid) summation order
    with torch.no_grad():
        sample_bayesian(bmodel, inputs, S)
        bmodel(**inputs)
    return bmodel, inputs


def _last_and_logits(out):
    return out.logits, out.hidden_states[-1], out.hidden_states[-2]


@pytest.mark.gpu
def test_same_logits_and_log_probs_as_the_full_layer(bert):
    """BERT-base as benchmarked, S = 10, the same seed: the narrow path against the full one (forced by
    output_hidden_states=True).  The log-prob sums are bit-equal (the sampling launch is the same).  The logits are not
    asked to be bit-equal: the three dense layers of the narrow path stream W_s through the small-M kernel, which sums each
    output's k in four interleaved wave-partials (and, at K = 3072, three workgroup splits) instead of the ring kernel's
    single running sum.  So both paths are measured against a float64 evaluation of layer 11, the pooler and the classifier
    on the SAME sampled weights and the same layer-11 input, and the narrow path must be no worse than 1.5 x the full
    path's own error (the margin covers a different fp32 summation order over K = 768 / 3072 and nothing more)."""
    bmodel, inputs = bert
    B, L = inputs["input_ids"].shape
    calls0 = dict(ops.ROWS_CALLS)
    bf.manual_seed(SEED)
    with torch.no_grad():
        n_n, fl_n, (raw_n, _, lp_n, lq_n) = _gemm_profile(lambda: sample_bayesian(bmodel, inputs, S))
    lps_n = bmodel.log_prob_samples().clone()
    assert {k: ops.ROWS_CALLS[k] - calls0[k] for k in calls0} == {"gemm": 3, "attention": 1, "layernorm": 1}
    bf.manual_seed(SEED)
    with torch.no_grad():
        n_f, fl_f, (raw_f, _, lp_f, lq_f) = _gemm_profile(
            lambda: sample_bayesian(bmodel, dict(inputs, output_hidden_states=True), S, select=_last_and_logits))
    lps_f = bmodel.log_prob_samples().clone()
    assert n_n == n_f == 48
    assert fl_f == _flop(S, B * L, B * L) and fl_n == _flop(S, B * L, B)
    print(f"[pooled last layer] max |log-prob sums, narrow - full| = {(lps_n - lps_f).abs().max().item():.3e}")
    assert torch.equal(lps_n, lps_f) and torch.equal(lp_n, lp_f) and torch.equal(lq_n, lq_f)
    logits_n, logits_f = raw_n[0].double().view(S * B, -1), raw_f[0].double().view(S * B, -1)
    hidden = bmodel.model.config.hidden_size
    assert tuple(raw_f[1].shape[-2:]) == (L, hidden)       # the full path materialises every row of the last layer
    h = raw_f[2].reshape(S, B * L, hidden).double()          # layer 11's input: the same tensor in both paths

    # the sampled weights of this forward: layer 11's from the plan's arena, the pooler's and the classifier's (small-M
    # kernel: sampled in registers) drawn again from the same counters
    plan, head = bmodel._plan, bmodel.model
    last = head.bert.encoder.layer[-1]

    def planned(layer):
        w, b = plan.views[id(layer)]
        return w.double(), b.double()

    def drawn(layer):
        from bayeformers_amd.nn.parameters.base import NoneParameter

        outs, _ = ops.sample_logprob([layer.weight, layer.bias], [NoneParameter()] * 2,
                                     [2 * layer.layer_id, 2 * layer.layer_id + 1], S, bfr.STATE.seed, bmodel._last_base,
                                     out_dtype=torch.float32)
        return outs[0].to(torch.bfloat16).double(), outs[1].double()

    def lin(x, wb):
        return torch.einsum("smk,snk->smn", x, wb[0]) + wb[1][:, None, :]

    def ln(x, m):
        mu, var = x.mean(-1, keepdim=True), x.var(-1, unbiased=False, keepdim=True)
        return (x - mu) / torch.sqrt(var + m.eps) * m.weight.double() + m.bias.double()

    sa = last.attention.self
    Hh, D = sa.num_attention_heads, sa.attention_head_size
    cls = h.view(S, B, L, hidden)[:, :, 0]
    q = lin(cls, planned(sa.query)).view(S, B, Hh, D)
    k = lin(h, planned(sa.key)).view(S, B, L, Hh, D)
    v = lin(h, planned(sa.value)).view(S, B, L, Hh, D)
    p = torch.softmax(torch.einsum("sbhd,sblhd->sbhl", q, k) * sa.scaling, dim=-1)   # (the benchmark's mask hides nothing)
    a = torch.einsum("sbhl,sblhd->sbhd", p, v).reshape(S, B, hidden)
    y = ln(lin(a, planned(last.attention.output.dense)) + cls, last.attention.output.LayerNorm)
    z = lin(y, planned(last.intermediate.dense))
    z = 0.5 * z * (1.0 + torch.erf(z / np.sqrt(2.0)))
    z = ln(lin(z, planned(last.output.dense)) + y, last.output.LayerNorm)
    pooled = torch.tanh(lin(z, drawn(head.bert.pooler.dense)))
    ref = lin(pooled, drawn(head.classifier)).view(S * B, -1)

    err_n, err_f = (logits_n - ref).abs().max().item(), (logits_f - ref).abs().max().item()
    rms_n, rms_f = (logits_n - ref).pow(2).mean().sqrt().item(), (logits_f - ref).pow(2).mean().sqrt().item()
    print(f"[pooled last layer] bit-equal logits: {bool(torch.equal(logits_n, logits_f))}; max |logit - fp64|: narrow "
          f"{err_n:.3e}, full {err_f:.3e} (ratio {err_n / err_f:.3f}); rms: narrow {rms_n:.3e}, full {rms_f:.3e} "
          f"(ratio {rms_n / rms_f:.3f}); max |narrow - full| {(logits_n - logits_f).abs().max().item():.3e}; "
          f"max |logit| {ref.abs().max().item():.3f}")
    assert err_n <= 1.5 * err_f and rms_n <= 1.5 * rms_f


@pytest.mark.gpu
def test_fallbacks_run_the_full_layer(bert):
    bmodel, inputs = bert
    B, L = inputs["input_ids"].shape
    full, narrow = _flop(1, B * L, B * L), _flop(1, B * L, B)
    last = bmodel.model.bert.encoder.layer[-1]

    def run(**extra):
        bf.manual_seed(SEED)
        return _gemm_profile(lambda: bmodel(**dict(inputs, **extra)))

    was = bmodel.graph_replay
    bmodel.graph_replay = False
    try:
        with torch.no_grad():
            n, fl, out = run()
            assert (n, fl) == (48, narrow)
            logits = out.logits.clone()
            n, fl, out = run(output_hidden_states=True)
            assert (n, fl) == (48, full) and tuple(out.hidden_states[-1].shape) == (B, L, bmodel.model.config.hidden_size)
            want_last = out.hidden_states[-1].clone()
            fired = []
            hook = last.output.register_forward_hook(lambda m, a, o: fired.append(tuple(o.shape)))
            try:
                for _ in range(2):
                    n, fl, out = run()
                    assert (n, fl) == (48, full)
                assert fired == [(B, L, bmodel.model.config.hidden_size)] * 2
                full_logits = out.logits.clone()
            finally:
                hook.remove()
            bf.pooled_last_layer(False)
            try:
                n, fl, out = run(output_hidden_states=True)
                assert (n, fl) == (48, full) and torch.equal(out.hidden_states[-1], want_last)  # the full path is today's
                assert torch.equal(out.logits, full_logits)
            finally:
                bf.pooled_last_layer(True)
            n, fl, out = run()
            assert (n, fl) == (48, narrow) and torch.equal(out.logits, logits)
        n, fl, _ = run()                                   # grad mode
        assert (n, fl) == (48, full)
    finally:
        bmodel.graph_replay = was


@pytest.mark.gpu
def test_question_answering_never_takes_the_narrow_path():
    import transformers

    cfg = transformers.BertConfig(hidden_size=256, num_hidden_layers=2, num_attention_heads=4, intermediate_size=512)
    torch.manual_seed(0)
    b = _fuse(transformers.BertForQuestionAnswering(cfg).eval()).cuda().to(torch.bfloat16)
    bf.set_compute_dtype("bf16")
    B, L = 2, 128
    ids = torch.randint(0, cfg.vocab_size, (B, L), device="cuda")
    calls0 = dict(ops.ROWS_CALLS)
    bf.manual_seed(SEED)
    with torch.no_grad():
        n, fl, _ = _gemm_profile(lambda: b(input_ids=ids))
    assert ops.ROWS_CALLS == calls0
    # (the span head's own launch comes on top of the encoder's 8: at least the full layers' FLOP, never the narrow count)
    assert n >= 8 and fl >= _flop(1, B * L, B * L, layers=2, H=256, F=512)


@pytest.mark.gpu
def test_switch_recaptures_a_replayed_forward(bert):
    """A forward replayed from a HIP graph was captured with the narrow layer; flipping the switch captures it again (the
    switch is part of graphs.baked_state), so the replays are the eager steps of the path now asked for, bit for bit."""
    bmodel, inputs = bert

    def loop(n=5):
        bf.manual_seed(SEED)
        with torch.no_grad():
            return [bmodel(**inputs).logits.clone() for _ in range(n)]

    def same(a, b):
        return all(torch.equal(x, y) for x, y in zip(a, b))

    was = bmodel.graph_replay
    try:
        bmodel.graph_replay = False
        narrow = loop()
        bf.pooled_last_layer(False)
        try:
            full = loop()
        finally:
            bf.pooled_last_layer(True)
        assert not same(narrow, full)             # (the two paths sum k in different orders)
        bmodel.graph_replay = True
        assert same(loop(), narrow) and len(bmodel._graphs.forwards) == 1
        captures = bmodel._graphs.forwards[0][1].captures
        bf.pooled_last_layer(False)
        try:
            assert same(loop(), full)
        finally:
            bf.pooled_last_layer(True)
        assert bmodel._graphs.forwards[0][1].captures == captures + 1
        assert same(loop(), narrow)
    finally:
        bmodel.graph_replay = was
        bmodel._graphs.close()
