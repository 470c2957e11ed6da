"""Host side of sample_generate(speculative=γ) (no GPU): the torch restatement of bf_spec_accept's contract
(tests/speculative_ref.py) against a naive sequential greedy loop on hand-built cases, the entry's header, symbol and
refusals, plan.mean_weight_bytes, and what sample_generate refuses before any launch."""
import os

import pytest
import torch

import speculative_ref as ref
from speculative_ref import B, EOS, G, N_NEW, PAD, S, T0, V

CASES = ref.hand_cases()


def _naive(args):
    """Sequential greedy decoding from the same per-position argmax table: position j's token is argmax[:, j] for every
    row; the next position may be read only while every row that was live when the iteration began drafted exactly that
    token (the table's next column is conditioned on the drafts), and while a token is left before n."""
    step, eos = int(args["state"][0]), args["eos_token_id"]
    fin0 = args["finished"] if eos is not None else torch.zeros(B, dtype=torch.bool)
    kept = 0
    while step + kept < N_NEW:
        kept += 1
        j = kept - 1
        if j >= G or step + kept >= N_NEW:
            break
        if any(int(args["draft"][b, j]) != int(args["argmax"][b, j]) for b in range(B) if not bool(fin0[b])):
            break
    toks, added, fin = ref.greedy_replay(args["argmax"], step, N_NEW, kept, fin0, eos, PAD)
    return kept, toks, added, fin


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_is_sequential_greedy_decoding(name):
    args0, expect = CASES[name]
    args = ref.clone_args(args0)
    ref.speculative_accept(**args)
    step = int(args0["state"][0])
    if expect is None:
        assert int(args["rewind"][0]) == G + 1
        for k, v in args0.items():
            if isinstance(v, torch.Tensor) and k != "rewind":
                assert torch.equal(args[k], v), k
        return
    kept, toks, added, fin = _naive(args0)
    a = kept - 1
    assert a == expect
    assert int(args["state"][0]) == step + kept and int(args["state"][1]) == 0
    assert int(args["rewind"][0]) == G - a
    assert torch.equal(args["sequences"][:, T0 + step:T0 + step + kept], toks)
    assert (args["sequences"][:, :T0 + step] == -5).all() and (args["sequences"][:, T0 + step + kept:] == -5).all()
    assert torch.equal(args["lengths"], args0["lengths"] + added)
    if args0["eos_token_id"] is not None:
        assert torch.equal(args["finished"], fin)
    # the statistics: the position's entropies and the probability of the token written; zero where the row emitted pad
    fin0 = args0["finished"] if args0["eos_token_id"] is not None else torch.zeros(B, dtype=torch.bool)
    live = ~fin0
    for j in range(kept):
        for b in range(B):
            r = b * (G + 1) + j
            want = [0.0] * 4
            if bool(live[b]):
                want = [float(args0[k][r]) for k in ("predictive_entropy", "expected_entropy", "mutual_information")]
                want.append(float(args0["probs"][r, int(toks[b, j])]))
            assert [float(x) for x in args["stats"][:, b, step + j]] == want, (j, b)
        if args0["eos_token_id"] is not None:
            live = live & (toks[:, j] != EOS)
    assert (args["stats"][:, :, :step] == -1).all() and (args["stats"][:, :, step + kept:] == -1).all()
    # the next iteration's inputs
    before = toks[:, -2] if kept > 1 else args0["verify_ids"][:B, 0]
    assert torch.equal(args["draft_ids"], torch.stack([before, toks[:, -1]], 1))
    assert torch.equal(args["verify_ids"][:, 0], toks[:, -1].repeat(S)) and (args["verify_ids"][:, 1:] == -7).all()
    assert torch.equal(args["verify_positions"], args0["verify_positions"] + kept)
    assert torch.equal(args["draft_positions"], args0["draft_positions"] + kept)
    room = min(G, N_NEW - step - 1)
    assert args["speculation"].tolist() == [3 + 1, 10 + room, 4 + a]


def test_header_and_symbol():
    from bayeformers_amd import _C

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "bayeformers_amd_spec.h")).read()
    assert "int bf_spec_accept(" in header and set(_C.SPEC_SYMBOLS) == {"bf_spec_accept"}
    assert '#include "bayeformers_amd_spec.h"' in open(os.path.join(root, "include", "bayeformers_amd.h")).read()
    assert _C.lib().bf_spec_accept.argtypes == _C.SPEC_SYMBOLS["bf_spec_accept"][1]


def _entry_args(**kw):
    """bf_spec_accept's arguments on host memory: every refusal below is made before anything is launched."""
    import ctypes

    a = ref.clone_args(CASES["minimum_rules"][0])
    a["finished"] = a["finished"].to(torch.uint8)
    a.update(kw)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr() if isinstance(t, torch.Tensor) else t)
    _entry_args.keep = a
    return (ptr(a["argmax"]), ptr(a["draft"]), ptr(a["probs"]), ptr(a["predictive_entropy"]), ptr(a["expected_entropy"]),
            ptr(a["mutual_information"]), a.get("B", B), a.get("G", G), a.get("V", V), S, ptr(a["state"]), a.get("n", N_NEW),
            ptr(a["sequences"]), a.get("seq_stride", T0 + N_NEW), T0, ptr(a["stats"]), ptr(a["finished"]), ptr(a["lengths"]),
            ptr(a["verify_ids"]), ptr(a["verify_positions"]), ptr(a["draft_ids"]), ptr(a["draft_positions"]),
            ptr(a["rewind"]), ptr(a["speculation"]), EOS, PAD, None)


@pytest.mark.parametrize("kw,what", [(dict(G=0), b"gamma"), (dict(B=4), b"at most 16"), (dict(B=0), b"gamma"),
                                     (dict(V=0), b"positive"), (dict(n=0), b"positive"), (dict(seq_stride=T0 + N_NEW - 1), b"hold"),
                                     (dict(rewind=0), b"NULL"), (dict(finished=0), b"finished"), (dict(state=12), b"aligned")])
def test_entry_refuses(kw, what):
    from bayeformers_amd import _C

    lib = _C.lib()
    assert lib.bf_spec_accept(*_entry_args(**kw)) != 0 and what in lib.bf_last_error()


# ---- plan.mean_weight_bytes and sample_generate's refusals ---------------------------------------------------------------
def _small_llama():
    from transformers import LlamaConfig, LlamaForCausalLM

    import bayeformers_amd as bf

    cfg = LlamaConfig(hidden_size=64, num_attention_heads=4, num_key_value_heads=2, num_hidden_layers=2,
                      intermediate_size=128, vocab_size=96, max_position_embeddings=64, tie_word_embeddings=False)
    torch.manual_seed(0)
    return bf.to_bayesian(LlamaForCausalLM(cfg).eval(), delta=0.05, freeze=True).eval()


def test_mean_weight_bytes():
    import bayeformers_amd.nn as bnn
    from bayeformers_amd import plan

    model = _small_llama()
    P = sum(l.in_features * l.out_features for l in model.fused_children() if isinstance(l, bnn.Linear))
    assert P > 0 and plan.mean_weight_bytes(model, torch.bfloat16) == 2 * P == plan.mean_weight_bytes(model, torch.float16)
    assert plan.mean_weight_bytes(model, torch.float32) == 4 * P
    assert plan.kept_weight_bytes(model, 5, torch.bfloat16) >= 5 * plan.mean_weight_bytes(model, torch.bfloat16)
    with pytest.raises(ValueError, match="dtype"):
        plan.mean_weight_bytes(model, torch.int8)


def test_sample_generate_speculative_refusals():
    from bayeformers_amd import ops
    from bayeformers_amd.sampling import Generation, sample_generate

    model = _small_llama()
    ids = torch.zeros(2, 4, dtype=torch.long)
    kw = dict(samples=2, max_new_tokens=4, keep_weights=True)
    with torch.no_grad():
        for bad in (0, -1, ops.DECODE_MAX_QUERIES, 2.0, True, "3"):
            with pytest.raises(ValueError, match="speculative"):
                sample_generate(model, ids, speculative=bad, **kw)
        with pytest.raises(ValueError, match=r"B \* \(γ \+ 1\)"):  # 2 rows of 8 + 1 positions
            sample_generate(model, ids, speculative=8, **kw)
        with pytest.raises(ValueError, match=r"B \* \(γ \+ 1\)"):
            sample_generate(model, torch.zeros(9, 4, dtype=torch.long), speculative=1, **kw)
        for keep in (False, None):
            with pytest.raises(ValueError, match="keep_weights"):
                sample_generate(model, ids, speculative=3, **dict(kw, keep_weights=keep))
        with pytest.raises(ValueError, match="greedy"):
            sample_generate(model, ids, speculative=3, do_sample=True, **kw)
        for name, v in (("top_k", 5), ("top_p", 0.9), ("min_p", 0.1)):
            for do_sample in (False, True):
                with pytest.raises(ValueError, match="speculative"):
                    sample_generate(model, ids, speculative=3, do_sample=do_sample, **{name: v}, **kw)
        for name, v in (("repetition_penalty", 1.2), ("no_repeat_ngram_size", 2), ("min_new_tokens", 2)):
            with pytest.raises(ValueError, match="earlier positions"):
                sample_generate(model, ids, speculative=3, eos_token_id=1, **{name: v}, **kw)
        with pytest.raises(ValueError, match="ring"):
            sample_generate(model, ids, speculative=3, sliding_cache="ring", **kw)
        with pytest.raises(ValueError, match="single process"):
            sample_generate(model, ids, speculative=3, group=object(), **kw)
    assert Generation(*[torch.zeros(1)] * 8).speculation is None


def test_speculative_refuses_layers_without_a_mean_form():
    import bayeformers_amd as bf
    import bayeformers_amd.nn as bnn
    from bayeformers_amd.sampling import sample_generate

    model = _small_llama()
    ids = torch.zeros(1, 4, dtype=torch.long)
    inner = model.model
    emb = inner.get_input_embeddings()
    inner.set_input_embeddings(bnn.Embedding(emb.num_embeddings, emb.embedding_dim))
    model.refresh()
    with torch.no_grad():
        with pytest.raises(ValueError, match="Embedding"):
            sample_generate(model, ids, samples=2, max_new_tokens=3, keep_weights=True, speculative=2)
        with pytest.raises(ValueError, match="Embedding"):
            with model.posterior_mean():
                pass
    lora = bf.to_bayesian_lora(_small_llama_plain(), r=4).eval()
    with torch.no_grad(), pytest.raises(ValueError, match="LoRALinear"):
        sample_generate(lora, ids, samples=2, max_new_tokens=3, keep_weights=True, speculative=2)


def _small_llama_plain():
    from transformers import LlamaConfig, LlamaForCausalLM

    cfg = LlamaConfig(hidden_size=64, num_attention_heads=4, num_key_value_heads=2, num_hidden_layers=1,
                      intermediate_size=128, vocab_size=96, max_position_embeddings=64, tie_word_embeddings=False)
    torch.manual_seed(0)
    return LlamaForCausalLM(cfg).eval()
