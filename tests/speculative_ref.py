"""bf_spec_accept's contract (include/bayeformers_amd_spec.h) restated in plain torch, on tensors of any device: the epilogue of
one speculative iteration of sample_generate(speculative=γ).  Same arguments as ops.speculative_accept, updated in place."""
import torch


def speculative_accept(argmax, draft, probs, predictive_entropy, expected_entropy, mutual_information, samples, state,
                       sequences, T0, stats, finished, lengths, verify_ids, verify_positions, draft_ids, draft_positions,
                       rewind, speculation, eos_token_id, pad_token_id):
    B, G = draft.shape
    V = probs.shape[1]
    n = stats.shape[-1]
    S = int(samples)
    step = int(state[0])
    if step >= n:  # past the last token: the iteration's forwards still moved both fills by γ + 1
        rewind[0] = G + 1
        return
    eos = eos_token_id
    live = [b for b in range(B) if not (eos is not None and bool(finished[b]))]
    room = min(G, n - step - 1)
    a = room
    for b in live:
        run = 0
        while run < G and int(draft[b, run]) == int(argmax[b, run]):
            run += 1
        a = min(a, run)
    entropies = (predictive_entropy, expected_entropy, mutual_information)
    for b in range(B):
        done = eos is not None and bool(finished[b])
        tok = int(verify_ids[b, 0])
        for j in range(a + 1):
            r = b * (G + 1) + j
            before = tok
            tok = int(pad_token_id) if done else int(draft[b, j] if j < a else argmax[b, a])
            for i in range(3):
                stats[i, b, step + j] = 0.0 if done else entropies[i][r]
            stats[3, b, step + j] = 0.0 if done or not 0 <= tok < V else probs[r, tok]
            sequences[b, T0 + step + j] = tok
            if not done:
                lengths[b] += 1
            if eos is not None:
                done = done or tok == int(eos)
        if eos is not None:
            finished[b] = done
        draft_ids[b, 0], draft_ids[b, 1] = before, tok
        verify_ids.view(S, B, G + 1)[:, b, 0] = tok
    if verify_positions is not None:
        verify_positions += a + 1
    if draft_positions is not None:
        draft_positions += a + 1
    state[0] = step + a + 1
    rewind[0] = G - a
    speculation += torch.tensor([1, room, a], dtype=speculation.dtype, device=speculation.device)


def greedy_replay(table, step, n, n_steps, finished, eos_token_id, pad_token_id):
    """The naive loop the contract must agree with: sequential greedy decoding of every row for `n_steps` tokens from step
    `step`, reading each row's next token from `table` [B, n_steps] (the argmax at each of its positions).  Returns
    (tokens [B, n_steps], lengths added [B], finished [B])."""
    B = table.shape[0]
    toks = torch.full((B, n_steps), int(pad_token_id), dtype=torch.long)
    added = torch.zeros(B, dtype=torch.long)
    fin = finished.clone()
    for j in range(n_steps):
        for b in range(B):
            if eos_token_id is not None and bool(fin[b]):
                continue
            toks[b, j] = table[b, j]
            added[b] += 1
            if eos_token_id is not None and int(table[b, j]) == int(eos_token_id):
                fin[b] = True
    return toks, added, fin


# ---- the hand-built cases of the CPU and the GPU test: B 3, γ 4, V 37, n 9 ---------------------------------------------
B, G, V, N_NEW, T0, S, EOS, PAD = 3, 4, 37, 9, 6, 2, 5, 36


def hand_cases():
    """name -> (arguments of speculative_accept as CPU tensors, the expected run length a; None: a no-op launch)."""
    g = torch.Generator().manual_seed(1234)
    out = {}

    def case(name, runs, step=2, finished=(False, False, False), eos=EOS, eos_at=None, expect=None):
        # (tokens 6 .. 35: never EOS or PAD by chance)
        argmax = torch.randint(6, 36, (B, G + 1), generator=g)
        if eos_at is not None:
            argmax[eos_at[0], eos_at[1]] = EOS
        draft = argmax[:, :G].clone()
        for b, run in enumerate(runs):
            if run < G:
                draft[b, run] = (draft[b, run] + 1 - 6) % 30 + 6  # the first disagreement; later drafts stay equal
        probs = torch.softmax(torch.randn(B * (G + 1), V, generator=g), -1)
        ent = [torch.rand(B * (G + 1), generator=g) for _ in range(3)]
        sequences = torch.full((B, T0 + N_NEW), -5, dtype=torch.long)
        last = torch.randint(6, 36, (B,), generator=g)
        verify_ids = torch.full((S * B, G + 1), -7, dtype=torch.long)
        verify_ids[:, 0] = last.repeat(S)
        pos = torch.tensor([T0 + step - 1, T0 + step - 3, T0 + step - 2])  # (row 1 and 2 left-padded)
        steps = torch.arange(G + 1)
        fin = torch.tensor(finished)
        args = dict(argmax=argmax, draft=draft, probs=probs, predictive_entropy=ent[0], expected_entropy=ent[1],
                    mutual_information=ent[2], samples=S, state=torch.tensor([step, 0]), sequences=sequences, T0=T0,
                    stats=torch.full((4, B, N_NEW), -1.0), finished=fin if eos is not None else None,
                    lengths=torch.where(fin, 1, step), verify_ids=verify_ids,
                    verify_positions=(pos[:, None] + steps[None, :]).repeat(S, 1),
                    draft_ids=torch.full((B, 2), -9, dtype=torch.long),
                    draft_positions=pos[:, None] - 1 + steps[None, :], rewind=torch.tensor([-1]),
                    speculation=torch.tensor([3, 10, 4]), eos_token_id=eos, pad_token_id=PAD)
        out[name] = (args, expect)

    case("nothing_accepted", (0, 4, 2), expect=0)
    case("everything_accepted", (4, 4, 4), expect=4)
    case("minimum_rules", (3, 1, 2), expect=1)
    case("no_eos_token", (2, 3, 4), eos=None, expect=2)
    case("finished_row_is_not_counted", (2, 0, 3), finished=(False, True, False), expect=2)
    case("eos_inside_the_accepted_span", (3, 4, 3), eos_at=(0, 1), expect=3)
    case("eos_as_the_correction", (1, 4, 1), eos_at=(2, 1), expect=1)
    case("every_row_finished", (0, 1, 0), finished=(True, True, True), expect=4)
    case("clipped_before_n", (4, 4, 4), step=7, expect=1)
    case("last_token", (4, 4, 4), step=8, expect=0)
    case("past_n_is_a_no_op", (4, 4, 4), step=9, expect=None)
    return out


def clone_args(args, device="cpu"):
    return {k: (v.clone().to(device) if isinstance(v, torch.Tensor) else v) for k, v in args.items()}
