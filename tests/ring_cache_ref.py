"""Pure-Python restatement of the ring-buffer KV cache's placement (include/bayeformers_amd_ring.h), shared by the CPU and
the GPU tests of sliding_cache="ring": the key with sequence index j lives in slot j % C."""


def placement(fill, T, C):
    """{slot: source row} after appending rows 0 .. T - 1 at fill `fill` to a ring of C slots, one row after the other: row
    i is bound for slot (fill + i) % C and a later row overwrites an earlier one's slot.  Slots not in the dict are not
    addressed by the call."""
    assert fill >= 0 and T >= 1 and C >= 1
    slots = {}
    for i in range(T):
        slots[(fill + i) % C] = i
    return slots


def written_rows(T, C):
    """The rows a single launch writes so that no slot is written twice: the last min(T, C)."""
    return list(range(max(0, T - C), T))


def live_keys(L, C):
    """The sequence indices a ring of C slots holds at fill L, and the slot of each."""
    return {j: j % C for j in range(max(0, L - C), L)}


def visible_span(L, Tq, W):
    """[lo, hi): the keys some query of a step sees whose Tq rows were appended at fill L - Tq (the fill is L after it)."""
    return max(0, L - Tq - W + 1), L
