"""The attention interface routes every call of the recorded grid where it always did (no GPU).

tests/golden/attention_routes.json is the route table recorded by tests/golden/make_attention_routes.py (its docstring
describes the grid, the recorders and what was pruned).  This test replays the same grid and compares each case's
outcome — the entry reached, its non-tensor arguments, which optional tensors were passed, or the exception — with the
table.  The table is regenerated only when a route is meant to change."""
import importlib.util
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _generator():
    spec = importlib.util.spec_from_file_location("make_attention_routes", os.path.join(GOLDEN, "make_attention_routes.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def test_every_call_of_the_grid_takes_its_recorded_route():
    gen = _generator()
    with open(gen.JSON_PATH) as f:
        table = json.load(f)
    cases = list(gen.cases())
    assert table["axes"] == list(gen.AXES) and table["cases"] == len(cases) == len(table["rows"])
    outcomes, rows = gen.replay()
    assert len(rows) == len(cases)
    wrong = [(case, table["outcomes"][want], outcomes[got])
             for case, want, got in zip(cases, table["rows"], rows) if table["outcomes"][want] != outcomes[got]]
    shown = "\n".join(f"{case}\n  recorded: {want}\n  now:      {got}" for case, want, got in wrong[:10])
    assert not wrong, f"{len(wrong)} of {len(cases)} calls changed their route; the first:\n{shown}"
