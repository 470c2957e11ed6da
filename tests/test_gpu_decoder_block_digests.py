"""The twelve decoder-block wrappers return the recorded bits.

tests/golden/decoder_block_digests.json holds one SHA-256 per group of calls, recorded on an MI355X by
tests/golden/make_decoder_block_digests.py (its docstring describes the grid and how a group's digest is formed).  This
test replays each group and compares.  A digest that differs means the arithmetic, a rounding or the order of a sum
changed: `make_decoder_block_digests.py --list` on the two builds shows which call."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

with open(os.path.join(GOLDEN, "decoder_block_digests.json")) as _f:
    RECORDED = json.load(_f)


@pytest.fixture(scope="module")
def maker():
    spec = importlib.util.spec_from_file_location("make_decoder_block_digests",
                                                  os.path.join(GOLDEN, "make_decoder_block_digests.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def test_the_table_lists_every_group_cpu(maker):
    assert [name for name, _ in maker.groups()] == list(RECORDED)


@pytest.mark.gpu
@pytest.mark.parametrize("group", list(RECORDED))
def test_group_reproduces_its_digest(maker, group):
    calls = dict(maker.groups())[group]
    assert maker.digest(calls()) == RECORDED[group], f"{group}: the results' bits differ from the recorded ones"
