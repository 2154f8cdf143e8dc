"""Every model's contract in front of the first launch, against tests/golden/model_contract.json (tests/model_contract_cases.py:
recorded from the commit in front of the model table, csrc/kge_models.hpp and dglke_amd/models.py): which ids and widths each C
entry takes and the text it refuses the others with, the byte layout of every workspace for each model, and what the command lines
say to each flag combination.  No device: every call is refused before a launch or only measures."""
import json
import os
import sys

import pytest

import model_contract_cases as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dgl-ke_amd"))


@pytest.fixture(scope="module")
def golden():
    with open(M.FIXTURE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def now():
    import __graft_entry__
    __graft_entry__.build()
    from dglke_amd import _lib as L
    return M.collect_c(L.lib(), L)


def _text(rec, a):
    return None if a < 0 else rec["answers"][a]


def test_the_fixture_covers_the_grid_and_holds_refusals_only(golden):
    assert golden["grid"] == M.grid()
    assert M.MODEL_GRID == list(range(-1, 17)) + [99] and len(M.DIMS) == 9 and len(M.NAMES) == 13
    M.check_refusals(golden)
    cells = len(M.MODEL_GRID) * len(M.DIMS)
    assert len(golden["null"]) == 21 and all(len(rows) == cells for rows in golden["null"].values())
    assert len(golden["short"]) == 7 and all(len(rows) == 26 for rows in golden["short"].values())
    assert len(golden["sizes"]) == 8 and all(len(rows) == 26 for rows in golden["sizes"].values())
    assert {row[0] for row in golden["topk_dims"]} == {0, 1, 2, 3, 4, 5, 6, 8, 10, 12, 14}
    assert os.path.getsize(M.FIXTURE) < (1 << 20)


def test_every_entry_refuses_what_it_refused_with_the_same_words(golden, now):
    assert sorted(now["null"]) == sorted(golden["null"])
    cells = [(m, d) for m in M.MODEL_GRID for d in M.DIMS]
    for entry, rows in golden["null"].items():
        for cell, want, got in zip(cells, rows, now["null"][entry]):
            assert _text(now, got) == _text(golden, want), (entry, cell)
    assert [r[:3] + _text(now, r[3]) for r in now["topk_dims"]] == [r[:3] + _text(golden, r[3]) for r in golden["topk_dims"]]


def test_a_workspace_one_byte_short_is_refused_with_the_same_words(golden, now):
    assert sorted(now["short"]) == sorted(golden["short"])
    cells = [(n, s) for n in M.NAMES for s in M.SHAPES]
    for entry, rows in golden["short"].items():
        for cell, want, got in zip(cells, rows, now["short"][entry]):
            assert _text(now, got) == _text(golden, want), (entry, cell)


def test_every_workspace_keeps_its_layout_entry_by_entry(golden, now):
    assert sorted(now["sizes"]) == sorted(golden["sizes"])
    cells = [(n, s) for n in M.NAMES for s in M.SHAPES]
    for fn, rows in golden["sizes"].items():
        for cell, want, got in zip(cells, rows, now["sizes"][fn]):
            assert got == want, (fn, cell)
    assert now["rel_sizes"] == golden["rel_sizes"]


def test_the_command_lines_say_the_same_to_every_flag_combination(golden, now):
    py = M.collect_python()
    for section in ("widths", "train", "eval"):
        assert len(py[section]) == len(golden["python"][section])
    cells = [c for c in M.flag_grid()]
    for cell, want, got in zip(cells, golden["python"]["train"], py["train"]):
        assert _text(py, got) == _text(golden["python"], want), ("train", cell)
    for cell, want, got in zip([c for c in cells if not c[5]], golden["python"]["eval"], py["eval"]):
        assert _text(py, got) == _text(golden["python"], want), ("eval", cell)
    assert [_text(py, a) for a in py["widths"]] == [_text(golden["python"], a) for a in golden["python"]["widths"]]
