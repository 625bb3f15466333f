"""The host side of the grouped weight-gradient launch decides what it decided before it was split into named pieces
(csrc/conv_wgrad_plan.hip): tests/golden/wgrad_layout_parent.npz holds the plan's (kind, splits) pairs, every unit-table row and every
refusal of twelve problem lists at six dealing modes, written on the commit before by tests/golden/gen_wgrad_layout_parent.py. This test
records them again with the library under test and compares entry by entry. No GPU, no tolerance."""
import importlib.util
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def _generator():
    spec = importlib.util.spec_from_file_location("gen_wgrad_layout_parent", os.path.join(GOLDEN, "gen_wgrad_layout_parent.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def both():
    gold = np.load(os.path.join(GOLDEN, "wgrad_layout_parent.npz"))          # plain arrays: no pickle
    return {k: gold[k] for k in gold.files}, _generator().record()


def test_same_entries(both):
    gold, got = both
    assert sorted(gold) == sorted(got)
    assert sum(k.startswith("rows:") for k in gold) == 12 * 6 and sum(k.startswith("plan:") for k in gold) == 12


def test_plan_pairs_are_the_parents(both):
    gold, got = both
    for k in gold:
        if k.startswith("plan:"):
            assert np.array_equal(got[k], gold[k]), k


def test_unit_tables_are_the_parents(both):
    gold, got = both
    for k in gold:
        if k.startswith("rows:"):
            assert got[k].shape == gold[k].shape and np.array_equal(got[k], gold[k]), k


def test_refusals_are_the_parents(both):
    gold, got = both
    assert len(gold["refusal_names"]) == 9
    for k in ("refusal_names", "refusal_status", "refusal_messages"):
        assert gold[k].tolist() == got[k].tolist(), k
