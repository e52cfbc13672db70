"""CPU: the numpy rules of the PUCT player answer what they answered before they were restated as one search with options
(tests/puct_search_rule.py).  tests/golden/puct_rules_parent.npz was written once by tests/golden/make_golden_puct_rules.py
from the rule modules of the commit before the restatement; here the same script computes every entry again from the
rules of this tree -- through the cases modules' cached references, so that in one process with the other tests it costs
little beyond them -- and every array must equal the stored one: no tolerance, no entry left out.  The stored SHA-256 of
the leaves an evaluator saw pins the selections, which the outputs alone do not.

With it the comparisons that now hold a class against itself (``SolverPuct(solver=False)`` and ``LeavesPuct``,
``FpuPuct(fpu=None)`` and ``SolverPuct``, ``ForcedPuct(forced=None)`` and ``FpuPuct``) are held against the classes as they
were: the entries "built_on/..." are both sides of each, on the inputs of those tests."""
import importlib.util
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def make():
    spec = importlib.util.spec_from_file_location("make_puct_rules", os.path.join(GOLDEN, "make_golden_puct_rules.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


@pytest.fixture(scope="module")
def stored(make):
    with np.load(make.OUT) as z:
        return make.unpack({name: z[name] for name in z.files})


GROUPS = ("leaves", "solver", "forced", "near_tie", "per_row", "built_on", "cross")


@pytest.mark.parametrize("group", GROUPS)
def test_the_rules_answer_what_they_answered_before_the_restatement(make, stored, group):
    (entries,) = [g for g in make.GROUPS if g.__name__ == group + "_entries"]
    prefixes, seen = set(), 0
    for key, entry in entries():
        prefixes.add(key.split("/")[0])
        for field, value in entry.items():
            want, value = stored[f"{key}/{field}"], np.asarray(value)
            assert value.dtype == want.dtype and value.shape == want.shape and np.array_equal(value, want), (key, field)
            seen += 1
        assert {name for name in stored if name.startswith(key + "/")} == {f"{key}/{field}" for field in entry}, key
    assert seen == sum(1 for name in stored if name.split("/")[0] in prefixes) > 0  # no stored array was left out


def test_the_file_holds_nothing_but_the_groups_and_stays_small(make, stored):
    assert len(GROUPS) == len(make.GROUPS)
    assert {name.split("/")[0] for name in stored} == {"leaves", "solver", "forced", "near_tie", "async_fpu", "async_keep",
                                                       "built_on", "cross"}
    assert os.path.getsize(make.OUT) < 500 * 1024
    # both sides of every comparison that became a class against itself, and every option against every other
    for side in ("solver_off-3x3x3-1", "first_rule-0", "solver_off_one_leaf-0", "kept-reuse-3x3x3-0", "kept-solver_off-3x3x3-0",
                 "solver-9x9x5-4-True", "fpu_none-9x9x5-4-True", "fpu-9x9x5-4-True", "forced_none-9x9x5-4-True"):
        assert f"built_on/{side}/leaves" in stored, side
    assert sum(1 for name in stored if name.startswith("cross/") and name.endswith("/leaves")) == 2 * 2 * 2 * 2 * 3 * 2 * 3
