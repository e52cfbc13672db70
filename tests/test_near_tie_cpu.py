"""CPU: why the near-tie cases exist, shown with the numpy rules alone.

Every PUCT form claims to equal its rule bit for bit, and include/mnk_hip.h states the rule down to the single float32
rounding.  The evaluators of the older tests are dyadic, and on them most of those roundings round nothing.  This file
plants, into the rules (through tests/puct_ops.py), the departures a kernel could plausibly have --

    assoc          the exploration term as c * (p * sq) in the place of (c * p) * sq
    f64_score      the score evaluated in float64 and rounded once
    sqrt_low       the square root one ulp low for a third of its arguments
    reversed       the backups of a round taken in reverse slot order
    fpu_fused      q_v - r * mass with the product left unrounded
    forcing_assoc  the forcing test against k * (P * S')
    floor_assoc    the pruning's floor from k * (P * (n_0 - 1))

-- and asserts (1) that the evaluator of tests/near_tie_evaluator.py is the same function, bit for bit, in numpy and in
torch, for every leaf and output dtype; (2) that every planted defect but the two reassociated bounds (which no table
can show: 2b) changes the answer of every case of tests/near_tie_cases.py it applies to, one pair on 19x19x5 excepted
(OUT_OF_REACH, with the reason and 2c) -- a condition on the cases: where one did not meet it, another ``ulps`` or table seed was
searched for with ``PYTHONPATH=. python tests/test_near_tie_cpu.py`` and written into the case table; (3) that under the dyadic
evaluator and constants of the older tests none of them changes anything; (4) that the per-row cases end a game, record
fast and full plies and notice the first of the defects."""
import functools

import numpy as np
import pytest
import torch

import near_tie_cases as cases
import puct_ops
from near_tie_evaluator import near_np, near_torch
from tactical_rule import random_positions

f32, f64 = np.float32, np.float64


# ----------------------------------------------------------------------------- the planted defects
def _assoc(q, c, prior, sq, na):
    u = c * (prior * sq) / (1 + na).astype(f32)
    return (q + u.astype(f32)).astype(f32)


def _f64_score(q, c, prior, sq, na):
    return (q.astype(f64) + f64(c) * prior.astype(f64) * f64(sq) / (1 + na).astype(f64)).astype(f32)


def _sqrt_low(x):
    """one ulp low for the arguments with n % 3 == 1"""
    r = np.sqrt(f32(x))
    return np.nextafter(r, f32(0)) if int(x) % 3 == 1 else r


def _sqrt_low_off_squares(x):
    """the same, but right on the perfect squares, as a square root made of an approximate reciprocal root and a
    correction step is.  Section 3 plants this one: the one above, low at 1, 4, 16, ... as well, does show under the dyadic
    inputs, on 2 of their 36 cases (4x6x3 "forced" and "gumbel")"""
    r = np.sqrt(f32(x))
    return r if int(round(float(r))) ** 2 == int(x) else _sqrt_low(x)


def _reversed(L):
    return range(L - 1, -1, -1)


def _fpu_fused(qv, r, mass):
    return f32(f64(qv) - f64(r) * f64(mass))


def _bound_assoc(k_forced, prior, S):
    return f32(f32(k_forced) * f32(prior * S))


#           name            the operation of puct_ops, what stands in for it, the forms it applies to
DEFECTS = {"assoc": ("score", _assoc, cases.FORMS),
           "f64_score": ("score", _f64_score, cases.FORMS),
           "sqrt_low": ("sqrt", _sqrt_low, cases.FORMS),
           "reversed": ("backup_order", _reversed, ("leaves", "all")),
           "fpu_fused": ("fpu_q", _fpu_fused, ("fpu", "all")),
           "forcing_assoc": ("forcing_bound", _bound_assoc, ("forced", "all")),
           "floor_assoc": ("floor_bound", _bound_assoc, ("forced", "all"))}
# the two reassociated bounds are compared with the square of an integer, so an ulp more or less shows only where k * P * S'
# lies within an ulp or two of a perfect square: with k = 1.7 and P within a few ulps of 1 / C it never does (17 S' = 10 C n^2
# has no solution at these budgets), whatever ``ulps`` or table seed -- test 2b below asserts that, in the place of 2
BOUNDS = ("forcing_assoc", "floor_assoc")
# and one pair no table reaches (ulps 2, 4, 8 times the seeds 0 .. 79 were tried): on 19x19x5 Sequential Halving over four
# cells gives no node below the root more than six visits, and the Gumbel root itself takes no square root.  Of 1 .. 6 the low
# root touches 1 and 4: the root of a node with one visit scales the scores of children that are all unvisited, with q = 0,
# by one factor, which keeps their order; that leaves the nodes of four visits, a handful in 48 simulations.  Test 2c
# asserts the six visits.  The low root is noticed on this board by the eight other forms
OUT_OF_REACH = {("19x19x5", "gumbel", "sqrt_low")}
PLANTED = [(name, form, defect) for name, form in cases.LOCKSTEP for defect, (_, _, forms) in DEFECTS.items()
           if form in forms and defect not in BOUNDS and (name, form, defect) not in OUT_OF_REACH]


def planted(monkeypatch, defect):
    op, stand_in, _ = DEFECTS[defect]
    monkeypatch.setattr(puct_ops, op, stand_in)


# ----------------------------------------------------------------------------- 1. one evaluator, the same bits on both sides
@functools.lru_cache(maxsize=None)
def many_positions(name):
    (m, n, k), _, _, _, _ = cases.BOARDS[name]
    return random_positions(m, n, k, 300, np.random.default_rng(m * n), max_fill=0.9)


@pytest.mark.parametrize("bf16,out_dtype", [(False, torch.float32), (True, torch.bfloat16), (True, torch.float32)])
@pytest.mark.parametrize("leaf_dtype", [torch.float32, torch.bfloat16, torch.uint8])
@pytest.mark.parametrize("name", list(cases.BOARDS))
def test_numpy_and_torch_evaluate_the_same_bits(name, leaf_dtype, bf16, out_dtype):
    (m, n, k), _, _, ulps, seed = cases.BOARDS[name]
    C = m * n
    obs = many_positions(name)
    mask = (obs.reshape(len(obs), 2, C) == 0).all(axis=1)
    mask[::7] &= np.random.default_rng(1).random((len(mask[::7]), C)) < 0.5  # (a mask of its own: the product is the mask's)
    priors, values = near_np(C, ulps, seed, bf16)(obs, mask)
    got_p, got_v = near_torch(C, ulps, seed, out_dtype, bf16=bf16)(torch.from_numpy(obs).to(leaf_dtype),
                                                                  torch.from_numpy(mask))
    assert got_p.dtype == out_dtype and got_v.dtype == out_dtype
    assert np.array_equal(got_p.float().numpy().view(np.uint32), priors.view(np.uint32))
    assert np.array_equal(got_v.float().numpy().view(np.uint32), values.view(np.uint32))
    # the inputs are what they are meant to be: within ``ulps`` of 1 / C and of a level, and no two the same everywhere
    step = 1 << 16 if bf16 else 1
    base = int(f32(1.0 / C).view(np.uint32)) & (0xFFFF0000 if bf16 else 0xFFFFFFFF)
    off = (priors[mask].view(np.uint32).astype(np.int64) - base) // step
    assert off.min() == 0 and off.max() == ulps and (priors[~mask] == 0).all()
    assert len(np.unique(values)) > 4 and np.abs(np.abs(values) - 0.2).max() < 0.11


# ----------------------------------------------------------------------------- 2. every defect is caught on every case
@pytest.mark.parametrize("name,form,defect", PLANTED)
def test_a_planted_defect_changes_the_answer_of_the_case(name, form, defect, monkeypatch):
    tables = cases.tables_of(name, form)
    want = [cases.reference(name, form, table) for table in tables]
    planted(monkeypatch, defect)
    assert any(cases.differs(cases.run(name, form, table=table), w) for table, w in zip(tables, want)), (name, form, defect)


@pytest.mark.parametrize("name", list(cases.BOARDS))
def test_no_choice_of_table_lets_a_reassociated_bound_show(name):
    """2b: for every prior a table of this board can hold (0 .. 8 ulps above 1 / C), every S' up to four times the budget
    and every integer n', the rule's bound and the reassociated one lie on the same side of n'^2.  (The noised priors of
    the "all" form are no table values; there a bound within two ulps of a square would be an accident of one in millions.)"""
    (m, n, _), _, I, _, _ = cases.BOARDS[name]
    S = np.arange(1, 4 * I + 1).astype(f32)
    squares = (np.arange(0, 4 * I + 1) ** 2).astype(f32)[:, None]
    for off in range(9):
        P = (f32(1.0 / (m * n)).view(np.uint32) + np.uint32(off)).view(f32)
        rule = np.array([puct_ops.forcing_bound(cases.K_FORCED, P, s) for s in S])
        other = np.array([_bound_assoc(cases.K_FORCED, P, s) for s in S])
        assert np.array_equal(rule, np.array([puct_ops.floor_bound(cases.K_FORCED, P, s) for s in S]))
        assert (rule != other).any() or off  # (the two do differ: it is the comparison that cannot see it)
        assert np.array_equal(squares < rule, squares < other) and np.array_equal(squares >= rule, squares >= other)


def test_the_gumbel_root_on_19x19x5_takes_the_square_root_of_no_count_above_six(monkeypatch):
    """2c: every argument of the square root in that case is at most 6; the low root differs from the right one at 1 and 4
    alone, and the one that is right on the perfect squares at none of them"""
    asked, sqrt = set(), puct_ops.sqrt
    monkeypatch.setattr(puct_ops, "sqrt", lambda x: (asked.add(int(x)), sqrt(x))[1])
    cases.run("19x19x5", "gumbel")
    assert asked and max(asked) <= 6, sorted(asked)
    assert {x for x in asked if _sqrt_low(x) != sqrt(x)} <= {1, 4}
    assert all(_sqrt_low_off_squares(x) == sqrt(x) for x in asked)


# ----------------------------------------------------------------------------- 3. and was not under the older inputs
@pytest.mark.parametrize("defect", list(DEFECTS))
def test_under_the_dyadic_inputs_of_the_older_tests_the_defect_changes_nothing(defect, monkeypatch):
    """(the low square root in the form that is right on the perfect squares: see ``_sqrt_low_off_squares``)"""
    forms = DEFECTS[defect][2]
    want = {(name, form): cases.run(name, form, today=True) for name in cases.BOARDS for form in forms}
    planted(monkeypatch, defect)
    if defect == "sqrt_low":
        monkeypatch.setattr(puct_ops, "sqrt", _sqrt_low_off_squares)
    changed = [key for key in want if cases.differs(cases.run(*key, today=True), want[key])]
    assert not changed, (defect, changed)


# ----------------------------------------------------------------------------- 4. the per-row cases
@pytest.mark.parametrize("name,form", cases.ASYNC)
def test_a_per_row_case_ends_a_game_and_records_fast_and_full_plies(name, form):
    rule = cases.async_run(name, form)[0]
    assert not rule.errors and rule.N % 4
    assert rule.stats[0] > 0 and rule.fast_records > 0 and rule.full_records > 0
    assert len(set(rule.row_plies.tolist())) > 1  # the rows are out of step


@pytest.mark.parametrize("name,form", [case for case in cases.ASYNC if case[0] == "3x3x3"])
def test_a_per_row_case_notices_the_reassociated_exploration_term(name, form, monkeypatch):
    """(on 3x3x3: eight iterations over the 81 near-equal priors of 9x9x5 visit too few children twice for the plain
    kernel's case to notice; that board is there for the shape of the code, the lockstep cases for the roundings)"""
    want = cases.async_run(name, form)[1]
    planted(monkeypatch, "assoc")
    got = cases.async_run.__wrapped__(name, form)[1]
    assert any(not np.array_equal(g, w) for g, w in zip(got, want)), (name, form)


# ----------------------------------------------------------------------------- the search behind the case table
def search():
    """for every lockstep case: the board's own (ulps, table seed), else the first of the seeds 0 .. 79 times ulps 2, 4, 8
    that lets no defect through, as a line of ``near_tie_cases.CHOICE``; where there is none, the defects each choice that
    shows the most of them leaves (the case then takes a second table: ``near_tie_cases.SECOND``)"""
    import unittest.mock

    for name, form in cases.LOCKSTEP:
        todo = [d for d, (_, _, forms) in DEFECTS.items() if (name, form, d) in PLANTED]
        least = None
        for ulps, seed in [cases.BOARDS[name][3:]] + [(u, s) for s in range(80) for u in (2, 4, 8)]:
            want, missed = cases.run(name, form, table=(ulps, seed)), []
            for d in todo:
                with unittest.mock.patch.object(puct_ops, DEFECTS[d][0], DEFECTS[d][1]):
                    if not cases.differs(cases.run(name, form, table=(ulps, seed)), want):
                        missed.append(d)
            if least is None or len(missed) < len(least[1]):
                least = ((ulps, seed), missed)
            if not missed:
                break
        print(f'    ("{name}", "{form}"): {least[0]},' + (f"  # MISSED {least[1]}" if least[1] else ""), flush=True)


if __name__ == "__main__":
    search()
