"""CPU: per-row search self-play with a Gumbel root -- the C ABI of ``mnk_search_selfplay_advance_gumbel`` (header,
export, binding, the host's argument checks, which reject before anything is enqueued), the argument checks of
``AsyncSearchSelfPlay(gumbel=...)``, the numpy restatement in tests/search_selfplay_async_gumbel_rule.py against the
lockstep composition (``gumbel_puct`` -> ``GumbelSelfPlayRule.step_moves``) with every ply full, and the seeds and shapes
of tests/test_gpu_search_selfplay_async_gumbel.py: with them the rule reaches every branch of the kernel."""
import functools
import re

import numpy as np
import pytest

from oracle.packing import record_words
from player_cases import HEADER, check_header_and_binding, lib  # noqa: F401 (lib: the fixture)
from puct_gumbel_rule import GumbelSelfPlayRule, gumbel_puct, schedule
from search_selfplay_async_gumbel_rule import AsyncGumbelRule
from search_selfplay_async_keep_cases import start_state
from search_selfplay_async_rule import exact_np

# what the GPU tests share with this file: the mixed budgets (a fast budget below `considered`: the fast table's rows are
# a truncated first round of Sequential Halving), the row id of row 0, and the cases: board, rows, rounds, seed, start
# ("golden": a stored env state near the end of games, tests/golden/search_selfplay_async_starts.npz), and what only the
# device reads -- leaf dtype, dtype of priors and values, device key word.  The first three are indexed below; the others
# put the entry point on every kind of board it is compiled for: 12x13x5, 16x15x5 (C = 240: the plane fills its last word)
# and 19x19x5 (C = 361: no multiple of four, so the draw's row stride is not C, and six trips of a per-cell loop) are
# siblings of or the built-in variants <6,13,5>, <8,15,5> and <12,19,5>, 12x12x5 is the generic form of five words and
# 7x7x4 that of two, from the empty board for more than a lap of its ring.  The rule gives (games, full / fast records,
# row plies) in test_every_case_records_fast_and_full_plies_and_leaves_the_rows_out_of_step's output.
FULL, FAST, CONSIDERED, THRESHOLD, ENV_ID0 = 8, 3, 4, 2 ** 31, 3
MIXED_CASES = [
    ((3, 3, 3), 7, 130, 6, None, "float32", "float32", False),
    ((4, 6, 3), 5, 200, 6, None, "float32", "float32", False),
    ((9, 9, 5), 5, 150, 6, None, "float32", "bfloat16", False),
    ((12, 13, 5), 5, 150, 6, "golden", "bfloat16", "float32", False),
    ((16, 15, 5), 5, 150, 6, "golden", "float32", "bfloat16", False),
    ((19, 19, 5), 3, 150, 6, "golden", "uint8", "float32", False),
    ((12, 12, 5), 3, 150, 6, "golden", "float32", "float32", True),
    ((7, 7, 4), 5, 500, 6, None, "uint8", "bfloat16", True),
    # the generic forms of sixteen and of thirty-two words (ten and 21 words a plane; C = 289 and 625: the draw's row
    # stride is not C), from a computed start ("late": five rows three to eight stones short of a drawn board)
    ((17, 17, 5), 5, 150, 6, "late", "uint8", "float32", False),
    ((25, 25, 5), 5, 150, 6, "late", "bfloat16", "bfloat16", True),
]


# ----------------------------------------------------------------------------- a. the entry point
def _params(name):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert decl, name
    return [" ".join(a.split()) for a in decl.group(1).split(",") if a.strip()]


def test_the_header_declares_the_entry_point_and_the_binding_has_it(lib):
    check_header_and_binding(lib, "mnk_search_selfplay_advance_gumbel")
    old, new = _params("mnk_search_selfplay_advance"), _params("mnk_search_selfplay_advance_gumbel")
    # every argument of the plain entry point up to err but temp_plies, the Gumbel root's, the stream
    assert "int temp_plies" in old
    assert new == [a for a in old[:-1] if a != "int temp_plies"] + [
        "int considered", "float c_visit", "float c_scale", "float gumbel_scale", "const uint16_t* table_full",
        "const uint16_t* table_fast", "float* gscore", "float* vroot", "void* stream"]
    sig = lib.SIGNATURES
    at = old.index("int temp_plies")
    assert sig["mnk_search_selfplay_advance_gumbel"][:len(old) - 2] == (sig["mnk_search_selfplay_advance"][:at] +
                                                                        sig["mnk_search_selfplay_advance"][at + 1:-1])
    assert lib.ABI_VERSION == 6  # additive, like every entry point since version 6


# ----------------------------------------------------------------------------- b. the host's checks
def test_host_rejects_bad_arguments_and_enqueues_nothing(lib):
    """every host check raises MnkHipError (the fake device pointers are never dereferenced: nothing is launched when a
    check fails, and N = 0 launches nothing either)"""
    p = 0x1000
    nan, inf = float("nan"), float("inf")

    def adv(ws=p, pl=p, me=p, N=8, m=9, n=9, k=5, I=8, fast=4, thr=2 ** 31, pri=p, pdt=0, val=p, vdt=0, c=1.25, rows=p,
            T=81, rp=p, rv=p, rz=p, lo=p, ldt=0, lm=p, cons=4, cv=50.0, cs=0.5, gs=1.0, tfull=p, tfast=p, gscore=p,
            vroot=p):
        return lib.call("mnk_search_selfplay_advance_gumbel", ws, pl, me, N, m, n, k, I, fast, thr, pri, pdt, val, vdt, c,
                        1, None, 0, rows, T, rp, rv, rz, lo, ldt, lm, None, None, None, None, cons, cv, cs, gs, tfull,
                        tfast, gscore, vroot, None)

    for bad in (dict(ws=None), dict(pl=None), dict(me=None), dict(pri=None), dict(val=None), dict(rows=None),
                dict(rp=None), dict(rv=None), dict(rz=None), dict(lo=None), dict(lm=None), dict(N=-1), dict(T=80),
                dict(fast=9), dict(fast=0), dict(I=0, fast=0), dict(I=2049, fast=1), dict(thr=2 ** 32 + 1), dict(pdt=2),
                dict(vdt=-1), dict(ldt=3), dict(c=-1.0), dict(c=nan), dict(k=10), dict(m=40, n=40),
                dict(cons=0), dict(cons=lib.PUCT_CONSIDERED_MAX + 1), dict(cons=-1), dict(cv=-1.0), dict(cv=nan),
                dict(cv=inf), dict(cs=-0.5), dict(cs=nan), dict(gs=-1.0), dict(gs=nan), dict(gs=inf), dict(tfull=None),
                dict(tfast=None), dict(gscore=None), dict(vroot=None)):
        for N in (8, 0):  # (the checks come before the empty batch's early return)
            with pytest.raises(lib.MnkHipError, match="mnk_search_selfplay_advance_gumbel"):
                adv(**dict(bad, N=bad.get("N", N)))
    assert adv(N=0) == 0 and adv(N=0, thr=2 ** 32, fast=8) == 0 and adv(N=0, thr=0, fast=1, I=2048) == 0
    assert adv(N=0, cons=1, cv=0.0, cs=0.0, gs=0.0) == 0 and adv(N=0, cons=lib.PUCT_CONSIDERED_MAX, gs=3.0e38) == 0
    assert adv(N=0, m=25, n=25, T=625) == 0  # (a large board)


# ----------------------------------------------------------------------------- c. the class
def test_the_class_checks_its_options_before_touching_the_gpu(lib):
    from selfplay.search_selfplay import AsyncSearchSelfPlay

    ev = lambda o, m: None  # noqa: E731 (never called)
    for bad, word in ((dict(root_noise=(0.3, 0.25)), "root_noise"), (dict(solver=True), "solver"),
                      (dict(keep_tree=True), "keep_tree"), (dict(leaves=2), "leaves")):
        with pytest.raises(ValueError, match="gumbel does not combine with " + word):
            AsyncSearchSelfPlay(3, 3, 3, 4, evaluator=ev, iterations=8, device="no such device", gumbel=4, **bad)
    for bad in (dict(gumbel=0), dict(gumbel=lib.PUCT_CONSIDERED_MAX + 1), dict(gumbel=2.5), dict(gumbel=True),
                dict(gumbel=4, gumbel_c=(50.0,)), dict(gumbel=4, gumbel_c=(-1.0, 0.5)),
                dict(gumbel=4, gumbel_scale=float("nan")), dict(gumbel_scale=-1.0)):
        with pytest.raises(ValueError, match="gumbel"):
            AsyncSearchSelfPlay(3, 3, 3, 4, evaluator=ev, iterations=8, device="no such device", **bad)


# ----------------------------------------------------------------------------- d. the rule against the lockstep rule
@pytest.mark.parametrize("board,N,P", [((3, 3, 3), 6, 2 * 9 + 3), ((4, 6, 3), 4, 24 + 4)])
def test_with_every_ply_full_the_rule_is_the_lockstep_gumbel_rule(board, N, P):
    m, n, k = board
    C, I, cons, seed, id0 = m * n, 8, 4, 13, 5
    ev = exact_np(C)
    rule = AsyncGumbelRule(m, n, k, N, C, I, I, 2 ** 32, 1.25, seed, cons, env_id0=id0)
    obs, mask = rule.view()
    for r in range(P * (I + 1)):
        obs, mask, fresh = rule.advance(*ev(obs, mask))
        assert fresh.tolist() == [int(r % (I + 1) == I)] * N  # the rows stay in step
    lock = GumbelSelfPlayRule(m, n, k, N, C)
    view = lock.view()
    for p in range(P):
        actions, _, _, policy, _ = gumbel_puct(view[0], k, I, 1.25, ev, cons, seed=seed, step=p, env_id0=id0)
        view = lock.step_moves(policy, actions, p)
    assert not rule.errors and not lock.errors
    assert np.array_equal(rule.ring_planes, lock.ring_planes) and np.array_equal(rule.ring_visits, lock.ring_visits)
    assert np.array_equal(rule.ring_z, lock.ring_z) and np.array_equal(rule.boards, lock.boards)
    assert np.array_equal(rule.meta(), lock.meta()) and rule.stats.tolist() == lock.stats.tolist()
    assert np.array_equal(obs, view[0]) and np.array_equal(mask, view[1])  # the next roots
    assert rule.row_plies.tolist() == [P] * N and rule.plies_max == P
    assert lock.stats[0] > 0 and lock.ring_visits.any() and rule.fast_records == 0


# ----------------------------------------------------------------------------- e. the GPU tests' seeds and shapes
MIXED_RUNS = [case[:4] for case in MIXED_CASES]               # what the tests are parametrized by,
MIXED_HOW = {case[:4]: case[4:] for case in MIXED_CASES}       # and the rest of a case by it
assert len(MIXED_HOW) == len(MIXED_CASES)


def new_rule(board, N, seed, start=None, T=None, env_id0=ENV_ID0):
    m, n, k = board
    rule = AsyncGumbelRule(m, n, k, N, T or m * n, FULL, FAST, THRESHOLD, 1.25, seed, CONSIDERED, env_id0=env_id0)
    state = start_state(board, start)
    if state is not None:
        rule.load(*state)
        rule.begin()
    return rule


@functools.lru_cache(maxsize=None)
def mixed_run(board, N, rounds, seed, start=None, *read_on_the_device):
    rule = new_rule(board, N, seed, start)
    ev = exact_np(rule.C)
    obs, mask = rule.view()
    for _ in range(rounds):
        obs, mask, _ = rule.advance(*ev(obs, mask))
    return rule


def test_the_fast_table_is_a_truncated_first_round_of_sequential_halving():
    assert FAST < CONSIDERED <= FULL
    fast, full = schedule(CONSIDERED, FAST), schedule(CONSIDERED, FULL)
    assert fast[CONSIDERED].tolist() == [0] * FAST  # three of the four considered moves get one visit each, and that is all
    assert full[CONSIDERED].tolist() == [0, 0, 0, 0, 1, 1, 2, 2]
    assert fast[2].tolist() == [0, 0, 1] and fast[1].tolist() == [0, 1, 2]


@pytest.mark.parametrize("board,N,rounds,seed", MIXED_RUNS)
def test_every_case_records_fast_and_full_plies_and_leaves_the_rows_out_of_step(board, N, rounds, seed):
    start = MIXED_HOW[board, N, rounds, seed][0]
    rule = mixed_run(board, N, rounds, seed, *MIXED_HOW[board, N, rounds, seed])
    print(f"{board}: games {rule.stats[0]}, full / fast records {rule.full_records} / {rule.fast_records}, row plies "
          f"{rule.row_plies.tolist()}")
    assert not rule.errors and N % 4
    if (board, start) != ((9, 9, 5), None):  # (150 launches from the empty 9x9 board end no game: every other case does)
        assert rule.stats[0] > 0
    assert rule.full_records > 0 and rule.fast_records > 0
    assert len(set(rule.row_plies.tolist())) > 1
    assert any(e["full"] for e in rule.log) and any(not e["full"] for e in rule.log)
    full_roots = {mp for mp, budget in rule.root_rows if budget == FULL}
    fast_roots = {mp for mp, budget in rule.root_rows if budget == FAST}
    assert CONSIDERED in full_roots and CONSIDERED in fast_roots  # both tables' last rows are read


def test_the_cases_together_reach_every_branch():
    small = mixed_run(*MIXED_CASES[0])
    rows = {mp for mp, _ in small.root_rows}
    assert rows == {1, 2, 3, 4}  # roots with F < considered (schedule rows m' < m) and with F = 1 (row m' = 1)
    assert any(e["free"] < CONSIDERED and e["full"] for e in small.log)      # a policy target of such a root
    assert any(e["free"] < CONSIDERED and not e["full"] for e in small.log)  # and a fast ply of one
    assert any(e["won"] for e in small.log) and any(e["drawn"] for e in small.log)  # a game ends by a win, one by a draw
    assert small.stats[1] > 0 and small.stats[2] > 0 and small.stats[3] > 0
    assert small.row_plies.min() > 2 * small.C  # the ring (T = C) wraps, more than twice
    mid = mixed_run(*MIXED_CASES[1])
    assert mid.row_plies.min() > mid.C and mid.stats[0] > 0  # and on a generic board
    large = mixed_run(*MIXED_CASES[2])
    assert large.row_plies.min() > 8  # several plies of every row on the flagship board


def test_the_new_boards_are_one_of_every_kind_and_every_dtype_is_read():
    """the boards of MIXED_CASES[3:] by the form that runs them (the built-in rows of MNK_DISPATCH are <1,3,3>, <3,9,5>,
    <6,13,5>, <8,15,5> and <12,19,5>: 32-bit words per plane, columns, k; any other board takes the generic form of its
    word count), and what the device reads and writes spread over them"""
    new = MIXED_CASES[3:8]
    assert [(record_words(b[0], b[1]), b[1], b[2]) for b, *_ in new[:3]] == [(6, 13, 5), (8, 15, 5), (12, 19, 5)]
    assert [record_words(b[0], b[1]) for b, *_ in new[3:]] == [5, 2]
    assert 16 * (15 + 1) % 32 == 0 and 19 * 19 % 4  # rows of n + 1 bits fill the last word; a row stride that is not C
    assert ((19, 19, 5), "uint8") in {(c[0], c[5]) for c in new}  # 361-byte leaf rows at odd offsets
    assert "bfloat16" in {c[5] for c in new} and "bfloat16" in {c[6] for c in new} and True in {c[7] for c in new}
    assert all(c[4] == "golden" for c in new[:4]) and new[4][4] is None
    small = mixed_run(*new[4])
    assert small.row_plies.min() > small.C  # from the empty board: more than a lap of the ring (T = C)
