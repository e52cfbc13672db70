"""CPU: per-row search self-play with several leaves per evaluator call -- the C ABI of
``mnk_search_selfplay_advance_leaves`` (header, exports, binding, the host's argument checks, which reject before anything
is enqueued), the argument checks of ``AsyncSearchSelfPlay(leaves=...)``, and the numpy restatement in
tests/search_selfplay_async_leaves_rule.py: at one leaf against ``AsyncOptsRule`` round by round, with every ply full
against the lockstep composition (``SolverPuct(L=...)`` visits -> ``SelfPlayRule.step``), and the runs that the GPU test
compares the kernel with, whose seeds are chosen here so that every branch of the rule is reached."""
import functools
import os
import re

import numpy as np
import pytest

import puct_solver_rule as ps
from player_cases import HEADER, check_header_and_binding, lib  # noqa: F401 (lib: the fixture)
from search_selfplay_async_keep_cases import start_state
from search_selfplay_async_leaves_rule import AsyncLeavesRule
from search_selfplay_async_opts_rule import AsyncOptsRule
from search_selfplay_async_rule import exact_np
from search_selfplay_rule import Z_UNKNOWN, SelfPlayRule

NOISE = (0.3, 0.25)


# ----------------------------------------------------------------------------- a. the entry point
def _params(name):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert decl, name
    return [" ".join(a.split()) for a in decl.group(1).split(",") if a.strip()]


def test_the_header_declares_the_entry_point_and_the_binding_has_it(lib):
    check_header_and_binding(lib, "mnk_search_selfplay_advance_leaves")
    old, new = _params("mnk_search_selfplay_advance_opts"), _params("mnk_search_selfplay_advance_leaves")
    at = old.index("int fast_iterations") + 1
    # the options' arguments, `leaves` behind fast_iterations and row_sims before the stream
    assert new == old[:at] + ["int leaves"] + old[at:-1] + ["uint32_t* row_sims", "void* stream"]
    sig = lib.SIGNATURES
    a, b = sig["mnk_search_selfplay_advance_opts"], sig["mnk_search_selfplay_advance_leaves"]
    assert b[:at] == a[:at] and b[at + 1:-2] == a[at:-1] and len(b) == len(a) + 2
    assert lib.ABI_VERSION == 6  # additive, like every entry point since version 6
    assert int(re.search(r"#define MNK_PUCT_LEAVES_MAX (\d+)", open(HEADER).read()).group(1)) == lib.PUCT_LEAVES_MAX == 16


# ----------------------------------------------------------------------------- b. the host's checks
def test_host_rejects_bad_arguments_and_enqueues_nothing(lib):
    """every host check raises MnkHipError (the fake device pointers are never dereferenced: nothing is launched when a
    check fails, and N = 0 launches nothing either)"""
    p = 0x1000
    nan, inf = float("nan"), float("inf")

    def adv(ws=p, pl=p, me=p, N=8, m=9, n=9, k=5, I=8, fast=3, L=4, thr=2 ** 31, pri=p, pdt=0, val=p, vdt=0, c=1.25,
            temp=0, rows=p, T=81, rp=p, rv=p, rz=p, lo=p, ldt=0, lm=p, solver=1, alpha=0.3, eps=0.25, nfast=0, roots=None,
            sims=p):
        return lib.call("mnk_search_selfplay_advance_leaves", ws, pl, me, N, m, n, k, I, fast, L, thr, pri, pdt, val, vdt,
                        c, temp, 1, None, 0, rows, T, rp, rv, rz, lo, ldt, lm, None, None, None, None, solver, alpha, eps,
                        nfast, roots, sims, None)

    for bad in (dict(L=0), dict(L=17), dict(L=-1), dict(L=3), dict(I=6), dict(I=12, L=8), dict(sims=None),
                # and every check of mnk_search_selfplay_advance_opts
                dict(ws=None), dict(pl=None), dict(me=None), dict(pri=None), dict(val=None), dict(rows=None),
                dict(rp=None), dict(rv=None), dict(rz=None), dict(lo=None), dict(lm=None), dict(N=-1), dict(T=80),
                dict(fast=9), dict(fast=0), dict(I=0, fast=0), dict(I=2052, fast=1), dict(thr=2 ** 32 + 1), dict(pdt=2),
                dict(vdt=-1), dict(ldt=3), dict(c=-1.0), dict(c=nan), dict(temp=-1), dict(k=10), dict(m=40, n=40),
                dict(solver=2), dict(solver=-1), dict(alpha=-0.3), dict(alpha=nan), dict(alpha=inf), dict(eps=-0.1),
                dict(eps=1.5), dict(eps=nan), dict(eps=1.5, alpha=0.0), dict(nfast=2), dict(nfast=-1)):
        for N in (8, 0):  # (the checks come before the empty batch's early return)
            with pytest.raises(lib.MnkHipError, match="mnk_search_selfplay_advance_leaves"):
                adv(**dict(bad, N=bad.get("N", N)))
    assert adv(N=0) == 0 and adv(N=0, thr=2 ** 32, fast=8) == 0 and adv(N=0, thr=0, fast=1, I=2048, L=16) == 0
    assert adv(N=0, L=1, fast=7) == 0 and adv(N=0, L=16, I=16, fast=5) == 0 and adv(N=0, L=8) == 0
    assert adv(N=0, solver=0, alpha=0.0, eps=0.0) == 0 and adv(N=0, alpha=0.0, eps=1.0, nfast=1, roots=p) == 0
    assert adv(N=0, alpha=3.0e38, eps=0.0) == 0 and adv(N=0, m=25, n=25, T=625) == 0  # (a large board)


# ----------------------------------------------------------------------------- c. the class
def test_the_class_checks_leaves_before_touching_the_gpu(lib):
    from selfplay.search_selfplay import AsyncSearchSelfPlay

    ev = lambda o, m: None  # noqa: E731 (never called)
    for bad in (dict(leaves=4, keep_tree=True), dict(iterations=6, leaves=4), dict(leaves=0), dict(leaves=17),
                dict(leaves=2.5)):
        with pytest.raises(ValueError):
            AsyncSearchSelfPlay(3, 3, 3, 4, evaluator=ev, **dict(dict(iterations=8, device="no such device"), **bad))


# ----------------------------------------------------------------------------- d. one leaf: the rule before
M, N_, K = 3, 3, 3
C = M * N_
FULL, FAST, THRESHOLD = 6, 2, 3 * 2 ** 30


def run(rule, rounds, other=None):
    """``rounds`` launches of ``rule`` with the dyadic evaluator; ``other``: a rule that must go the same way"""
    ev = exact_np(rule.C)
    obs, mask = rule.view()
    for r in range(rounds):
        out = rule.advance(*ev(obs, mask))
        if other is not None:
            want = other.advance(*ev(obs, mask))
            for a, b, what in zip(out, want, ("leaves", "masks", "fresh")):
                assert np.array_equal(a, b), f"{what}, round {r}"
        obs, mask, _ = out
    return rule


def assert_same_games(a, b):
    assert np.array_equal(a.ring_planes, b.ring_planes) and np.array_equal(a.ring_visits, b.ring_visits)
    assert np.array_equal(a.ring_z, b.ring_z) and np.array_equal(a.boards, b.boards) and np.array_equal(a.meta(), b.meta())
    assert a.row_plies.tolist() == b.row_plies.tolist() and a.stats.tolist() == b.stats.tolist()
    assert a.plies_max == b.plies_max and a.errors == b.errors == []
    assert (a.full_records, a.fast_records) == (b.full_records, b.fast_records)


@pytest.mark.parametrize("options", [dict(), dict(solver=True), dict(root_noise=NOISE), dict(root_noise=NOISE, solver=True,
                                                                                             noise_on_fast=True)])
def test_with_one_leaf_it_is_the_rule_of_the_options_round_by_round(options):
    args = (M, N_, K, 7, C, FULL, FAST, THRESHOLD, 1.25, 2, 6, 3)
    old = AsyncOptsRule(*args, **options)
    rule = run(AsyncLeavesRule(*args, leaves=1, **options), 130, old)
    assert_same_games(rule, old)
    assert old.stats[0] > 0 and old.fast_records > 0 and old.full_records > 0 and old.row_plies.min() > C
    assert rule.void_by_walk == rule.void_by_cap == 0 and rule.ring_wraps > 0
    assert len(rule.proven_plies) == len(old.proven_plies) and bool(rule.proven_plies) == bool(options.get("solver"))
    # the counter is n_root - 1 once the pending evaluation is backed up: n_root as the tree stands between two launches
    assert rule.row_sims.tolist() == [rule.trees[i].n[0] for i in range(rule.N)]


# ----------------------------------------------------------------------------- e. every ply full: the lockstep player
@functools.lru_cache(maxsize=None)
def lockstep_runs(board, N, I, L, solver, temp=3, seed=13, id0=5):
    """every ply full, T = 8 C: the rule until every row has P = 2 C plies, and the lockstep composition for P plies:
    (rule, lockstep rule, P, launches used)"""
    m, n, k = board
    cells = m * n
    T, P = 8 * cells, 2 * cells
    ev = exact_np(cells)
    rule = AsyncLeavesRule(m, n, k, N, T, I, I, 2 ** 32, 1.25, temp, seed, id0, solver=solver, leaves=L)
    obs, mask = rule.view()
    rounds = 0
    while rule.row_plies.min() < P:
        obs, mask, _ = rule.advance(*ev(obs, mask))
        rounds += 1
        assert rounds <= 3 * P * (I // L + 1)
    lock = SelfPlayRule(m, n, k, N, T)
    search = ps.SolverPuct(k, I, 1.25, ev, L=L, seed=seed, env_id0=id0, solver=solver)
    for p in range(P):
        _, visits, _, _, _ = search.act(lock.view()[0], step=p)
        lock.step(visits, temp, seed, p, id0)
    return rule, lock, P, rounds


@pytest.mark.parametrize("board,N,I,L", [((3, 3, 3), 6, 8, 2), ((3, 3, 3), 6, 8, 4), ((4, 6, 3), 4, 8, 4)])
@pytest.mark.parametrize("solver", [False, True])
def test_with_every_ply_full_it_leaves_what_the_lockstep_rule_leaves(board, N, I, L, solver):
    rule, lock, P, rounds = lockstep_runs(board, N, I, L, solver)
    assert not rule.errors and not lock.errors
    for i in range(rule.N):
        assert np.array_equal(rule.ring_planes[:P, :, :, i], lock.ring_planes[:P, :, :, i]), f"planes, row {i}"
        assert np.array_equal(rule.ring_visits[:P, i], lock.ring_visits[:P, i]), f"visits, row {i}"
    known = lock.ring_z[:P] != Z_UNKNOWN
    assert known.any() and np.array_equal(rule.ring_z[:P][known], lock.ring_z[:P][known])
    assert lock.stats[0] > 0 and lock.ring_visits[:P].any()
    if solver:  # proven roots play at once: fewer launches
        assert rounds < P * (I // L + 1)
        assert any(rec[4] for rec in rule.proven_plies)
    else:  # a ply of budget I takes exactly I / L + 1 launches
        assert rounds == P * (I // L + 1) and rule.row_plies.tolist() == [P] * N
        assert_same_games(rule, _as_async(lock, rule))
    assert rule.row_plies.max() <= rule.T  # (no slot below P was written twice)


@pytest.mark.parametrize("board,N", [((3, 3, 3), 6), ((4, 6, 3), 5)])
def test_the_solver_runs_of_the_gpu_test_need_fewer_launches_than_the_lockstep_player(board, N):
    """the seeds of tests/test_gpu_search_selfplay_async_leaves.py, case 3: I = 16, L = 4"""
    rule, lock, P, rounds = lockstep_runs(board, N, 16, 4, True)
    assert not rule.errors and rounds < P * (16 // 4 + 1) and rule.row_plies.max() <= rule.T
    assert np.array_equal(rule.ring_visits[:P], lock.ring_visits[:P]) and np.array_equal(rule.ring_planes[:P], lock.ring_planes[:P])


def _as_async(lock, like):
    """the lockstep rule with the counters an async rule keeps, for ``assert_same_games``"""
    lock.row_plies, lock.plies_max = like.row_plies.copy(), like.plies_max
    lock.full_records, lock.fast_records = like.full_records, like.fast_records
    return lock


def test_a_budget_is_met_exactly_whatever_its_remainder():
    """fast = 3 with L = 4 and L = 2: a fast ply takes ceil(3 / L) + 1 launches and its root gets at most 3 visits above
    its own evaluation"""
    for L, launches in ((4, 2), (2, 3)):
        rule = AsyncLeavesRule(M, N_, K, 3, C, 8, 3, 0, 1.25, 2, 6, 3, leaves=L)  # (threshold 0: every ply fast)
        ev = exact_np(C)
        obs, mask = rule.view()
        for r in range(4 * launches):
            if r % launches == launches - 1:
                assert rule.row_sims.tolist() == [3] * 3
            obs, mask, fresh = rule.advance(*ev(obs, mask))
            assert fresh.tolist() == [int(r % launches == launches - 1)] * 3
        assert rule.row_plies.tolist() == [4] * 3 and rule.void_by_cap == 3 * 4 * (L * (launches - 1) - 3)


# ----------------------------------------------------------------------------- f. the runs of the GPU test
# board, rows, leaf dtype, dtype of priors and values, device key word, temp_plies, rounds, start ("golden": a stored env
# state near the end of games), seed, root_noise, noise_on_fast, solver, leaves, c:
# tests/test_gpu_search_selfplay_async_leaves.py runs the kernel beside these.  The seeds are chosen here, with the rule
# alone, so that every case shows a void slot by the walk, one by the cap, a finished game, with the solver a ply ended by
# proof and on the small boards a ring that wraps.
#
# A walk makes a slot void when it runs into a node that an earlier slot of the round created, which takes a node whose
# best child is still best under a virtual visit (q = -1 on a new child).  With the dyadic evaluator's priors -- several
# cells share every value -- that happens where few cells are free: all the time on 3x3x3, and on none of the other
# boards in 150 seeds of the rule.  So the other cases mix in a root noise that is nearly all on one cell (a small alpha,
# eps = 0.9: P' = 0.1 P + 0.9 eta), and where the board's priors still hold the second slot off (c sqrt(2) (P'_a / 2 -
# P'_b) must exceed 1) a larger c: then the second slot of a noised root's first round follows the first into its new
# child.  8x3x3, 7x7x4 and 16x15x5 get the noise on top of what they are asked to cover.
GPU_FULL, GPU_FAST = 8, 3
GPU_CASES = {
    "3x3x3": ((3, 3, 3), 7, "f32", "f32", False, 2, 90, None, 6, NOISE, False, True, 4, 1.25),
    "9x9x5": ((9, 9, 5), 5, "bf16", "f32", False, 6, 250, None, 2, (0.006, 0.9), True, False, 4, 1.25),
    "7x7x4": ((7, 7, 4), 5, "u8", "f32", True, 4, 300, None, 3, (0.01, 0.9), False, True, 2, 4.0),
    "8x3x3": ((8, 3, 3), 7, "u8", "bf16", False, 2, 200, None, 3, (0.02, 0.9), False, True, 4, 1.25),
    "19x19x5": ((19, 19, 5), 3, "f32", "f32", False, 4, 60, "golden", 3, (0.003, 0.9), False, True, 4, 4.0),
    "16x15x5": ((16, 15, 5), 5, "f32", "bf16", False, 4, 90, "golden", 3, (0.003, 0.9), False, False, 2, 4.0),
    # the generic forms of sixteen and of thirty-two words, from a computed start ("late")
    "17x17x5": ((17, 17, 5), 5, "u8", "f32", False, 4, 150, "late", 3, (0.003, 0.9), False, True, 4, 4.0),
    "25x25x5": ((25, 25, 5), 5, "bf16", "bf16", False, 4, 150, "late", 3, (0.003, 0.9), False, False, 2, 4.0),
}
ENV_ID0 = 3


def gpu_rule(case, state=None):
    board, N, _, _, _, temp, _, _, seed, noise, on_fast, solver, L, c = GPU_CASES[case]
    m, n, k = board
    rule = AsyncLeavesRule(m, n, k, N, m * n, GPU_FULL, GPU_FAST, THRESHOLD, c, temp, seed, ENV_ID0, root_noise=noise,
                           noise_on_fast=on_fast, solver=solver, leaves=L)
    if state is not None:
        rule.load(*state)
        rule.begin()
    return rule


def assert_every_branch_was_reached(case, rule):
    board, start, solver = GPU_CASES[case][0], GPU_CASES[case][7], GPU_CASES[case][11]
    by_proof = sum(1 for rec in rule.proven_plies if rec[4])
    print(f"{case}: games {rule.stats[0]}, fast / full records {rule.fast_records} / {rule.full_records}, row plies "
          f"{rule.row_plies.tolist()}, void by walk / by cap {rule.void_by_walk} / {rule.void_by_cap}, ring wraps "
          f"{rule.ring_wraps}, plies ended by proof {by_proof}")
    assert not rule.errors
    assert rule.void_by_walk > 0 and rule.void_by_cap > 0 and rule.stats[0] > 0
    assert rule.fast_records > 0 and rule.full_records > 0
    if start is None:  # (from the empty board every case runs more than a lap of its T = C ring)
        assert rule.ring_wraps > 0
    if solver:
        assert by_proof > 0
    if GPU_CASES[case][9]:
        assert rule.noised_roots > 0  # with noise a root takes it


@pytest.mark.parametrize("case", list(GPU_CASES))
def test_the_gpu_cases_reach_every_branch_of_the_rule(case):
    state = None
    if GPU_CASES[case][7] == "golden":
        with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                                  "search_selfplay_async_starts.npz")) as z:
            state = z[case + "_planes"], z[case + "_meta"]
    elif GPU_CASES[case][7] == "late":
        state = start_state(GPU_CASES[case][0], "late")
    rule = gpu_rule(case, state)
    run(rule, GPU_CASES[case][6])
    assert_every_branch_was_reached(case, rule)
    assert len(set(rule.row_plies.tolist())) > 1
