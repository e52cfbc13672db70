"""CPU: per-row search self-play that keeps the played move's subtree -- the C ABI of
``mnk_search_selfplay_advance_keep`` (header, exports, binding, the host's argument checks, which reject before anything is
enqueued, the LDS total among them), the argument checks of ``AsyncSearchSelfPlay(keep_tree=..., tree_nodes=...)``, and the
numpy restatement in tests/search_selfplay_async_keep_rule.py: against ``AsyncOptsRule`` with ``keep_tree`` off, against
the lockstep composition (``ReusePuct.act`` visits -> ``SelfPlayRule.step``) with every ply full, and a carried proven root
with the solver.  The seeds of the GPU cases (tests/search_selfplay_async_keep_cases.py) are checked here with the rule."""
import numpy as np
import pytest
import torch

import search_selfplay_async_keep_cases as cases
from player_cases import check_header_and_binding, lib  # noqa: F401 (lib: the fixture)
from puct_reuse_rule import ReusePuct
from search_selfplay_async_keep_rule import AsyncKeepRule
from search_selfplay_async_opts_rule import AsyncOptsRule
from search_selfplay_async_rule import exact_np
from search_selfplay_rule import SelfPlayRule
from test_search_selfplay_async_opts_cpu import _params, assert_same_games, run


# ----------------------------------------------------------------------------- a. the entry point
def test_the_header_declares_the_entry_point_and_the_binding_has_it(lib):
    check_header_and_binding(lib, "mnk_search_selfplay_advance_keep")
    old, new = _params("mnk_search_selfplay_advance_opts"), _params("mnk_search_selfplay_advance_keep")
    # every argument of mnk_search_selfplay_advance_opts up to root_priors, the three new ones, the stream
    assert old[-2:] == ["float* root_priors", "void* stream"]
    assert new == old[:-1] + ["int tree_iterations", "int keep_nodes", "int32_t* carried", "void* stream"]
    sig = lib.SIGNATURES
    assert sig["mnk_search_selfplay_advance_keep"][:len(old) - 1] == sig["mnk_search_selfplay_advance_opts"][:-1]
    assert len(sig["mnk_search_selfplay_advance_keep"]) == len(new)
    assert lib.ABI_VERSION == 6  # additive, like every entry point since version 6


# ----------------------------------------------------------------------------- b. the host's checks
def test_host_rejects_bad_arguments_and_enqueues_nothing(lib):
    """every host check raises MnkHipError (the fake device pointers are never dereferenced: nothing is launched when a
    check fails, and N = 0 launches nothing either)"""
    p = 0x1000

    def adv(ws=p, N=8, m=9, n=9, k=5, I=8, fast=4, T=None, solver=1, alpha=0.3, eps=0.25, TI=16, keep=9, carried=p):
        return lib.call("mnk_search_selfplay_advance_keep", ws, p, p, N, m, n, k, I, fast, 2 ** 31, p, 0, p, 0, 1.25, 0, 1,
                        None, 0, p, m * n if T is None else T, p, p, p, p, 0, p, None, None, None, None, solver, alpha, eps,
                        0, None, TI, keep, carried, None)

    # the LDS total of 32x31 with noise at the largest tree: 4 * 992 doubles + 4 * 2 * 2050 u16 + 1024 B of static stage =
    # 65 568 B, 32 B above 64 KiB -- what a plain launch may ask for where no device answers, and on a device whose own
    # limit is that; a device that allows more takes the launch
    limit = 64 * 1024
    if torch.cuda.is_available():
        limit = torch.cuda.get_device_properties(0).shared_memory_per_block
    big = dict(m=32, n=31, TI=2048, keep=9)
    lds_overflow = (big,) if 4 * 992 * 8 + 4 * 2 * 2050 * 2 + 1024 > limit else ()
    assert lds_overflow or limit > 64 * 1024
    for bad in (dict(carried=None), dict(TI=7, keep=1), dict(I=2048, fast=1, TI=2049, keep=1), dict(TI=2049, keep=9),
                dict(keep=0), dict(keep=16 + 2 - 8), dict(keep=-1),
                # the checks of mnk_search_selfplay_advance_opts still hold
                dict(ws=None), dict(fast=9), dict(T=80), dict(solver=2), dict(alpha=-0.3), dict(eps=1.5), dict(k=10),
                ) + lds_overflow:
        for N in (8, 0):  # (the checks come before the empty batch's early return)
            with pytest.raises(lib.MnkHipError, match="mnk_search_selfplay_advance_keep"):
                adv(**dict(bad, N=N))
    # good edge cases: the smallest and the largest tree, the largest keep_nodes, and what fits the LDS
    assert adv(N=0) == 0 and adv(N=0, TI=8, keep=1) == 0 and adv(N=0, TI=16, keep=9) == 0
    assert adv(N=0, TI=2048, keep=2041) == 0 and adv(N=0, I=2048, fast=1, TI=2048, keep=1) == 0
    assert adv(N=0, **dict(big, alpha=0.0, eps=0.0)) == 0  # (without noise it fits)
    assert adv(N=0, **dict(big, TI=2046)) == 0 and adv(N=0, m=31, n=31, TI=2048, keep=9) == 0  # (65 536 and 64 576 B)
    assert adv(N=0, m=19, n=19, TI=2048, keep=9) == 0
    if not lds_overflow:
        assert adv(N=0, **big) == 0


# ----------------------------------------------------------------------------- c. the class
def test_the_class_checks_its_options_before_touching_the_gpu(lib):
    from selfplay.search_selfplay import AsyncSearchSelfPlay

    ev = lambda o, m: None  # noqa: E731 (never called)
    for bad in (dict(tree_nodes=17), dict(keep_tree=False, tree_nodes=17),  # tree_nodes without keep_tree
                dict(keep_tree=True, tree_nodes=8), dict(keep_tree=True, tree_nodes=2050),
                dict(keep_tree=True, tree_nodes=0)):
        with pytest.raises(ValueError, match="tree_nodes"):
            AsyncSearchSelfPlay(3, 3, 3, 4, evaluator=ev, iterations=8, device="no such device", **bad)
    with pytest.raises(ValueError, match="tree_nodes"):  # the default, 2 * iterations + 1, out of range
        AsyncSearchSelfPlay(3, 3, 3, 4, evaluator=ev, iterations=1025, device="no such device", keep_tree=True)
    # in range: the check passes and the device is what fails
    for good in (dict(keep_tree=True), dict(keep_tree=True, tree_nodes=9), dict(keep_tree=True, tree_nodes=2049)):
        with pytest.raises(Exception) as info:
            AsyncSearchSelfPlay(3, 3, 3, 4, evaluator=ev, iterations=8, device="no such device", **good)
        assert "tree_nodes" not in str(info.value)


# ----------------------------------------------------------------------------- d. the rule
M, N_, K = 3, 3, 3
C = M * N_
FULL, FAST, THRESHOLD = cases.FULL, cases.FAST, cases.THRESHOLD


def test_with_keep_tree_off_it_is_the_opts_rule_round_by_round():
    args = (M, N_, K, 7, C, FULL, FAST, THRESHOLD, 1.25, 2, 6, 3)
    kw = dict(root_noise=(0.3, 0.25), solver=True)
    opts = AsyncOptsRule(*args, **kw)
    rule = run(AsyncKeepRule(*args, **kw), 130, opts)
    assert_same_games(rule, opts)
    assert opts.stats[0] > 0 and opts.fast_records > 0 and opts.full_records > 0
    assert not rule.carried.any() and not rule.trace
    # and keeping the trees plays other games
    kept = run(AsyncKeepRule(*args, keep_tree=True, **kw), 130)
    assert not np.array_equal(kept.ring_visits, opts.ring_visits) and kept.carried.any()


@pytest.mark.parametrize("board,N,tree_nodes", [((3, 3, 3), 6, 13), ((3, 3, 3), 6, 8), ((4, 6, 3), 5, 13), ((4, 6, 3), 5, 8)])
def test_with_every_ply_full_it_is_the_lockstep_composition_slot_by_slot(board, N, tree_nodes):
    """``ReusePuct.act`` visits -> ``SelfPlayRule.step``, ply by ply; the rule's ``carried`` after the end of ply p is what
    the lockstep search reports at the start of ply p + 1"""
    m, n, k = board
    cells, I, seed, id0, temp = m * n, 6, 13, 5, 3
    T, P = 4 * cells, 2 * cells + 3
    ev = exact_np(cells)
    rule = AsyncKeepRule(m, n, k, N, T, I, I, 2 ** 32, 1.25, temp, seed, id0, keep_tree=True, tree_nodes=tree_nodes)
    lock = SelfPlayRule(m, n, k, N, T)
    search = ReusePuct(k, I, 1.25, ev, tree_nodes=tree_nodes, seed=seed, env_id0=id0)
    obs, mask = rule.view()
    after = None
    for p in range(P):
        _, visits, _, carried = search.act(lock.view()[0], step=p)
        assert after is None or np.array_equal(carried, after), f"carried, ply {p}"
        lock.step(visits, temp, seed, p, id0)
        for r in range(I + 1):
            obs, mask, fresh = rule.advance(*ev(obs, mask))
            assert fresh.tolist() == [int(r == I)] * N
        after = rule.carried.copy()
        assert np.array_equal(rule.ring_planes[p], lock.ring_planes[p]), f"planes, slot {p}"
        assert np.array_equal(rule.ring_visits[p], lock.ring_visits[p]), f"visits, slot {p}"
        assert np.array_equal(obs, lock.view()[0]), f"next roots, ply {p}"
    assert np.array_equal(rule.ring_z, lock.ring_z) and np.array_equal(rule.boards, lock.boards)
    assert rule.stats.tolist() == lock.stats.tolist() and lock.stats[0] > 0 and not rule.errors and not lock.errors
    kept = [t[3] for t in rule.trace]
    assert max(kept) > 1 and 0 in kept and max(kept) <= tree_nodes - I
    if tree_nodes == 8:
        assert max(kept) == 2  # children were dropped


def test_with_the_solver_a_carried_proven_root_plays_in_the_launch_that_renews_it():
    rule = AsyncKeepRule(M, N_, K, 7, C, FULL, FAST, THRESHOLD, 1.25, 2, 6, 3, solver=True, keep_tree=True)
    ev = exact_np(C)
    obs, mask = rule.view()
    seen = 0
    for _ in range(130):
        proven = [i for i in range(rule.N) if rule.renew[i] and rule.trees[i].proof[0]]
        plies, n_before = rule.row_plies.copy(), [rule.trees[i].n[0] for i in range(rule.N)]
        obs, mask, fresh = rule.advance(*ev(obs, mask))
        for i in proven:  # no iteration was run: the ply ended with the visits the root was carried with
            assert fresh[i] == 1 and rule.row_plies[i] == plies[i] + 1
            assert n_before[i] == [t for t in rule.trace if t[0] == i and t[1] == plies[i] - 1][0][4]
        seen += len(proven)
    assert seen > 0 and not rule.errors
    assert sum(1 for t in rule.trace if t[7]) >= seen  # (every one of them was proven when carried)
    assert all(t[3] > 1 and t[7] == t[5] for t in rule.trace if t[7])  # a proof is kept only with a child to play through


# ----------------------------------------------------------------------------- e. the seeds of the GPU cases
# Chosen here with the rule (tests/search_selfplay_async_keep_cases.py): seed 6 of every mixed case as in
# tests/test_gpu_search_selfplay_async_opts.py, with 19x19x5 under the peaked evaluator (under the dyadic one six
# iterations never visit a child twice there: seeds 6 .. 13 all keep one node at the most); the rule gives, per case,
# (games, the kept counts seen): 3x3x3 21 games, 9x9x5 8, 7x7x4 18, 8x3x3 37, 19x19x5 3 with kept counts 0 .. 7,
# 16x15x5 5, and 3x3x3 with the solver at tree_nodes 8 32 games, five carried roots that keep their proof and two that
# lose it to the truncation (seed 7 gives the same counts).  The chunk case: seeds 1 and 2 play three identical rows; seed 3 keeps 111 / 29 / 111, 95 / 77 / 95 and
# 123 / 116 / 123 nodes over its three plies.
@pytest.mark.parametrize("case", range(len(cases.MIXED)))
def test_the_mixed_cases_show_what_the_gpu_test_needs(case):
    rule = cases.mixed_run(case)
    many, fresh_after_end, truncated, proven = cases.conditions(rule)
    print(cases.MIXED[case][0], many, fresh_after_end, truncated, proven, "games", rule.stats[0], "kept",
          sorted({t[3] for t in rule.trace}))
    assert cases.MIXED[case][1] % 4 and not rule.errors
    assert many and fresh_after_end
    assert rule.fast_records > 0 and rule.full_records > 0 and len(set(rule.row_plies.tolist())) > 1
    noise, solver = cases.MIXED[case][9], cases.MIXED[case][11]
    by_proof = sum(1 for rec in rule.proven_plies if rec[4])
    print("plies ended by proof", by_proof, "noised / plain roots", rule.noised_roots, rule.plain_roots)
    assert by_proof > 0 or not solver  # with the solver a ply ends by proof,
    assert rule.noised_roots > 0 or not noise  # and with noise a root takes it


def test_some_mixed_case_truncates_and_some_carries_a_proven_root():
    found = [cases.conditions(cases.mixed_run(c)) for c in range(len(cases.MIXED))]
    assert any(f[2] for f in found) and any(f[3] for f, case in zip(found, cases.MIXED) if case[11])
    # and the last case has roots whose proof did not outlive the truncation, beside roots that kept theirs
    last = cases.mixed_run(cases.TRUNCATED_SOLVER)
    assert cases.dropped_proofs(last) > 0 and any(t[7] for t in last.trace)
    assert all(cases.dropped_proofs(cases.mixed_run(c)) == 0 for c in range(len(cases.MIXED)) if c != cases.TRUNCATED_SOLVER)


def test_the_chunk_case_keeps_more_than_a_chunk_and_no_multiple_of_eight():
    rule, _ = cases.chunk_run()
    kept = [t[3] for t in rule.trace]
    print("kept", kept)
    assert len(kept) == cases.CHUNK_N * cases.CHUNK_PLIES and not rule.errors
    assert any(x > 64 and x % 8 for x in kept) and len(set(kept[:cases.CHUNK_N])) > 1
    assert max(kept) <= cases.CHUNK_NODES - cases.CHUNK_I
