"""CPU: the PUCT player that proves wins, draws and losses -- the numpy restatement (tests/puct_solver_rule.py) with the
solver off against the rules it is built on, on their own cases; the soundness of every proof against a brute-force
negamax; a position on which the search without proofs is misled and the search with them is not; that the inputs of the
GPU test (tests/test_gpu_puct_solver.py) hold what they must; and the C ABI of ``mnk_puct_step_solver`` (header, binding,
host checks that reject before anything is enqueued)."""
import numpy as np
import pytest

from player_cases import check_header_and_binding, header_constants, lib  # noqa: F401 (lib: the fixture)
from playout_rule import has_run
from puct_leaves_cases import CASES as LEAVES_CASES
from puct_leaves_cases import reference as leaves_reference
from puct_reuse_cases import advance, exact_np, start
from puct_reuse_rule import ReusePuct
from puct_rule import puct
import puct_search_rule
from puct_solver_cases import (C_PUCT, CASES, ENV_ID0, LARGE, LEAVES, MISLED_BOARD, MISLED_FAR, MISLED_I, MISLED_OBS,
                               MISLED_WIN, REUSE_CASES, SEED, SIBLINGS, last_row_win, misled_reference, positions,
                               reference, reuse_reference)
from puct_solver_rule import PROOF_UNKNOWN, SolverPuct, negamax, puct_solver, value_after
from tactical_rule import random_positions, tactical_sets


def same(got, want, what):
    for j, name in enumerate(("actions", "visits", "root_value", "carried")[:len(want)]):
        g, w = got[j], want[j]
        if name == "root_value":
            g, w = g.view(np.uint32), w.view(np.uint32)
        assert np.array_equal(g, w), (what, name)


# ----------------------------------------------------------------------------- 1. the solver off
@pytest.mark.parametrize("name,L", [("3x3x3", 1), ("3x3x3", 4), ("4x6x3", 2), ("4x6x3", 16), ("9x9x5", 1), ("9x9x5", 8),
                                    ("19x19x5", 4), ("round", 8)])
def test_with_the_solver_off_the_rule_is_the_rule_of_several_leaves(name, L):
    (m, n, k), _, I, _ = LEAVES_CASES[name]
    obs, want, leaves, _ = leaves_reference(name, L)
    seen = []
    rule = SolverPuct(k, I, 1.25, exact_np(m * n), L, seed=43, env_id0=7, leaves=seen, solver=False)
    got = rule.act(obs, step=2)
    same(got, want, (name, L))
    assert (got[4] == PROOF_UNKNOWN).all() and len(seen) == len(leaves)
    for (lo, lm), (wo, wm) in zip(seen, leaves):
        assert np.array_equal(lo, wo) and np.array_equal(lm, wm)


@pytest.mark.parametrize("temperature", [0, 1])
def test_with_the_solver_off_one_leaf_is_the_first_rule(temperature):
    m, n, k, I = 4, 6, 3, 24
    obs = random_positions(m, n, k, 10, np.random.default_rng(5), max_fill=0.7)
    want = puct(obs, k, I, 1.25, exact_np(m * n), seed=5, step=3, env_id0=2, temperature=temperature)
    got = puct_solver(obs, k, I, 1.25, exact_np(m * n), 1, seed=5, step=3, env_id0=2, temperature=temperature,
                      solver=False)
    same(got, want, temperature)


@pytest.mark.parametrize("board,rows,J,distance", [((3, 3, 3), 6, 10, 1), ((4, 6, 3), 5, 12, 2)])
def test_with_the_solver_off_a_kept_tree_is_the_rule_of_the_kept_tree(board, rows, J, distance):
    m, n, k = board
    want_rule = ReusePuct(k, J, 1.25, exact_np(m * n), None, 41, 5)
    rule = SolverPuct(k, J, 1.25, exact_np(m * n), 1, reuse=True, seed=41, env_id0=5, solver=False)
    obs, resets, kept = start(m, n, k, rows, m * 100 + n * 10 + k + distance), np.zeros(rows, np.int64), 0
    for ply in range(8):
        want = want_rule.act(obs, step=ply)
        same(rule.act(obs, step=ply), want, (board, ply))
        kept += int((want[3][:, 0] > 1).sum())
        obs = advance(obs, want[0], k, distance, resets)
    assert kept


# ----------------------------------------------------------------------------- 2. soundness
def small_positions(m, n, k, rows, least, seed):
    """``rows`` random positions of at least ``least`` stones, no run on the board, a free cell"""
    rng, out = np.random.default_rng(seed), []
    while len(out) < rows:
        o = random_positions(m, n, k, 1, rng, max_fill=1.0)[0]
        if least <= o.sum() < m * n:
            out.append(o)
    return np.stack(out)


@pytest.mark.parametrize("L", [1, 4])
@pytest.mark.parametrize("board,least,seed", [((3, 3, 3), 2, 11), ((4, 4, 3), 9, 12)])
def test_every_proof_is_the_negamax_value(board, least, seed, L):
    """48 rows per board, I = 64.  The rule proves 35 / 48 of the 3x3x3 rows and 48 / 48 of the 4x4x3 rows at either L
    (asserted: at least half), and every proof is the value of the exhaustive search, the root value is that number
    exactly, and the move keeps it."""
    m, n, k = board
    rows = 48
    obs = small_positions(m, n, k, rows, least, seed)
    actions, visits, root_value, proof = puct_solver(obs, k, 64, C_PUCT, exact_np(m * n), L, seed=seed)
    proven = proof != PROOF_UNKNOWN
    print(board, L, "proven", int(proven.sum()), "of", rows)
    assert proven.sum() * 2 >= rows
    flat = obs.reshape(rows, 2, m * n) != 0
    for i in np.flatnonzero(proven):
        want = negamax(flat[i], m, n, k)
        assert proof[i] == want and root_value[i] == np.float32(want), (i, proof[i], want)
        assert value_after(flat[i], actions[i], m, n, k) == want, (i, actions[i])
        assert visits[i, actions[i]] > 0
    # and no count is left on a move the tree has proven to lose when another move is not
    for i in np.flatnonzero(proven & (proof >= 0)):
        for a in np.flatnonzero(visits[i]):
            assert value_after(flat[i], a, m, n, k) >= 0, (i, a)


# ----------------------------------------------------------------------------- 3. a misled search
def test_the_misled_position_is_what_it_is_said_to_be():
    m, n, k = MISLED_BOARD
    flat = MISLED_OBS.reshape(2, m * n) != 0
    assert not has_run(flat.reshape(2, m, n), k).any() and flat[0].sum() == flat[1].sum() and (~(flat[0] | flat[1])).sum() == 7
    values = {int(a): value_after(flat, a, m, n, k) for a in np.flatnonzero(~(flat[0] | flat[1]))}
    assert values.pop(MISLED_WIN) == 1 and set(values.values()) == {-1} and MISLED_FAR in values
    mine = flat[0].copy()
    mine[MISLED_WIN] = True
    assert not has_run(mine.reshape(1, m, n), k)[0]  # not at once: three plies


def test_proofs_put_a_misled_search_right():
    """priors of 0.9 on a far cell and a constant value: at I = 96 the search with proofs proves the root a win and plays
    the winning cell, the search without them plays the far cell"""
    assert MISLED_I <= 512
    actions, visits, root_value, _, proof = misled_reference(True)
    assert actions[0] == MISLED_WIN and proof[0] == 1 and root_value[0] == 1.0
    assert visits[0, MISLED_WIN] > 0 and visits[0].sum() == visits[0, MISLED_WIN]
    actions, visits, root_value, _, proof = misled_reference(False)
    assert actions[0] == MISLED_FAR and proof[0] == PROOF_UNKNOWN and root_value[0] < 0
    assert visits[0].sum() == MISLED_I


# ----------------------------------------------------------------------------- the GPU test's inputs
def test_the_gpu_cases_hold_wins_losses_unless_blocked_and_last_cells():
    wins = blocks = last = proven = unknown = 0
    for name, ((m, n, k), rows, _) in CASES.items():
        obs = positions(name)
        assert obs.shape == (rows, 2, m, n)
        flat = obs.reshape(rows, 2, -1) != 0
        assert not has_run(flat[:, 0].reshape(rows, m, n), k).any() and not has_run(flat[:, 1].reshape(rows, m, n), k).any()
        _, W, B = tactical_sets(obs, k)
        wins += int(W.any(axis=1).sum())
        blocks += int((B.any(axis=1) & ~W.any(axis=1)).sum())
        last += int(((~(flat[:, 0] | flat[:, 1])).sum(axis=1) == 1).sum())
        for L in LEAVES:
            proof = reference(name, L)[1][4]
            proven += int((proof != PROOF_UNKNOWN).sum())
            unknown += int((proof == PROOF_UNKNOWN).sum())
        if name == "9x9x5":
            assert ((~(flat[:, 0] | flat[:, 1])).sum(axis=1) <= 12).all()
        if name == "19x19x5":
            assert W[0].sum() == 1 and reference(name, 1)[1][4][0] == 1
    print(wins, blocks, last, proven, unknown)
    assert wins >= 10 and blocks >= 10 and last >= 3 and proven >= 50 and unknown >= 20


# ----------------------------------------------------------------------------- the sibling boards
VARIANT_ROWS = {3: 3, 9: 9, 13: 13, 15: 15, 19: 19}  # the board a built-in variant is named after is square: m = n


def test_the_sibling_cases_hold_what_a_wrong_row_count_gets_wrong():
    the_near_full_rows_hold_what_a_wrong_cell_count_gets_wrong(SIBLINGS)


def test_the_large_cases_hold_what_a_cell_count_from_the_word_count_gets_wrong():
    the_near_full_rows_hold_what_a_wrong_cell_count_gets_wrong(LARGE)


def the_near_full_rows_hold_what_a_wrong_cell_count_gets_wrong(names):
    for name in names:
        (m, n, k), rows, _ = CASES[name]
        obs = positions(name)
        free = (obs.reshape(rows, 2, -1) == 0).all(axis=1).sum(axis=1)
        assert free[:5].tolist() == [1, 2, 3, 0, 3] and (free[5:] > 4).all(), (name, free)
        _, W, _ = tactical_sets(obs, k)
        _, cell = last_row_win(m, n, k, np.random.default_rng(0))
        assert W[4, cell] and W[4].sum() == 1 and cell >= (m - 1) * n, name  # the one win at once, in the last row
        mine = obs[4, 0].copy().reshape(-1)
        mine[cell] = 1
        assert has_run(mine.reshape(1, m, n)[:, m - 1:] != 0, k)[0], name  # the run lies in that row
        for L in LEAVES:
            rule = SolverPuct(k, CASES[name][2], C_PUCT, exact_np(m * n), L, seed=SEED, env_id0=ENV_ID0)
            proof = rule.act(obs, step=2)[4]
            assert proof[0] != PROOF_UNKNOWN, (name, L, proof)
            # the board filled inside the search, a draw (k = 3: every free cell of a late position wins for a side)
            assert 2 in rule.trees[1].term + rule.trees[2].term or k == 3, (name, L)
            assert proof[4] == 1, (name, L, proof)  # the win in the last row was found


STUCK = 4  # in the planted rule's trees: a full board that it did not call drawn


def plant(monkeypatch, vm, vn):
    """``puct_search_rule`` as a kernel that took the variant's own board for the board would search, through the rule's
    patch point (``terminal`` and ``decided``): a new node is terminal when its mover has a run in the first ``vm`` rows
    or ``vm * vn`` stones lie on the board.  A full board that is then not terminal has no cell to go on to: the walk
    ends there every time, the node is evaluated again and its proof stays unknown (marked STUCK in the tree for
    ``select`` to stop at, read as unknown by ``decided``)."""
    select, decided = puct_search_rule.select, puct_search_rule.decided

    def planted_terminal(pos, side, m, n, k):
        won = bool(has_run(pos[side].reshape(1, m, n)[:, :vm], k)[0])
        return 1 if won else (2 if (pos[0] | pos[1]).sum() >= vm * vn else 0)

    def planted_select(tree, root, *args, **kw):
        before = len(tree.n)
        got = select(tree, root, *args, **kw)
        if got is None:
            return got
        path, pos, d, kind = got
        if len(tree.n) > before and not kind and (pos[0] | pos[1]).all():
            tree.proof[path[-1]] = STUCK
        return path, pos, d, 0 if kind == STUCK else kind

    def planted_decided(tree, x, occupied):
        kept = tree.proof
        tree.proof = [0 if pf == STUCK else pf for pf in kept]
        try:
            return decided(tree, x, occupied)
        finally:
            tree.proof = kept

    monkeypatch.setattr(puct_search_rule, "terminal", planted_terminal)
    monkeypatch.setattr(puct_search_rule, "select", planted_select)
    monkeypatch.setattr(puct_search_rule, "decided", planted_decided)


@pytest.mark.parametrize("L", LEAVES)
@pytest.mark.parametrize("name", SIBLINGS)
def test_the_sibling_cases_reject_the_variants_own_board(name, L, monkeypatch):
    """the one defect these boards are there to catch, planted in the rule: 9 cells / 3 rows for 8x3x3, 81 / 9 for 7x9x5,
    169 / 13 for 12x13x5, 225 / 15 for 16x15x5, 361 / 19 for 18x19x5.  With fewer cells or rows than the board has, draws
    are taken too early and the win in the last row is missed; with more, the boards that fill inside the search are not
    drawn and their roots' proofs are lost.  Either way the proofs and the root values of the batch are other ones."""
    (m, n, k), rows, I = CASES[name]
    vm = VARIANT_ROWS[n]
    assert vm != m
    obs, want, leaves = reference(name, L)
    plant(monkeypatch, vm, n)
    rule = SolverPuct(k, I, C_PUCT, exact_np(m * n), L, seed=SEED, env_id0=ENV_ID0)
    got = rule.act(obs, step=2)
    differs = [j for j in range(5) if not np.array_equal(got[j], want[j])]
    print(name, L, "differs in", differs, got[4][:5].tolist(), want[4][:5].tolist())
    assert 2 in differs and 4 in differs, (name, differs)  # the root values and the proofs
    if vm < m:
        assert got[4][4] != 1 and 1 in differs  # the win in row m - 1 is not seen: other visits too


WORD_BOARD = {"17x17x5": (20, 16), "25x25x5": (28, 24)}  # rows x columns of 32 bits a plane word: 320 and 672 cells


@pytest.mark.parametrize("L", LEAVES)
@pytest.mark.parametrize("name", LARGE)
def test_the_large_cases_reject_a_cell_count_taken_from_the_word_count(name, L, monkeypatch):
    """the defect the near-full rows of the two large generic boards are there to catch, planted in the rule: a board
    is full at 32 stones a plane word, 320 for 289 and 672 for 625.  The boards that fill inside the search are then
    not drawn, and the proofs and root values of the batch are other ones."""
    (m, n, k), rows, I = CASES[name]
    vm, vn = WORD_BOARD[name]
    assert vm >= m and m * n < vm * vn == 32 * ((m * (n + 1) + 31) // 32)  # (a row of the plane has a guard column)
    obs, want, leaves = reference(name, L)
    plant(monkeypatch, vm, vn)
    rule = SolverPuct(k, I, C_PUCT, exact_np(m * n), L, seed=SEED, env_id0=ENV_ID0)
    got = rule.act(obs, step=2)
    differs = [j for j in range(5) if not np.array_equal(got[j], want[j])]
    print(name, L, "differs in", differs, got[4][:5].tolist(), want[4][:5].tolist())
    assert 2 in differs and 4 in differs, (name, differs)  # the root values and the proofs


@pytest.mark.parametrize("distance", [1, 2])
@pytest.mark.parametrize("case", range(len(REUSE_CASES)))
def test_the_kept_trees_of_the_gpu_test_arrive_at_decided_roots(case, distance):
    plies, decided = reuse_reference(case, distance)
    print(REUSE_CASES[case], distance, "decided", decided, "carried", sum(int((out[3][:, 0] > 1).sum()) for _, out, _ in plies))
    assert decided >= 1
    assert any((out[3][:, 0] > 1).any() for _, out, _ in plies)


# ----------------------------------------------------------------------------- the C ABI
NAME = "mnk_puct_step_solver"


def test_header_declares_the_entry_point_and_the_binding_matches(lib):
    check_header_and_binding(lib, NAME)
    assert len(lib.SIGNATURES[NAME]) == len(lib.SIGNATURES["mnk_puct_step_leaves"]) + 1
    assert lib.PROOF_UNKNOWN == PROOF_UNKNOWN == -128
    assert "#define MNK_PROOF_UNKNOWN (-128)" in open(lib.__file__.replace("__init__.py", "../../include/mnk_hip.h")).read()
    assert header_constants()["MNK_PUCT_LEAVES_MAX"] == "16"


def test_host_rejects_bad_arguments_and_enqueues_nothing(lib):
    """every host check raises MnkHipError (the fake device pointers are never dereferenced: nothing is launched when a
    check fails, and N = 0 launches nothing either)"""
    p = 0x1000  # a non-NULL pointer that must never be touched

    def step(ws=p, N=8, m=9, n=9, k=5, I=256, L=4, pr=p, pdt=0, va=p, vdt=0, c=1.25, last=0, temp=0, lo=p, ldt=0, lm=p,
             acts=p, proof=None):
        return lib.call(NAME, ws, N, m, n, k, I, L, pr, pdt, va, vdt, c, last, temp, 1, None, 0, None, 0, 0, lo, ldt, lm,
                        acts, None, None, proof, None)

    for bad in (dict(ws=None), dict(pr=None), dict(va=None), dict(N=-1), dict(pdt=2), dict(vdt=-1), dict(I=0),
                dict(I=2052), dict(c=-0.5), dict(c=float("nan")), dict(temp=2), dict(last=2), dict(lo=None), dict(lm=None),
                dict(ldt=3), dict(last=1, acts=None), dict(k=10), dict(m=40, n=40), dict(L=0), dict(L=-1), dict(L=17),
                dict(L=3), dict(I=250, L=4), dict(I=8, L=16)):
        with pytest.raises(lib.MnkHipError, match=NAME):
            step(**bad)
    assert step(N=0) == 0 and step(N=0, last=1, lo=None, lm=None, ldt=9, proof=p) == 0
    assert step(N=0, L=1) == 0 and step(N=0, I=16, L=16) == 0


def test_the_constructors_take_the_flag(lib):
    import torch

    from selfplay.policy import PUCTSearchPolicy
    from selfplay.search_selfplay import SearchSelfPlay  # noqa: F401

    ev = lambda o, msk: (msk.float(), torch.zeros(len(msk)))  # noqa: E731
    assert not PUCTSearchPolicy(5, evaluator=ev).solver
    pol = PUCTSearchPolicy(5, evaluator=ev, iterations=48, leaves=16, reuse=True, root_noise=(0.3, 0.25), solver=True)
    assert pol.solver and pol.evaluations_per_act == 4
    assert "solver" in SearchSelfPlay.__init__.__code__.co_varnames
