"""The cases of per-row search self-play with first-play urgency, shared by tests/test_puct_fpu_cpu.py (which checks with
the rule alone that every case shows what it is there for) and tests/test_gpu_search_selfplay_async_fpu.py (which runs them
on the device).  No torch here."""
import functools

import numpy as np

from oracle.packing import pack_boards
from puct_fpu_rule import AsyncKeepFpuRule
from puct_solver_cases import drawn_board
from search_selfplay_async_keep_cases import ENV_ID0, FAST, FULL, THRESHOLD, start_state
from search_selfplay_async_rule import exact_np

NOISE, FPU, N = (0.3, 0.25), (0.25, 0.5), 5  # (five rows: a partial workgroup)
FAINT = (0.03, 0.25)  # the noise of the 19x19x5 case of tests/test_gpu_search_selfplay_async_opts.py


def late_start(m, n, k, rows, seed=1):
    """(planes, meta) of ``rows`` env states: the drawn board less 3 .. 8 stones taken off at random, the side to move by
    the parity of the stones, as the rows of the fixture two stones short of a drawn board.  (The seed: with 0 a noised
    root has one free cell, of prior 1, on which the mix with a Dirichlet draw over one cell is the prior itself, and
    ``Beside`` asks every noised root to differ from its plain priors; checked with the rule on the CPU.)"""
    full, rng = drawn_board(m, n, k), np.random.default_rng(seed)
    boards = []
    for i in range(rows):
        keep = np.ones(m * n, bool)
        keep[rng.choice(m * n, size=3 + i % 6, replace=False)] = False
        boards.append(full & keep.reshape(m, n))
    boards = np.stack(boards)
    moves = boards.reshape(rows, -1).sum(axis=1)
    return pack_boards(boards, m, n), ((moves << 1) | (moves & 1)).astype(np.uint32)


def state_of(board, start):
    return start_state(board, start)  # ("late": ``late_start`` of N rows)


# board, start, temp_plies, rounds, seed, root_noise, solver, keep_tree, tree_nodes.  The rows are N, or as many as a
# stored start state has ("golden": tests/golden/search_selfplay_async_starts.npz, three rows on 19x19x5 and 12x12x5).
# Without keep_tree the entry point is mnk_search_selfplay_advance_opts_fpu, with it mnk_search_selfplay_advance_keep_fpu;
# from the eighth case on both run on the variants <6,13,5> (12x13x5), <8,15,5> (16x15x5) and <12,19,5> (19x19x5) and on
# the generic forms of five words (12x12x5) and of two (7x7x4).
CASES = [
    ((3, 3, 3), None, 2, 130, 6, NOISE, True, False, None),
    ((3, 3, 3), None, 2, 130, 6, None, True, True, 13),
    ((3, 3, 3), None, 2, 130, 6, None, False, True, 8),
    ((9, 9, 5), "late", 4, 150, 6, NOISE, False, False, None),
    ((9, 9, 5), "late", 4, 150, 6, NOISE, True, True, 13),
    ((9, 9, 5), "late", 4, 150, 6, None, True, False, None),
    ((7, 9, 5), "golden", 4, 150, 6, None, False, True, 13),
    ((19, 19, 5), "golden", 4, 150, 6, FAINT, True, True, 13),
    ((16, 15, 5), "golden", 4, 150, 6, None, True, False, None),
    ((12, 13, 5), "golden", 4, 150, 6, None, False, False, None),
    ((12, 12, 5), "golden", 4, 150, 6, NOISE, False, True, 13),
    ((7, 7, 4), None, 4, 500, 6, None, True, True, 13),
    # and the other entry point on each of those kinds.  (Noise only where no stored row is two stones short of a drawn
    # board -- 19x19x5 and 12x12x5: such a row's last root has one free cell, of prior 1, which the mix with a Dirichlet
    # draw over one cell leaves as it is, and ``Beside`` asks every noised root to differ from its plain priors.)
    ((19, 19, 5), "golden", 4, 150, 6, FAINT, True, False, None),
    ((16, 15, 5), "golden", 4, 150, 6, None, False, True, 13),
    ((12, 13, 5), "golden", 4, 150, 6, None, True, True, 13),
    ((12, 12, 5), "golden", 4, 150, 6, None, True, False, None),
    ((7, 7, 4), None, 4, 500, 6, NOISE, False, False, None),
    # both entry points on the generic forms of sixteen and of thirty-two words (ten and 21 words a plane), from a
    # computed start: no row of ``late_start`` has a root with a single free cell, so the noise may be on
    ((17, 17, 5), "late", 4, 150, 6, NOISE, True, False, None),
    ((25, 25, 5), "late", 4, 150, 6, NOISE, False, True, 13),
    ((17, 17, 5), "late", 4, 150, 6, None, True, True, 13),
    ((25, 25, 5), "late", 4, 150, 6, NOISE, True, False, None),
]


def rows_of(state):
    return N if state is None else len(state[1])


def new_rule(board, start, temp, seed, noise, solver, keep, tree_nodes):
    """(the rule of a case on its start state, that state or None)"""
    m, n, k = board
    state = state_of(board, start)
    rule = AsyncKeepFpuRule(m, n, k, rows_of(state), m * n, FULL, FAST, THRESHOLD, 1.25, temp, seed, ENV_ID0,
                            root_noise=noise, solver=solver, keep_tree=keep, tree_nodes=tree_nodes, fpu=FPU)
    if state is not None:
        rule.load(*state)
        rule.begin()
    return rule, state


@functools.lru_cache(maxsize=None)
def mixed_run(case):
    """the rule's run of CASES[case] alone, with its own noise"""
    board, start, temp, _, seed, noise, solver, keep, tree_nodes = CASES[case]
    rule, _ = new_rule(board, start, temp, seed, noise, solver, keep, tree_nodes)
    ev = exact_np(rule.C)
    obs, mask = rule.view()
    for _ in range(CASES[case][3]):
        obs, mask, _ = rule.advance(*ev(obs, mask))
    return rule


def conditions(rule):
    """what a run shows of its options, from the rule's own records: (plies ended by proof before their budget, carried
    plies that kept more than one node, roots backed up with noise)"""
    return (sum(1 for rec in rule.proven_plies if rec[4]), sum(1 for t in rule.trace if t[3] > 1), rule.noised_roots)


def assert_every_option_was_used(case, rule):
    """every case: a game ends, fast and full plies are recorded, the rows are out of step; with the solver a ply ends
    by proof, with ``keep_tree`` a carried ply keeps more than one node, with noise a root takes it"""
    _, _, _, _, _, noise, solver, keep, _ = CASES[case]
    by_proof, kept_many, noised = conditions(rule)
    assert not rule.errors and rule.N % 4
    assert rule.stats[0] > 0 and rule.fast_records > 0 and rule.full_records > 0
    assert len(set(rule.row_plies.tolist())) > 1
    assert by_proof > 0 or not solver
    assert kept_many > 0 or not keep
    assert noised > 0 or not noise
