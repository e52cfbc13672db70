"""What the CPU and the GPU tests of the PUCT player with proofs share (tests/test_puct_solver_cpu.py,
tests/test_gpu_puct_solver.py): the boards, budgets and positions, the position of the misled search, and the rule's
answer on each (tests/puct_solver_rule.py), computed once per process."""
import functools

import numpy as np

from playout_rule import has_run
from player_cases import board
from puct_solver_rule import SolverPuct
from tactical_rule import random_positions
from test_gpu_puct_reuse import advance, exact_np

C_PUCT, SEED, ENV_ID0 = 1.25, 47, 3
#        name      board        rows  I
CASES = {
    "3x3x3": ((3, 3, 3), 64, 64),      # NW = 1; every stage of a game, the last free cell included
    "4x6x3": ((4, 6, 3), 16, 48),      # a built-in sibling variant
    "5x5x4": ((5, 5, 4), 16, 96),      # the generic form
    "9x9x5": ((9, 9, 5), 16, 128),     # late in the game: at most 12 free cells; C > 64
    "19x19x5": ((19, 19, 5), 4, 32),   # the multi-word form; one immediate win on the board
}
LEAVES = (1, 4)


def drawn_board(m, n, k):
    """a full board [2, m, n] without a run of k of either side: stripes of k - 1 cells (or fewer, where no shift from row
    to row keeps them from lining up), so that a stone taken off the end of a stripe leaves a winning cell"""
    for width in range(k - 1, 0, -1):
        for shift in range(1, 2 * width):
            x = np.array([[((c + shift * r) // width) % 2 == 0 for c in range(n)] for r in range(m)])
            if not has_run(x[None], k)[0] and not has_run(~x[None], k)[0]:
                return np.stack([x, ~x])
    raise AssertionError((m, n, k))


def late_positions(m, n, k, rows, rng, most_free):
    """the drawn board less 1 .. most_free stones taken off at random, either side to move"""
    full = drawn_board(m, n, k)
    out = np.zeros((rows, 2, m, n), np.float32)
    for i in range(rows):
        keep = np.ones(m * n, bool)
        keep[rng.choice(m * n, size=1 + (i * 5) % most_free, replace=False)] = False
        out[i] = full[:: 1 if i % 2 else -1] & keep.reshape(m, n)
    return out


@functools.lru_cache(maxsize=None)
def _positions(name):
    (m, n, k), rows, _ = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)) + 1)
    if name == "9x9x5":
        return late_positions(m, n, k, rows, rng, 12)
    if name == "19x19x5":
        obs = random_positions(m, n, k, rows, rng, max_fill=0.2)
        obs[0] = 0  # four in a row of the side to move, the one open end at cell 0, where the evaluator's prior peaks
        obs[0, 0, 0, 1:5] = 1
        obs[0, 1, 0, 5] = obs[0, 1, 3, 3] = obs[0, 1, 15, 12] = obs[0, 1, 12, 2] = 1
        return obs
    obs = random_positions(m, n, k, rows, rng, max_fill=1.0)
    half = rows // 4
    obs[:half] = late_positions(m, n, k, half, rng, 4)  # the last cells of a game: a full board next ply among them
    return obs


def positions(name):
    return _positions(name).copy()


@functools.lru_cache(maxsize=None)
def reference(name, L, temperature=0):
    """(obs, (actions, visits, root_value, carried, proof), every evaluation's (leaf_obs, leaf_mask)) of the rule"""
    (m, n, k), _, I = CASES[name]
    obs, seen = positions(name), []
    rule = SolverPuct(k, I, C_PUCT, exact_np(m * n), L, seed=SEED, env_id0=ENV_ID0, temperature=temperature, leaves=seen)
    return obs, rule.act(obs, step=2), seen


# ----------------------------------------------------------------------------- the misled search
# 5x5x4, x to move: cell 13 (row 2, column 3) takes the cell that would complete o's diagonal from (0, 1) to (3, 4) and
# makes three in row 2 with both ends free, so x wins at its next move whatever o answers (three plies); every other move
# loses at once.  The evaluator puts 0.9 of the prior on the far corner, cell 4, at every node and values every position
# +1 for its side to move.
MISLED_BOARD = (5, 5, 4)
MISLED_OBS = board([".oxo.",
                    "xooxx",
                    ".xx..",
                    "oooxo",
                    ".xxo."])
MISLED_WIN, MISLED_FAR, MISLED_I = 13, 4, 96


def misled_tables():
    prior = np.full(25, 0.1 / 24, np.float32)
    prior[MISLED_FAR] = 0.9
    return prior


def misled_np(leaf_obs, leaf_mask):
    return leaf_mask * misled_tables(), np.ones(len(leaf_mask), np.float32)


@functools.lru_cache(maxsize=None)
def misled_reference(solver, L=1):
    rule = SolverPuct(MISLED_BOARD[2], MISLED_I, C_PUCT, misled_np, L, seed=SEED, solver=solver)
    return rule.act(MISLED_OBS, deterministic=True)


# ----------------------------------------------------------------------------- a kept tree
#               board      rows  I   L
REUSE_CASES = [((3, 3, 3), 8, 16, 1), ((9, 9, 5), 6, 32, 4)]
REUSE_PLIES = 6


def reuse_start(brd, rows):
    """rows near the end of a game"""
    m, n, k = brd
    rng = np.random.default_rng(m * n + k)
    if brd == (3, 3, 3):
        out = []
        while len(out) < rows:
            o = random_positions(m, n, k, 1, rng, max_fill=0.7)[0]
            if 3 <= o.sum() <= 5:
                out.append(o)
        return np.stack(out)
    return late_positions(m, n, k, rows, rng, 12)


@functools.lru_cache(maxsize=None)
def reuse_reference(case, distance):
    """the rule over REUSE_PLIES plies of a kept tree: per ply (obs, the act's outputs, its evaluations' leaves), and how
    many rows arrived at a carried root that its kept children's proofs decide"""
    brd, rows, I, L = REUSE_CASES[case]
    m, n, k = brd
    seen = []
    rule = SolverPuct(k, I, C_PUCT, exact_np(m * n), L, reuse=True, seed=SEED, env_id0=ENV_ID0, leaves=seen)
    obs, resets, plies, decided = reuse_start(brd, rows), np.zeros(rows, np.int64), [], 0
    for ply in range(REUSE_PLIES):
        del seen[:]
        out = rule.act(obs, step=ply)
        decided += int(rule.proven.sum())
        plies.append((obs, out, list(seen)))
        obs = advance(obs, out[0], k, distance, resets)
    return plies, decided
