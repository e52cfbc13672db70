"""What the CPU and the GPU tests of the PUCT player with proofs share (tests/test_puct_solver_cpu.py,
tests/test_gpu_puct_solver.py): the boards, budgets and positions, the position of the misled search, and the rule's
answer on each (tests/puct_solver_rule.py), computed once per process."""
import functools

import numpy as np

from playout_rule import has_run
from player_cases import board
from puct_reuse_cases import advance, exact_np
from puct_solver_rule import SolverPuct
from tactical_rule import random_positions, tactical_sets

C_PUCT, SEED, ENV_ID0 = 1.25, 47, 3
#        name      board        rows  I
CASES = {
    "3x3x3": ((3, 3, 3), 64, 64),      # NW = 1; every stage of a game, the last free cell included
    "4x6x3": ((4, 6, 3), 16, 48),      # a built-in sibling variant
    "5x5x4": ((5, 5, 4), 16, 96),      # the generic form
    "9x9x5": ((9, 9, 5), 16, 128),     # late in the game: at most 12 free cells; C > 64
    "19x19x5": ((19, 19, 5), 4, 32),   # the multi-word form; one immediate win on the board
    # the boards that share a built-in variant with a board of another row count (tests/line_rule.py): the batch of
    # ``sibling_positions``, which needs seven rows -- a partial workgroup on the three large boards
    "8x3x3": ((8, 3, 3), 16, 48),      # <1,3,3>: 24 cells for the variant's 9; a plane that fills its word exactly
    "7x9x5": ((7, 9, 5), 8, 64),       # <3,9,5>: 63 cells for 81
    "12x13x5": ((12, 13, 5), 7, 32),   # <6,13,5>: 156 cells for 169
    "16x15x5": ((16, 15, 5), 7, 32),   # <8,15,5>: 240 cells for 225, 256 bits
    "18x19x5": ((18, 19, 5), 7, 32),   # <12,19,5>: 342 cells for 361
    # the generic forms of four and of eight words
    "7x9x7": ((7, 9, 7), 8, 32),       # three words
    "12x12x5": ((12, 12, 5), 8, 16),   # five words
    # the generic forms of sixteen and of thirty-two words, on the batch of ``sibling_positions``: a kernel that took its
    # cell count from the word count (320 for 289, 672 for 625) would not draw the boards that fill inside the search
    "17x17x5": ((17, 17, 5), 7, 32),   # ten words; a guard-column row of 18 bits
    "25x25x5": ((25, 25, 5), 7, 32),   # 21 words: an odd count; a guard-column row of 26 bits
}
SIBLINGS = ("8x3x3", "7x9x5", "12x13x5", "16x15x5", "18x19x5")
LARGE = ("17x17x5", "25x25x5")
LARGE_SEED = 2  # of their rows: chosen with the rule so that at L = 1 and 4 a board fills inside the search and the win in
#                 the last row is found (tests/test_puct_solver_cpu.py); the rows named after the board find neither
LEAVES = (1, 4)


@functools.lru_cache(maxsize=None)
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


def last_row_win(m, n, k, rng, more=2):
    """the drawn board less the stone of one side at the end of a stripe of the other in row m - 1 -- the other side, to
    move, completes a run that lies in that row -- and less ``more`` stones above it.  Returns (obs [2, m, n], the cell)"""
    full = drawn_board(m, n, k)
    for cell in range(m * n - 1, (m - 1) * n - 1, -1):
        for side in (0, 1):
            row = full[side, m - 1].copy()
            if row[cell - (m - 1) * n]:
                continue
            row[cell - (m - 1) * n] = True
            if has_run(row.reshape(1, 1, n), k)[0]:
                while True:  # (the stones taken off above must leave the side to move no other run to complete)
                    keep = np.ones(m * n, bool)
                    keep[cell] = False
                    keep[rng.choice((m - 1) * n, size=more, replace=False)] = False
                    obs = (full[:: 1 if side == 0 else -1] & keep.reshape(m, n)).astype(np.float32)
                    if tactical_sets(obs[None], k)[1].sum() == 1:
                        return obs, cell
    raise AssertionError((m, n, k))


def sibling_positions(m, n, k, rows, rng):
    """what a kernel that took the variant's own cell or row count for the board's would get wrong: one free cell; two
    and three free cells (with two, neither side can complete a run: the board fills inside the search, a draw at m * n
    stones); a full board; a win at once whose run lies in row m - 1 (three free cells); mid-game rows"""
    assert rows >= 7
    obs = np.zeros((rows, 2, m, n), np.float32)
    for _ in range(4096):  # (on 8x3x3 every stone off the drawn board leaves a winning cell: the last try stands)
        obs[:3] = late_positions(m, n, k, 3, rng, 4)
        if not tactical_sets(obs[1:2], k)[0].any():
            break
    obs[3] = drawn_board(m, n, k)
    obs[4], _ = last_row_win(m, n, k, rng)
    obs[5:] = random_positions(m, n, k, rows - 5, rng, max_fill=0.5)
    return obs


@functools.lru_cache(maxsize=None)
def _positions(name):
    (m, n, k), rows, _ = CASES[name]
    rng = np.random.default_rng(LARGE_SEED if name in LARGE else sum(map(ord, name)) + 1)
    if name in SIBLINGS + LARGE:
        return sibling_positions(m, n, k, rows, rng)
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
