"""Writes tests/golden/search_selfplay_async_starts.npz: env states near the end of games, the start of the large-board
cases of tests/test_gpu_search_selfplay_async.py (a search of a few iterations does not finish a game on such a board from
the empty position within a test's rounds): 12x12x5 and 19x19x5, and 7x9x5, 12x13x5, 16x15x5 and 18x19x5, boards that run a
built-in variant named after a board of another row count.  The positions come from the oracle's uniformly random play
(oracle.rollout.random_rollout on an OracleVectorEnv): of 128 games after PLIES plies, the rows whose side to move can
complete a run at once, the most advanced first.  The four non-square boards get two more rows, two stones short of a full
board without a run (``late_rows``): there the board fills, and the game is drawn at m * n stones.

usage: python tests/golden/make_golden_search_selfplay_async.py   (from the repository root; needs no GPU)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from oracle.env_torch import OracleVectorEnv  # noqa: E402
from oracle.packing import pack_boards  # noqa: E402
from oracle.rollout import random_rollout  # noqa: E402
from puct_solver_cases import drawn_board  # noqa: E402
from tactical_rule import completions  # noqa: E402

# m, n, k, rows, plies of random play, rows two stones short of a drawn board
CASES = {"12x12x5": (12, 12, 5, 3, 70, 0), "19x19x5": (19, 19, 5, 3, 150, 0), "7x9x5": (7, 9, 5, 3, 30, 2),
         "12x13x5": (12, 13, 5, 3, 70, 2), "16x15x5": (16, 15, 5, 3, 120, 2), "18x19x5": (18, 19, 5, 3, 150, 2)}


def late_rows(m, n, k, rows, seed=0):
    """(boards bool [rows, 2, m, n], side, moves): ``puct_solver_cases.drawn_board`` less two stones such that neither side
    can complete a run on either free cell -- two plies on the board is full and the game a draw"""
    full = drawn_board(m, n, k)
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < rows:
        keep = np.ones(m * n, bool)
        keep[rng.choice(m * n, size=2, replace=False)] = False
        b = full & keep.reshape(m, n)
        free = ~(b[0] | b[1])
        if not completions(b, np.stack([free, free]), k).any():
            out.append(b)
    boards = np.stack(out)
    moves = boards.reshape(rows, -1).sum(axis=1)
    return boards, moves & 1, moves


def starts(m, n, k, rows, plies, late=0, seed=0, envs=128):
    env = OracleVectorEnv(m, n, k, envs)
    random_rollout(env, seed, 0, plies)
    boards = env.boards.numpy() != 0  # [envs, 2, m, n], plane 0 = black
    side = env.current_player.numpy()
    moves = env.move_counts.numpy()
    idx = np.arange(envs)
    mine = boards[idx, side]
    wins = completions(mine, ~(boards[:, 0] | boards[:, 1]), k).reshape(envs, -1).any(axis=1)
    order = sorted(idx, key=lambda i: (not wins[i], -moves[i], i))[:rows]
    assert all(wins[i] for i in order)
    boards, side, moves = boards[order], side[order], moves[order]
    if late:
        more = late_rows(m, n, k, late)
        boards, side, moves = (np.concatenate([a, b]) for a, b in zip((boards, side, moves), more))
    return pack_boards(boards, m, n), ((moves << 1) | side).astype(np.uint32)


if __name__ == "__main__":
    out = {}
    for name, (m, n, k, rows, plies, late) in CASES.items():
        out[name + "_planes"], out[name + "_meta"] = starts(m, n, k, rows, plies, late)
        print(name, "move counts", (out[name + "_meta"] >> 1).tolist())
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "search_selfplay_async_starts.npz"), **out)
