"""Writes tests/golden/search_selfplay_async_starts.npz: env states near the end of games on 12x12x5 and 19x19x5, the
start of the large-board cases of tests/test_gpu_search_selfplay_async.py (a search of a few iterations does not finish a
game on such a board from the empty position within a test's rounds).  The positions come from the oracle's uniformly
random play (oracle.rollout.random_rollout on an OracleVectorEnv): of 128 games after PLIES plies, the rows whose side to
move can complete a run at once, the most advanced first.

usage: python tests/golden/make_golden_search_selfplay_async.py   (from the repository root; needs no GPU)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from oracle.env_torch import OracleVectorEnv  # noqa: E402
from oracle.packing import pack_boards  # noqa: E402
from oracle.rollout import random_rollout  # noqa: E402
from tactical_rule import completions  # noqa: E402

CASES = {"12x12x5": (12, 12, 5, 3, 70), "19x19x5": (19, 19, 5, 3, 150)}  # m, n, k, rows, plies of random play


def starts(m, n, k, rows, plies, seed=0, envs=128):
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
    return pack_boards(boards[order], m, n), ((moves[order] << 1) | side[order]).astype(np.uint32)


if __name__ == "__main__":
    out = {}
    for name, (m, n, k, rows, plies) in CASES.items():
        out[name + "_planes"], out[name + "_meta"] = starts(m, n, k, rows, plies)
        print(name, "move counts", (out[name + "_meta"] >> 1).tolist())
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "search_selfplay_async_starts.npz"), **out)
