"""The inputs the tests of the PUCT player that keeps its tree share (tests/test_gpu_puct_reuse.py and the cases modules
and CPU tests of the later forms): the dyadic evaluator in numpy, the rows a sequence starts on, and the next roots one
or two plies on.  numpy alone, so that a cases module need not import a GPU test."""
import numpy as np

from playout_rule import has_run
from tactical_rule import random_positions


def prior_table(C, mult=1):
    """a per-cell table of powers of two (exact in bfloat16 too), peaked on the lowest cells (``mult`` = 1): trees narrow
    enough for a child to own a subtree worth carrying, and in which the second mover's lowest free cell was searched"""
    a = (np.arange(C) * mult) % C
    return (2.0 ** -(np.minimum(a // 4, 7) + 1 + max(int(np.ceil(np.log2(C))) - 4, 0))).astype(np.float32)


def value_weights(C):
    return (np.arange(C) % 7 + 1).astype(np.float32)


def exact_np(C, J=None):
    """a deterministic function of the leaf: the table on its legal cells, a value k / 8 from a weighted stone difference;
    with ``J``, every call 0 (mod J + 1) -- the roots' -- answers with another table"""
    tables, weights = (prior_table(C), prior_table(C, 11)), value_weights(C)
    calls = [0]

    def evaluate(leaf_obs, leaf_mask):
        table = tables[1 if J is not None and calls[0] % (J + 1) == 0 else 0]
        calls[0] += 1
        o = leaf_obs.reshape(len(leaf_obs), 2, -1)
        s = ((o[:, 0] - o[:, 1]) * weights).sum(axis=1)
        return leaf_mask * table, ((np.mod(s, 9) - 4) / 8).astype(np.float32)

    return evaluate


def start(m, n, k, rows, seed):
    """the rows a sequence starts on: an empty board, then positions a few stones in"""
    obs = random_positions(m, n, k, rows, np.random.default_rng(seed), max_fill=0.25)
    obs[0] = 0
    return obs


def place(obs, i, cell, k):
    """row i's side to move plays ``cell``; the row as its next side to move sees it, or an empty board when that ended
    the game.  Returns whether it did."""
    _, m, n = obs[i].shape
    me = obs[i, 0].reshape(-1).copy()
    assert me[cell] == 0 and obs[i, 1].reshape(-1)[cell] == 0
    me[cell] = 1
    other = obs[i, 1].copy()
    ended = bool(has_run(me.reshape(1, m, n) != 0, k)[0]) or bool((me + other.reshape(-1)).all())
    obs[i, 0], obs[i, 1] = (0, 0) if ended else (other, me.reshape(m, n))
    return ended


def advance(obs, actions, k, distance, resets):
    """the next roots: every row's action played and, with ``distance`` 2, the lowest free cell by a second mover;
    ``resets[i]`` counts the games of row i that ended"""
    obs = obs.copy()
    for i in range(len(obs)):
        ended = place(obs, i, int(actions[i]), k)
        if not ended and distance == 2:
            free = np.flatnonzero((obs[i, 0] + obs[i, 1]).reshape(-1) == 0)
            ended = place(obs, i, int(free[0]), k)
        resets[i] += ended
    return obs
