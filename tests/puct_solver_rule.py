"""numpy restatement of the PUCT player that proves wins, draws and losses in its tree (test helper; the rule is stated
in include/mnk_hip.h, mnk_puct_step_solver), and a brute-force negamax to hold its proofs against.  The player is
``puct_search_rule.PuctSearch`` with ``solver`` on: the proofs, the selection that leaves out the children proven LOSS and
ends in a child with a proof, the backup that proves what it can along the path, the adjusted counts the move is made
from and a proven root that selects nothing more are stated there."""
import functools

import numpy as np

from puct_search_rule import DRAW, LOSS, PROOF_UNKNOWN, WIN, _VALUE, PuctSearch  # noqa: F401 (the names the tests know)


class SolverPuct(PuctSearch):
    """``PuctSearch`` (its arguments) with ``solver`` on unless it is turned off"""

    def __init__(self, *args, solver=True, **kw):
        super().__init__(*args, solver=solver, **kw)


def puct_solver(obs, k, iterations, c, evaluator, L=1, seed=0, step=0, env_id0=0, temperature=0, deterministic=False,
                leaves=None, solver=True):
    """one act of a fresh ``SolverPuct``: (actions, visits, root_value, proof)"""
    rule = SolverPuct(k, iterations, c, evaluator, L, seed=seed, env_id0=env_id0, temperature=temperature, leaves=leaves,
                      solver=solver)
    out = rule.act(obs, step=step, deterministic=deterministic)
    return out[0], out[1], out[2], out[4]


# ----------------------------------------------------------------------------- brute force
@functools.lru_cache(maxsize=None)
def _lines(m, n, k):
    """every run of k cells in a row, column or diagonal of the board, as a bit set over the cells"""
    out = []
    for r in range(m):
        for c in range(n):
            for dr, dc in ((0, 1), (1, 0), (1, 1), (1, -1)):
                cells = [(r + j * dr, c + j * dc) for j in range(k)]
                if all(0 <= y < m and 0 <= x < n for y, x in cells):
                    out.append(sum(1 << (y * n + x) for y, x in cells))
    return tuple(out)


def _bits(plane):
    return sum(1 << int(a) for a in np.flatnonzero(plane))


def _after(me, other, a, m, n, k, value):
    """the value for the mover of playing cell a: me, other = the mover's and the other side's stones as bit sets"""
    mine = me | (1 << a)
    if any(mine & line == line for line in _lines(m, n, k)):
        return 1
    if (mine | other) == (1 << m * n) - 1:
        return 0
    return -value(other, mine)


def _negamax(m, n, k):
    @functools.lru_cache(maxsize=None)
    def value(me, other):
        return max(_after(me, other, a, m, n, k, value) for a in range(m * n) if not (me | other) >> a & 1)

    return value


def negamax(pos, m, n, k):
    """the game-theoretic value (+1 win, 0 draw, -1 loss) of ``pos`` (bool [2, C], plane 0 = the side to move; no run on
    the board, a free cell) for its side to move, by exhaustive search; for positions of at most 7 free cells"""
    assert 1 <= (~(pos[0] | pos[1])).sum() <= 7
    return _negamax(m, n, k)(_bits(pos[0]), _bits(pos[1]))


def value_after(pos, a, m, n, k):
    """the value for the side to move of ``pos`` of playing the free cell ``a``"""
    assert not pos[0][a] and not pos[1][a] and (~(pos[0] | pos[1])).sum() <= 8
    return _after(_bits(pos[0]), _bits(pos[1]), int(a), m, n, k, _negamax(m, n, k))
