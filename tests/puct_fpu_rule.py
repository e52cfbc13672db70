"""numpy restatement of the PUCT player with first-play urgency (test helper; the rule is stated in include/mnk_hip.h,
mnk_puct_step_fpu).  ``select`` is ``puct_solver_rule._select`` with one change: a free cell without a visit scores with
``q = max(q_v - r * mass, -1)`` in the place of 0, where ``q_v`` is the node's own mean value, ``mass`` the square root of
the prior mass of its visited cells (summed as 32-bit fixed-point integers) and ``r`` the reduction -- ``fpu_root`` at the
root, ``fpu`` below it.  Trees, rounds, virtual visits, proofs, the backup and the move are ``puct_solver_rule``'s, whose
``SolverPuct`` ``FpuPuct`` equals with ``fpu=None``; the per-row self-play rules are ``AsyncOptsRule`` / ``AsyncKeepRule``
with that selection.

Those classes call ``puct_solver_rule._select`` by name, so the selection is swapped in for the length of a call
(``fpu_selection``) instead of copying their loops."""
import contextlib
import functools

import numpy as np

import puct_ops
import puct_solver_rule as ps
from playout_rule import has_run
from search_selfplay_async_keep_rule import AsyncKeepRule
from search_selfplay_async_opts_rule import AsyncOptsRule


def as_pair(fpu):
    """None, or (fpu, fpu_root) as float32: a number r stands for (r, r)"""
    if fpu is None:
        return None
    r, r0 = (fpu, fpu) if np.isscalar(fpu) else fpu
    return np.float32(r), np.float32(r0)


def mass_of(priors):
    """fl32(sqrt(T * 2^-32)), T = the sum over ``priors`` (float32, the visited free cells') of the prior clipped to
    [0, 1], times 2^32, truncated: Python integers, so no order of summation can matter"""
    clipped = np.minimum(np.maximum(np.asarray(priors, np.float32), np.float32(0)), np.float32(1))
    T = sum(int(np.float64(p) * 4294967296.0) for p in clipped)  # (p * 2^32 is exact in f64; int() truncates)
    return np.float32(np.sqrt(np.float64(T) * 2.0 ** -32))


def untried_q(tree, v, visited_priors, fpu):
    """the q of node v's free cells without a visit; ``fpu`` = (fpu, fpu_root) as float32"""
    qv = np.float32(-np.float32(tree.w[v])) / np.float32(tree.n[v])  # (the stored counts: no virtual visits)
    r = fpu[1] if v == 0 else fpu[0]
    return np.maximum(puct_ops.fpu_q(qv, r, mass_of(visited_priors)), np.float32(-1))


def select(tree, root, m, n, k, c, vl, nodes0, solver, fpu):
    """``puct_solver_rule._select`` with first-play urgency"""
    pos = root.copy()
    v, d, path = 0, 0, [0]
    while True:
        legal = np.flatnonzero(~(pos[0] | pos[1]))
        kids = [tree.kids[v].get(int(a)) for a in legal]
        # the mass is over every free cell with a visit (virtual ones included), the children proven LOSS too
        seen = np.array([ch is not None and tree.n[ch] + vl.get(ch, 0) > 0 for ch in kids], bool)
        qu = untried_q(tree, v, tree.prior[v][legal[seen]], fpu)
        if solver:
            held = np.array([ch is None or tree.proof[ch] != ps.LOSS for ch in kids])
            if held.any():
                legal, kids = legal[held], [ch for ch, h in zip(kids, held) if h]
        va = np.array([0 if ch is None else vl.get(ch, 0) for ch in kids], np.int64)
        na = np.array([0 if ch is None else tree.n[ch] for ch in kids], np.int64) + va
        wa = np.array([0 if ch is None else tree.w[ch] for ch in kids], np.float32) + (-va.astype(np.float32))
        q = np.where(na > 0, wa / np.maximum(na, 1).astype(np.float32), qu).astype(np.float32)
        s = puct_ops.score(q, c, tree.prior[v][legal], puct_ops.sqrt(tree.n[v] + vl.get(v, 0)), na)
        a = int(legal[int(np.argmax(s))])  # (the first maximum: ties go to the lowest cell)
        side = d & 1
        pos[side, a] = True
        d += 1
        if a not in tree.kids[v]:
            won = bool(has_run(pos[side].reshape(1, m, n), k)[0])
            full = bool((pos[0] | pos[1]).all())
            ch = tree.add(a, 1 if won else (2 if full else 0))
            tree.kids[v][a] = ch
            path.append(ch)
            return path, pos, d, tree.term[ch]
        ch = tree.kids[v][a]
        path.append(ch)
        kind = tree.proof[ch] if solver else tree.term[ch]
        if kind:
            return path, pos, d, kind
        if ch >= nodes0:
            return None
        v = ch


@contextlib.contextmanager
def fpu_selection(fpu):
    """while it is open, the classes built on ``puct_solver_rule._select`` select with first-play urgency (``fpu``: None
    -- nothing changes -- or (fpu, fpu_root))"""
    if fpu is None:
        yield
        return
    saved = ps._select
    ps._select = functools.partial(select, fpu=fpu)
    try:
        yield
    finally:
        ps._select = saved


class FpuPuct(ps.SolverPuct):
    """``SolverPuct`` (its arguments; ``solver`` defaults to False here) with ``fpu``: None, a number or (fpu, fpu_root)"""

    def __init__(self, *args, fpu=None, solver=False, **kw):
        super().__init__(*args, solver=solver, **kw)
        self.fpu = as_pair(fpu)

    def act(self, obs, step=0, deterministic=False):
        with fpu_selection(self.fpu):
            return super().act(obs, step=step, deterministic=deterministic)


class AsyncOptsFpuRule(AsyncOptsRule):
    def __init__(self, *args, fpu=None, **kw):
        self.fpu = as_pair(fpu)
        super().__init__(*args, **kw)

    def advance(self, priors, values, root_priors=None):
        with fpu_selection(self.fpu):
            return super().advance(priors, values, root_priors=root_priors)


class AsyncKeepFpuRule(AsyncKeepRule):
    def __init__(self, *args, fpu=None, **kw):
        self.fpu = as_pair(fpu)
        super().__init__(*args, **kw)

    def advance(self, priors, values, root_priors=None):
        with fpu_selection(self.fpu):
            return super().advance(priors, values, root_priors=root_priors)
