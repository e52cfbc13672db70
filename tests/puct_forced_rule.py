"""numpy restatement of the PUCT player with forced playouts and policy target pruning (test helper; the rule is stated
in include/mnk_hip.h, mnk_puct_step_forced).  ``select`` is ``puct_fpu_rule.select`` (which is ``puct_solver_rule._select``
when ``fpu`` is None) with one more class of candidate at the root: a free cell whose child has a stored visit, is not
proven LOSS and has ``n'^2 < k * P * S'`` is FORCED, and where a cell is FORCED only those are candidates.  ``prune`` is
the pruning of a tree's root, by the rule's own walk over j.  Trees, rounds, virtual visits, proofs, the backup and the
draw of the move are ``puct_solver_rule``'s; ``ForcedPuct`` equals ``FpuPuct`` with ``forced=None``.

The classes call ``puct_solver_rule._select`` by name, so the selection is swapped in for the length of a call
(``forced_selection``), as ``puct_fpu_rule.fpu_selection`` does."""
import contextlib
import functools

import numpy as np

import puct_ops
import puct_solver_rule as ps
from oracle import philox
from playout_rule import has_run
from puct_fpu_rule import FpuPuct, as_pair, untried_q
from search_selfplay_async_opts_rule import AsyncOptsRule, adjusted_counts
from search_selfplay_rule import STREAM_SELFPLAY, pick_by_visits

f32 = np.float32


def short_of_floor(tree, legal, kids, vl, k_forced):
    """bool over ``legal`` (the root's free cells, ``kids`` their children or None): the cells whose child has a stored
    visit and n'^2 < k * P * S' -- clauses (1) and (3) of the rule, whatever the child's proof"""
    S = f32(tree.n[0] + vl.get(0, 0) - 1)
    out = np.zeros(len(legal), bool)
    for j, (a, ch) in enumerate(zip(legal, kids)):
        if ch is None or tree.n[ch] == 0:
            continue
        n1 = f32(tree.n[ch] + vl.get(ch, 0))
        out[j] = f32(n1 * n1) < puct_ops.forcing_bound(k_forced, tree.prior[0][a], S)
    return out


def forced_cells(tree, legal, kids, vl, solver, k_forced):
    """bool over ``legal``: which are FORCED -- ``short_of_floor`` and, with the solver, not proven LOSS (clause (2))"""
    out = short_of_floor(tree, legal, kids, vl, k_forced)
    if solver:
        out &= np.array([ch is None or tree.proof[ch] != ps.LOSS for ch in kids], bool)
    return out


def select(tree, root, m, n, k, c, vl, nodes0, solver, fpu=None, forced=None, log=None, shunned=None):
    """``puct_fpu_rule.select`` (``fpu`` None: ``puct_solver_rule._select``) with the FORCED class at the root.  ``forced``:
    None or k, or a callable of the tree that returns one of those (the per-row loop's "this ply forces"); ``log`` (a
    list) takes, for every root selection with a FORCED cell, (the cell taken, the cell the plain score would have taken);
    ``shunned`` (a list) takes, for every root selection with the solver at which a child proven LOSS is short of its floor
    -- FORCED but for clause (2) --, (those cells, the cell taken, whether some free cell's child is not proven LOSS)"""
    if callable(forced):
        forced = forced(tree)
    pos = root.copy()
    v, d, path = 0, 0, [0]
    while True:
        legal = np.flatnonzero(~(pos[0] | pos[1]))
        kids = [tree.kids[v].get(int(a)) for a in legal]
        qu = f32(0)
        if fpu is not None:
            seen = np.array([ch is not None and tree.n[ch] + vl.get(ch, 0) > 0 for ch in kids], bool)
            qu = untried_q(tree, v, tree.prior[v][legal[seen]], fpu)
        lost = ()  # the root's cells proven LOSS that are short of their floor (counted ahead of the filter below)
        if solver and v == 0 and forced is not None:
            short = short_of_floor(tree, legal, kids, vl, forced)
            lost = tuple(int(a) for a, ch, sh in zip(legal, kids, short) if sh and tree.proof[ch] == ps.LOSS)
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
        if v == 0 and forced is not None:
            on = forced_cells(tree, legal, kids, vl, solver, forced)
            if on.any():
                plain = a
                a = int(legal[on][int(np.argmax(s[on]))])
                if log is not None:
                    log.append((a, plain))
            if lost and shunned is not None:
                shunned.append((lost, a, bool(held.any())))
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
def forced_selection(fpu, forced, log=None, shunned=None):
    """while it is open, the classes built on ``puct_solver_rule._select`` select with ``select`` above"""
    saved = ps._select
    ps._select = functools.partial(select, fpu=fpu, forced=forced, log=log, shunned=shunned)
    try:
        yield
    finally:
        ps._select = saved


def score(tree, a, j, c):
    """s_a(j) of the root's child through cell a"""
    ch = tree.kids[0][a]
    q = np.array([f32(tree.w[ch]) / f32(tree.n[ch])], f32)
    return puct_ops.score(q, f32(c), tree.prior[0][[a]], puct_ops.sqrt(tree.n[0]), np.array([j], np.int64))[0]


def floor_of(tree, a, n1, k_forced):
    """min(n'_a, F_a): F_a the least integer F >= 0 with fl(F * F) >= t_a"""
    t = puct_ops.floor_bound(k_forced, tree.prior[0][a], f32(tree.n[0] - 1))
    for F in range(n1):
        if f32(f32(F) * f32(F)) >= t:
            return F
    return n1


def prune(tree, counts, c, k_forced, info=None):
    """the pruned counts n'' (int64 [C]) of the root of ``tree`` from n' = ``counts``, by the rule's walk.  ``info`` (a
    dict) takes c*, s* and, per pruned cell, (lo, n', n'' before the single-visit rule)"""
    out = np.asarray(counts, np.int64).copy()
    if out.max() == 0:
        return out
    cstar = int(np.argmax(out))  # (the first maximum: ties to the lowest cell)
    sstar = score(tree, cstar, int(out[cstar]), c)
    if info is not None:
        info.update(cstar=cstar, sstar=sstar, cells={})
    for a in np.flatnonzero(out):
        a, n1 = int(a), int(out[a])
        if a == cstar or tree.prior[0][a] <= 0:
            continue
        lo = n1 - floor_of(tree, a, n1, k_forced)
        j = next((j for j in range(lo, n1 + 1) if score(tree, a, j, c) < sstar), n1)
        if info is not None and j != n1:
            info["cells"][a] = (lo, n1, j)
        out[a] = 0 if j == 1 and n1 > 1 else j
    return out


def root_counts(tree, C, solver):
    """(n' int64 [C], whether the solver keeps the WIN children alone) of a tree's root"""
    visits, kinds = np.zeros(C, np.int64), np.zeros(C, np.int64)
    for a, ch in tree.kids[0].items():
        visits[a], kinds[a] = tree.n[ch], tree.proof[ch]
    if not solver:
        return visits, False
    adjusted = adjusted_counts(visits, kinds)
    wins_only = bool((kinds == ps.WIN).any()) and bool(np.where(kinds == ps.WIN, visits, 0).any())
    return adjusted, wins_only


class ForcedPuct(FpuPuct):
    """``FpuPuct`` (its arguments) with ``forced``: None or k.  ``act`` returns the pruned ``visits`` and the move drawn
    from them; ``raw_visits`` keeps n', ``picks`` the (taken, plain) cells of the root selections with a FORCED cell,
    ``shunned`` ``select``'s record of the children proven LOSS that clause (2) kept from being forced, and
    ``pruned_info`` the per-row ``info`` of ``prune``"""

    def __init__(self, *args, forced=None, **kw):
        super().__init__(*args, **kw)
        self.forced = forced
        self.raw_visits, self.picks, self.shunned, self.pruned_info = None, [], [], []

    def act(self, obs, step=0, deterministic=False):
        if self.forced is None:
            return super().act(obs, step=step, deterministic=deterministic)
        self.picks, self.shunned, self.pruned_info = [], [], []
        with forced_selection(self.fpu, self.forced, self.picks, self.shunned):
            actions, visits, root_value, carried, proof = ps.SolverPuct.act(self, obs, step=step,
                                                                            deterministic=deterministic)
        N, C = visits.shape
        self.raw_visits = visits.copy()
        env = np.uint64(self.env_id0) + np.arange(N, dtype=np.uint64)
        x = philox.rand_u32(self.seed, env, step, philox.STREAM_SAMPLE)
        if deterministic:
            x = np.zeros(N, np.uint64)
        for i in range(N):
            info = {}
            self.pruned_info.append(info)
            counts, wins_only = root_counts(self.trees[i], C, self.solver)
            assert np.array_equal(counts, self.raw_visits[i])
            if wins_only or not self.live[i] or counts.max() == 0:
                continue
            visits[i] = prune(self.trees[i], counts, self.c, self.forced, info)
            S = np.flatnonzero(visits[i] == visits[i].max())
            if self.temperature == 1 and not deterministic:
                r = philox.mulhi32(x[i], int(visits[i].sum()))
                actions[i] = int(np.flatnonzero(np.cumsum(visits[i]) > r)[0])
            else:
                actions[i] = int(S[philox.mulhi32(x[i], len(S))])
        return actions, visits, root_value, carried, proof


class AsyncOptsForcedRule(AsyncOptsRule):
    """``AsyncOptsRule`` with ``fpu`` and ``forced``: a ply FORCES iff it is full or ``noise_on_fast`` is set -- a function
    of (row, the row's ply count), asked for where it is needed.  ``plies`` records, per ply played, (row, ply, full,
    forces, the root bool [2, C], n' int64 [C], the counts played from, the move)"""

    def __init__(self, *args, fpu=None, forced=None, **kw):
        self.fpu, self.forced = as_pair(fpu), forced
        self.picks, self.shunned, self.plies = [], [], []
        super().__init__(*args, **kw)

    def forces(self, i):
        """whether row i's current ply forces"""
        return self.forced is not None and (self.is_full(i) or self.noise_on_fast)

    def _forced_of(self, tree):
        """``select``'s ``forced`` of the row whose tree this is"""
        i = next(i for i, t in enumerate(self.trees) if t is tree)
        return self.forced if self.forces(i) else None

    def _ply(self, i, visits, full):
        raw = np.asarray(visits, np.int64).copy()
        forces = self.forces(i)  # (before the ply: its count is the row's still)
        if forces:
            _, wins_only = root_counts(self.trees[i], self.C, self.solver)
            if not wins_only and raw.max() > 0:
                visits = prune(self.trees[i], raw, self.c, self.forced)
        root, p, g = self.roots[i].copy(), int(self.row_plies[i]), int(self.moves[i])
        played = super()._ply(i, visits, full)
        if played:
            counts = np.where(root[0] | root[1], 0, np.clip(visits, 0, 65535))
            x = philox.rand_u32(self.seed, np.array([self.env_id0 + i], np.uint64), p, STREAM_SELFPLAY)[0]
            self.plies.append((i, p, full, forces, root, raw, counts, pick_by_visits(counts, x, g < self.temp_plies)))
        return played

    def advance(self, priors, values, root_priors=None):
        with forced_selection(self.fpu, self._forced_of, self.picks, self.shunned):
            return super().advance(priors, values, root_priors=root_priors)
