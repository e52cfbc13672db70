"""numpy restatement of search self-play with per-row budgets and a Gumbel root (test helper; the rule is stated in
include/mnk_hip.h, mnk_search_selfplay_advance_gumbel).

``AsyncGumbelRule`` is an ``AsyncSelfPlayRule`` (the games, the ring, the trees, the budget word) whose roots are
tests/puct_gumbel_rule.py's: ``gumbel_scores`` at step = the row's ply count when a fresh tree's root is backed up, the
root's cell by ``_pick`` with the schedule table of the ply's budget, the walk below it by ``_walk``, and at the end of a
ply the move by ``_pick`` among the cells of the most visits and -- on a full ply -- ``improved_policy`` quantised by
``ring_counts``.  Nothing of those is restated here.

``advance(priors, values, gscore=None)``: ``gscore`` (float32 [N, C]) optionally hands in the scores "as the kernel wrote
them"; the rows that back up a root's evaluation in this launch then search with those instead of the rule's own, so that
one ulp in a logarithm cannot send the two searches different ways.  What the rule itself computes for those rows is kept
in ``gscore_wanted`` ({row: float32 [C]} of the last launch) to compare with.

The helper keeps a log of what it went through (``log``: one dict per ply played, and ``root_rows``: the schedule row m' of
every root it searched), which the CPU test uses to show that the GPU tests' seeds and shapes reach every branch.
"""
import numpy as np

from oracle.packing import pack_cells
from playout_rule import has_run
from puct_gumbel_rule import _pick, _root_stats, _walk, gumbel_scores, improved_policy, ring_counts, schedule
from puct_rule import _backup, _canonical
from search_selfplay_async_rule import AsyncSelfPlayRule
from search_selfplay_rule import ERR_VISITS, Z_UNKNOWN


class AsyncGumbelRule(AsyncSelfPlayRule):
    def __init__(self, m, n, k, N, T, full, fast, threshold, c, seed, considered, c_visit=50.0, c_scale=0.5,
                 gumbel_scale=1.0, env_id0=0):
        self.considered, self.gumbel_scale = int(considered), gumbel_scale
        self.c_visit, self.c_scale = np.float32(c_visit), np.float32(c_scale)
        self.tables = {True: schedule(self.considered, full), False: schedule(self.considered, fast)}
        self.log = []        # one dict per ply played: row, ply, full, free cells, won, drawn, ring slot
        self.root_rows = []  # (m' = min(considered, F), budget) of every root whose evaluation was backed up
        self.gscore_wanted = {}
        super().__init__(m, n, k, N, T, full, fast, threshold, c, 0, seed, env_id0)

    def begin(self):
        self.gscore = np.full((self.N, self.C), np.nan, np.float32)
        self.vroot = np.zeros(self.N, np.float32)
        return super().begin()

    def _ply_move(self, i, a, policy, full):
        """one ply of one row from the search's own move: mnk_search_selfplay_step_moves's body with the row's ply"""
        m, n, k, T, C = self.m, self.n, self.k, self.T, self.C
        p = int(self.row_plies[i])
        t = p % T
        s = self.side[i]
        me, other = self.boards[i, s].copy(), self.boards[i, 1 - s].copy()
        occ = me | other
        if not 0 <= a < C or occ[a]:
            return False
        self.ring_planes[t, 0, :, i] = pack_cells(me[None], m, n)[:, 0]
        self.ring_planes[t, 1, :, i] = pack_cells(other[None], m, n)[:, 0]
        self.ring_visits[t, i] = ring_counts(policy, ~occ) if full else 0
        self.ring_z[t, i] = Z_UNKNOWN
        if full:
            self.full_records += 1
        else:
            self.fast_records += 1
        g = int(self.moves[i])
        self.boards[i, s, a] = True
        win = bool(has_run(self.boards[i, s].reshape(1, m, n), k)[0])
        done = win or g + 1 >= C
        self.moves[i] = g + 1
        self.side[i] = 1 - s
        self.log.append({"row": i, "ply": p, "full": bool(full), "free": int((~occ).sum()), "won": win,
                         "drawn": done and not win, "slot": t})
        if done:
            for d in range(min(g + 1, T)):
                self.ring_z[(t - d) % T, i] = (1 if d % 2 == 0 else -1) if win else 0
            self.stats += [1, int(win and s == 0), int(win and s == 1), int(not win), g + 1]
            self.boards[i] = False
            self.moves[i] = 0
            self.side[i] = 0
        self.row_plies[i] = p + 1
        self.plies_max = max(self.plies_max, p + 1)
        return True

    def advance(self, priors, values, gscore=None):
        """one launch: (leaf_obs f32 [N, 2, m, n], leaf_mask bool [N, C], fresh u8 [N])"""
        N, C, m, n = self.N, self.C, self.m, self.n
        priors = np.asarray(priors, np.float32).reshape(N, C)
        values = np.asarray(values, np.float32).reshape(N)
        leaf_obs = np.zeros((N, 2, m, n), np.float32)
        leaf_mask = np.zeros((N, C), bool)
        fresh = np.zeros(N, np.uint8)
        self.gscore_wanted = {}
        for i in range(N):
            tree, root = self.trees[i], self.roots[i]
            pos, d = root, 0
            if not self.live[i]:  # a root without a legal cell: reported, left alone, shown again
                self.errors.append((ERR_VISITS, i))
            else:
                full = self.is_full(i)
                budget = self.full if full else self.fast
                free = np.flatnonzero(~(root[0] | root[1]))
                if self.pending[i]:
                    if len(self.paths[i]) == 1:  # evaluation 0: the pending leaf is the root of a fresh tree
                        want, _ = gumbel_scores(priors[i][None], ~(root[0] | root[1])[None], self.gumbel_scale, self.seed,
                                                int(self.row_plies[i]), self.env_id0 + i)
                        self.gscore_wanted[i] = want[0]
                        self.gscore[i] = want[0] if gscore is None else np.asarray(gscore[i], np.float32)
                        self.vroot[i] = values[i]
                        self.root_rows.append((min(self.considered, len(free)), budget))
                    _backup(tree, self.paths[i], priors[i], values[i])
                    self.pending[i] = False
                it = tree.n[0] - 1
                if it < budget:
                    want = int(self.tables[full][min(self.considered, len(free)), it])
                    first = _pick(tree, free, self.gscore[i], want, self.c_visit, self.c_scale)
                    self.paths[i], pos, d = _walk(tree, root, m, n, self.k, self.c, first)
                    self.pending[i] = True
                else:
                    na, _, q = _root_stats(tree, free)
                    a = _pick(tree, free, self.gscore[i], None, self.c_visit, self.c_scale)
                    policy = (improved_policy(tree.prior[0], free, na, q, self.vroot[i], self.c_visit, self.c_scale)
                              if full else None)
                    if self._ply_move(i, a, policy, full):
                        self._fresh(i)
                        pos = self.roots[i]
                        fresh[i] = 1
                    else:
                        self.errors.append((ERR_VISITS, i))
            leaf_obs[i] = _canonical(pos, d, m, n)
            leaf_mask[i] = ~(pos[0] | pos[1])
        return leaf_obs, leaf_mask, fresh
