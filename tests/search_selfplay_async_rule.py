"""numpy restatement of search self-play with per-row budgets (test helper; the rule is stated in include/mnk_hip.h,
mnk_search_selfplay_advance).

``AsyncSelfPlayRule`` is a ``SelfPlayRule`` (the games, the ring, the statistics) with one ``puct_rule`` tree per row and
the plies every row has played (``row_plies``).  ``begin`` sets every row's tree up on its current position, as
mnk_puct_begin does, and returns the roots; ``advance(priors, values)`` is one launch of every row: the backup of the
row's pending evaluation, then either the next selection or -- when the budget of the row's ply, a function of (seed, row
id, the row's ply) alone, is spent -- the ply, its ring record, the outcome labels, the reset and a fresh tree on the
position reached.  It returns the leaves and ``fresh``.
"""
import numpy as np

from oracle import philox
from oracle.packing import pack_cells
from playout_rule import has_run
from puct_rule import _backup, _canonical, _select, _Tree
from search_selfplay_rule import ERR_VISITS, STREAM_SELFPLAY, Z_UNKNOWN, SelfPlayRule, pick_by_visits

STREAM_BUDGET = 9


def budget_word(seed, row_id, p):
    """the u32 that decides whether ply p of the row is searched with the full budget"""
    return int(philox.rand_u32(seed, np.array([row_id], np.uint64), p, STREAM_BUDGET)[0])


def exact_np(C):
    """the dyadic evaluator of the GPU tests in numpy: per-cell priors on the legal cells, a value from stone counts"""
    table = (((np.arange(C) * 37) % 16 + 1) / 16).astype(np.float32)

    def evaluate(leaf_obs, leaf_mask):
        cnt = leaf_obs.astype(np.float32).reshape(len(leaf_obs), 2, -1).sum(axis=2)
        return leaf_mask.astype(np.float32) * table, ((np.remainder(cnt[:, 0] - 2 * cnt[:, 1], 5) - 2) / 4).astype(np.float32)

    return evaluate


class AsyncSelfPlayRule(SelfPlayRule):
    def __init__(self, m, n, k, N, T, full, fast, threshold, c, temp_plies, seed, env_id0=0):
        super().__init__(m, n, k, N, T)
        assert 1 <= fast <= full and 0 <= threshold <= 2 ** 32
        self.full, self.fast, self.threshold = full, fast, threshold
        self.c, self.temp_plies, self.seed, self.env_id0 = np.float32(c), temp_plies, seed, env_id0
        self.row_plies = np.zeros(N, np.int64)
        self.plies_max = 0
        self.full_records = 0  # ring records written with visits / without (the counters are the helper's own)
        self.fast_records = 0
        self.begin()

    # ---- the trees
    def _root(self, i):
        s = self.side[i]
        return np.stack([self.boards[i, s], self.boards[i, 1 - s]])

    def _fresh(self, i):
        self.roots[i] = self._root(i)
        self.trees[i] = _Tree()
        self.paths[i] = [0]
        self.pending[i] = True
        self.live[i] = not (self.roots[i][0] | self.roots[i][1]).all()

    def begin(self):
        """every row's search starts afresh on its current position: (leaf_obs, leaf_mask) of the roots"""
        N = self.N
        self.roots = np.zeros((N, 2, self.C), bool)
        self.trees, self.paths = [None] * N, [None] * N
        self.pending, self.live = np.zeros(N, bool), np.zeros(N, bool)
        for i in range(N):
            self._fresh(i)
        return self.view()

    def is_full(self, i, p=None):
        p = int(self.row_plies[i]) if p is None else p
        return budget_word(self.seed, self.env_id0 + i, p) < self.threshold

    # ---- one ply of one row: SelfPlayRule.step's body with the row's own ply in the place of the global one
    def _ply(self, i, visits, full):
        m, n, k, T, C = self.m, self.n, self.k, self.T, self.C
        p = int(self.row_plies[i])
        t = p % T
        x = philox.rand_u32(self.seed, np.array([self.env_id0 + i], np.uint64), p, STREAM_SELFPLAY)[0]
        s = self.side[i]
        me, other = self.boards[i, s].copy(), self.boards[i, 1 - s].copy()
        na = np.where(me | other, 0, np.clip(visits, 0, 65535))
        if na.max() == 0:
            return False
        self.ring_planes[t, 0, :, i] = pack_cells(me[None], m, n)[:, 0]
        self.ring_planes[t, 1, :, i] = pack_cells(other[None], m, n)[:, 0]
        self.ring_visits[t, i] = na if full else 0
        self.ring_z[t, i] = Z_UNKNOWN
        if full:
            self.full_records += 1
        else:
            self.fast_records += 1
        g = int(self.moves[i])
        a = pick_by_visits(na, x, g < self.temp_plies)
        self.boards[i, s, a] = True
        win = bool(has_run(self.boards[i, s].reshape(1, m, n), k)[0])
        done = win or g + 1 >= C
        self.moves[i] = g + 1
        self.side[i] = 1 - s
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

    def advance(self, priors, values):
        """one launch: (leaf_obs f32 [N, 2, m, n], leaf_mask bool [N, C], fresh u8 [N])"""
        N, C, m, n = self.N, self.C, self.m, self.n
        priors = np.asarray(priors, np.float32).reshape(N, C)
        values = np.asarray(values, np.float32).reshape(N)
        leaf_obs = np.zeros((N, 2, m, n), np.float32)
        leaf_mask = np.zeros((N, C), bool)
        fresh = np.zeros(N, np.uint8)
        for i in range(N):
            tree, root = self.trees[i], self.roots[i]
            pos, d = root, 0
            played = False
            if not self.live[i]:  # a root without a legal cell: reported, left alone, shown again
                self.errors.append((ERR_VISITS, i))
            else:
                if self.pending[i]:
                    _backup(tree, self.paths[i], priors[i], values[i])
                    self.pending[i] = False
                full = self.is_full(i)
                if tree.n[0] - 1 < (self.full if full else self.fast):
                    self.paths[i], pos, d = _select(tree, root, m, n, self.k, self.c)
                    self.pending[i] = True
                else:
                    visits = np.zeros(C, np.int64)
                    for a, ch in tree.kids[0].items():
                        visits[a] = tree.n[ch]
                    played = self._ply(i, visits, full)
                    if played:
                        self._fresh(i)
                        pos = self.roots[i]
                        fresh[i] = 1
                    else:
                        self.errors.append((ERR_VISITS, i))
            leaf_obs[i] = _canonical(pos, d, m, n)
            leaf_mask[i] = ~(pos[0] | pos[1])
        return leaf_obs, leaf_mask, fresh
