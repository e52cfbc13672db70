"""numpy restatement of search self-play with per-row budgets and several leaves per evaluator call (test helper; the
rule is stated in include/mnk_hip.h, mnk_search_selfplay_advance_leaves).

``AsyncLeavesRule`` is an ``AsyncOptsRule`` whose rows hold L slots -- per row a list of (path, kind) or None for a void
slot -- and a counter of the simulations the row's current ply has been offered (``row_sims``).  A launch backs the row's
pending slots up in slot order (``puct_search_rule.backup``), then either ends the ply (the counter has reached the ply's
budget, or the root is proven) or lets ``s = min(L, budget - row_sims)`` slots select one after the other under the virtual
visits of the slots before them (``puct_search_rule.select`` with the round's ``vl`` and ``nodes0``, as ``PuctSearch.act``
uses them); the slots from s on are void.  Slot j of row i is batch row ``i * L + j``.

``advance(priors [N * L, C], values [N * L], root_priors=None) -> (leaf_obs [N * L, 2, m, n], leaf_mask [N * L, C], fresh
[N])``; ``root_priors`` is ``AsyncOptsRule.advance``'s.  The helper's own counters: ``void_by_walk`` (slots below s without
a leaf), ``void_by_cap`` (slots from s on), ``ring_wraps`` (records written over an older one), and its parents'
``proven_plies`` and ``stats`` (finished games).
"""
import numpy as np

import puct_ops
import puct_search_rule as ps
from puct_rule import _canonical
from search_selfplay_async_opts_rule import AsyncOptsRule
from search_selfplay_rule import ERR_VISITS


class AsyncLeavesRule(AsyncOptsRule):
    def __init__(self, m, n, k, N, T, full, fast, threshold, c, temp_plies, seed, env_id0=0, root_noise=None,
                 noise_on_fast=False, solver=False, leaves=1, fpu=None, forced=None):
        assert 1 <= leaves <= 16 and full % leaves == 0
        self.L = leaves
        self.void_by_walk = 0
        self.void_by_cap = 0
        self.ring_wraps = 0
        super().__init__(m, n, k, N, T, full, fast, threshold, c, temp_plies, seed, env_id0, root_noise, noise_on_fast,
                         solver, fpu, forced)

    def begin(self):
        """every row's search starts afresh: slot 0 is the root, the others are void and show it"""
        self.slots = [None] * self.N
        self.row_sims = np.zeros(self.N, np.int64)
        super().begin()
        return self.view()

    def view(self):
        obs, mask = super().view()
        return np.repeat(obs, self.L, axis=0), np.repeat(mask, self.L, axis=0)

    def _fresh(self, i):
        super()._fresh(i)
        self.slots[i] = [([0], 0)] + [None] * (self.L - 1)
        self.row_sims[i] = 0

    def _ply(self, i, visits, full):
        p = int(self.row_plies[i])
        played = super()._ply(i, visits, full)
        if played and p >= self.T:
            self.ring_wraps += 1
        return played

    def advance(self, priors, values, root_priors=None):
        N, C, m, n, L = self.N, self.C, self.m, self.n, self.L
        priors = np.asarray(priors, np.float32).reshape(N * L, C)
        values = np.asarray(values, np.float32).reshape(N * L)
        leaf_obs = np.zeros((N * L, 2, m, n), np.float32)
        leaf_mask = np.zeros((N * L, C), bool)
        fresh = np.zeros(N, np.uint8)
        self.root_wanted = {}
        for i in range(N):
            tree, root = self.trees[i], self.roots[i]
            shown = [(root, 0)] * L  # what the row's L batch rows show: (position, depth)
            if not self.live[i]:  # a root without a legal cell: reported, left alone, shown again
                self.errors.append((ERR_VISITS, i))
            else:
                full = self.is_full(i)
                for j in puct_ops.backup_order(L):
                    slot = self.slots[i][j]
                    if slot is None:
                        continue
                    path, kind = slot
                    prior = priors[i * L + j]
                    if j == 0 and len(path) == 1:  # evaluation 0: the pending leaf is the root of a fresh tree
                        prior = self._root_priors(i, prior, full, root_priors)
                    ps.backup(tree, root, path, kind, prior, values[i * L + j], self.solver)
                    self.slots[i][j] = None
                budget = self.full if full else self.fast
                proven = self.solver and tree.proof[0] != 0
                if self.row_sims[i] < budget and not proven:
                    s = min(L, budget - int(self.row_sims[i]))
                    nodes0, vl, open_ = len(tree.n), {}, True
                    slots = [None] * L
                    for j in range(s):
                        got = None
                        if open_ and len(tree.n) <= self.full:
                            got = self._walk(i, vl, nodes0)
                        if got is None:
                            open_ = False
                            self.void_by_walk += 1
                            continue
                        path, pos, d, kind = got
                        for x in path:
                            vl[x] = vl.get(x, 0) + 1
                        slots[j] = (path, kind)
                        shown[j] = (pos, d)
                    if slots[0] is None:  # no leaf at all: nothing pending, reported, the counter stays
                        self.void_by_walk -= s
                        self.errors.append((ERR_VISITS, i))
                    else:
                        self.void_by_cap += L - s
                        self.row_sims[i] += s
                    self.slots[i] = slots
                else:
                    visits, _ = ps.root_counts(tree, C, self.solver)
                    if proven:
                        self.proven_plies.append((i, int(self.row_plies[i]), root.copy(), tree.proof[0],
                                                  self.row_sims[i] < budget))
                    if self._ply(i, visits, full):
                        self._fresh(i)
                        shown = [(self.roots[i], 0)] * L
                        fresh[i] = 1
                    else:
                        self.errors.append((ERR_VISITS, i))
            for j, (pos, d) in enumerate(shown):
                leaf_obs[i * L + j] = _canonical(pos, d, m, n)
                leaf_mask[i * L + j] = ~(pos[0] | pos[1])
        return leaf_obs, leaf_mask, fresh
