"""numpy restatement of search self-play with per-row budgets and its two options, root noise and the solver (test
helper; the rule is stated in include/mnk_hip.h, mnk_search_selfplay_advance_opts).

``AsyncOptsRule`` is an ``AsyncSelfPlayRule`` whose trees carry proofs (``puct_search_rule``: its backup, its selection
with ``solver``, ``fpu`` and ``forced`` as arguments -- a ply FORCES iff it is full or ``noise_on_fast`` is set --, and
``decided`` inside the backup) and whose roots take ``puct_noise_rule.root_noise`` at step = the row's ply count.  With
every option off it plays what ``AsyncSelfPlayRule`` plays.  ``picks`` and ``shunned`` are the selection's records.

``advance(priors, values, root_priors=None)``: ``root_priors`` (float32 [N, C]) optionally hands in the priors the kernel
stored on the roots; the rows that back up a root's evaluation in this launch then store those instead of the rule's own,
so that one ulp in a logarithm cannot send the two searches different ways.  What the rule itself computes for those rows
is kept in ``root_wanted`` ({row: (noised, float32 [C])} of the last launch) to compare with.
"""
import numpy as np

import puct_search_rule as ps
from puct_noise_rule import root_noise
from puct_rule import _canonical
from search_selfplay_async_rule import AsyncSelfPlayRule
from search_selfplay_rule import ERR_VISITS


class AsyncOptsRule(AsyncSelfPlayRule):
    def __init__(self, m, n, k, N, T, full, fast, threshold, c, temp_plies, seed, env_id0=0, root_noise=None,
                 noise_on_fast=False, solver=False, fpu=None, forced=None):
        self.root_noise, self.noise_on_fast, self.solver = root_noise, noise_on_fast, solver
        self.fpu, self.forced, self.picks, self.shunned = ps.as_pair(fpu), forced, [], []
        self.noised_roots = 0  # roots backed up with noise / without (the counters are the helper's own)
        self.plain_roots = 0
        self.proven_plies = []  # (row, ply, root bool [2, C], the root's proof, ended before its budget) of proven roots
        self.root_wanted = {}
        super().__init__(m, n, k, N, T, full, fast, threshold, c, temp_plies, seed, env_id0)

    def begin(self):
        self.kinds = [0] * self.N  # the pending leaf's kind: its terminal kind, with the solver its proof
        return super().begin()

    def _fresh(self, i):
        super()._fresh(i)
        self.trees[i] = ps.Tree()  # (no proof on the root)
        self.kinds[i] = 0

    def forces(self, i):
        """whether row i's current ply forces"""
        return self.forced is not None and (self.is_full(i) or self.noise_on_fast)

    def _walk(self, i, vl, nodes0):
        """``select`` on row i's tree with the row's options"""
        return ps.select(self.trees[i], self.roots[i], self.m, self.n, self.k, self.c, vl, nodes0, solver=self.solver,
                         fpu=self.fpu, forced=self.forced if self.forces(i) else None, log=self.picks,
                         shunned=self.shunned)

    def _root_priors(self, i, prior, full, given):
        """what the root of row i stores at the backup of its evaluation"""
        noised = self.root_noise is not None and (full or self.noise_on_fast)
        want = prior
        if noised:
            alpha, eps = self.root_noise
            mask = ~(self.roots[i][0] | self.roots[i][1])
            want = root_noise(prior[None], mask[None], alpha, eps, self.seed, int(self.row_plies[i]), self.env_id0 + i)[0]
            self.noised_roots += 1
        else:
            self.plain_roots += 1
        self.root_wanted[i] = (noised, want)
        return want if given is None else np.asarray(given[i], np.float32)

    def advance(self, priors, values, root_priors=None):
        """one launch: (leaf_obs f32 [N, 2, m, n], leaf_mask bool [N, C], fresh u8 [N])"""
        N, C, m, n = self.N, self.C, self.m, self.n
        priors = np.asarray(priors, np.float32).reshape(N, C)
        values = np.asarray(values, np.float32).reshape(N)
        leaf_obs = np.zeros((N, 2, m, n), np.float32)
        leaf_mask = np.zeros((N, C), bool)
        fresh = np.zeros(N, np.uint8)
        self.root_wanted = {}
        for i in range(N):
            tree, root = self.trees[i], self.roots[i]
            pos, d = root, 0
            if not self.live[i]:  # a root without a legal cell: reported, left alone, shown again
                self.errors.append((ERR_VISITS, i))
            else:
                full = self.is_full(i)
                if self.pending[i]:
                    prior = priors[i]
                    if len(self.paths[i]) == 1:  # evaluation 0: the pending leaf is the root of a fresh tree
                        prior = self._root_priors(i, prior, full, root_priors)
                    ps.backup(tree, root, self.paths[i], self.kinds[i], prior, values[i], self.solver)
                    self.pending[i] = False
                budget = self.full if full else self.fast
                proven = self.solver and tree.proof[0] != 0
                if tree.n[0] - 1 < budget and not proven:
                    self.paths[i], pos, d, self.kinds[i] = self._walk(i, {}, len(tree.n))
                    self.pending[i] = True
                else:
                    visits, _ = ps.root_counts(tree, C, self.solver)
                    if proven:
                        self.proven_plies.append((i, int(self.row_plies[i]), root.copy(), tree.proof[0],
                                                  tree.n[0] - 1 < budget))
                    if self._ply(i, visits, full):
                        self._fresh(i)
                        pos = self.roots[i]
                        fresh[i] = 1
                    else:
                        self.errors.append((ERR_VISITS, i))
            leaf_obs[i] = _canonical(pos, d, m, n)
            leaf_mask[i] = ~(pos[0] | pos[1])
        return leaf_obs, leaf_mask, fresh
