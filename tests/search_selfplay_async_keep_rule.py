"""numpy restatement of search self-play with per-row budgets that keeps the played move's subtree (test helper; the rule
is stated in include/mnk_hip.h, mnk_search_selfplay_advance_keep).

``AsyncKeepRule`` is an ``AsyncOptsRule`` with ``keep_tree`` and ``tree_nodes``.  With ``keep_tree`` off it is that rule
line for line.  With it, the end of a ply carries the subtree of the root's child through the move
(``puct_search_rule.rebase``, which keeps the proofs; the child is what
``puct_search_rule.descend`` finds for the one-ply path) when the game goes on, and the budget of a ply counts the
iterations above the visits the root was carried with.  ``carried`` (int32 [N, 2]) is the entry point's; ``trace`` lists,
for every ply that ended, (row, ply, full, kept, carried n, the kept child's proof before the carry, keep_nodes, the proof
the new root kept): kept = 0 for a row that then started fresh.
"""
import numpy as np

import puct_search_rule as ps
from puct_rule import _canonical
from search_selfplay_async_opts_rule import AsyncOptsRule
from search_selfplay_rule import ERR_VISITS


class AsyncKeepRule(AsyncOptsRule):
    def __init__(self, m, n, k, N, T, full, fast, threshold, c, temp_plies, seed, env_id0=0, root_noise=None,
                 noise_on_fast=False, solver=False, keep_tree=False, tree_nodes=None, fpu=None, forced=None):
        if not keep_tree:
            assert tree_nodes is None
            tree_nodes = full + 1
        self.keep_tree = keep_tree
        self.tree_nodes = 2 * full + 1 if tree_nodes is None else tree_nodes
        assert full + 1 <= self.tree_nodes
        self.keep_nodes = self.tree_nodes - full
        self.carried = np.zeros((N, 2), np.int32)
        self.trace = []
        super().__init__(m, n, k, N, T, full, fast, threshold, c, temp_plies, seed, env_id0, root_noise, noise_on_fast,
                         solver, fpu, forced)

    def begin(self):
        self.renew = [False] * self.N  # the pending evaluation is a carried root's: it only renews the root's priors
        self.carried[:] = 0
        return super().begin()

    def _fresh(self, i):
        super()._fresh(i)
        self.renew[i] = False
        self.carried[i] = 0

    def _carry(self, i, a):
        """the row's tree becomes the subtree of its root's child through cell a: False when there is none to keep"""
        tree = self.trees[i]
        v = ps.descend(tree, [a])
        if v is None:
            return False
        proof = tree.proof[v]
        new, _ = ps.rebase(tree, v, self.keep_nodes)
        if self.solver and proof and len(new.n) > 1:
            kids = [new.proof[ch] for ch in new.kids[0].values()]
            # the proof it had as a child, when the kept children still justify it: it plays in the launch that renews it
            if proof == ps.WIN or (ps.WIN if proof == ps.LOSS else ps.DRAW) in kids:
                new.proof[0] = proof
        self.trees[i] = new
        self.roots[i] = self._root(i)
        self.paths[i] = [0]
        self.pending[i], self.renew[i], self.live[i] = True, True, True
        self.kinds[i] = 0
        self.carried[i] = len(new.n), new.n[0]
        self.trace[-1] = self.trace[-1][:3] + (len(new.n), int(new.n[0]), int(proof), self.keep_nodes, int(new.proof[0]))
        return True

    def advance(self, priors, values, root_priors=None):
        """one launch: (leaf_obs f32 [N, 2, m, n], leaf_mask bool [N, C], fresh u8 [N])"""
        if not self.keep_tree:
            return super().advance(priors, values, root_priors)
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
                    if len(self.paths[i]) == 1:  # evaluation 0: the pending leaf is the row's root, carried or not
                        prior = self._root_priors(i, prior, full, root_priors)
                    if self.renew[i]:
                        tree.prior[0] = np.asarray(prior, np.float32).copy()  # the priors again: no visit, no value
                    else:
                        ps.backup(tree, root, self.paths[i], self.kinds[i], prior, values[i], self.solver)
                    self.pending[i] = self.renew[i] = False
                budget = self.full if full else self.fast
                proven = self.solver and tree.proof[0] != 0
                it = max(int(tree.n[0]) - max(int(self.carried[i, 1]), 1), 0)  # the iterations of this ply
                if it < budget and not proven:
                    assert len(tree.n) <= self.tree_nodes - 1
                    self.paths[i], pos, d, self.kinds[i] = self._walk(i, {}, len(tree.n))
                    self.pending[i] = True
                else:
                    visits, _ = ps.root_counts(tree, C, self.solver)
                    if proven:
                        self.proven_plies.append((i, int(self.row_plies[i]), root.copy(), tree.proof[0], it < budget))
                    before, p = self.boards[i].copy(), int(self.row_plies[i])
                    if self._ply(i, visits, full):
                        self.trace.append((i, p, full, 0, 0, 0, self.keep_nodes, 0))
                        ended = self.moves[i] == 0
                        if ended or not self._carry(i, int(np.flatnonzero((self.boards[i] ^ before).any(axis=0))[0])):
                            self._fresh(i)
                        pos = self.roots[i]
                        fresh[i] = 1
                    else:
                        self.errors.append((ERR_VISITS, i))
            leaf_obs[i] = _canonical(pos, d, m, n)
            leaf_mask[i] = ~(pos[0] | pos[1])
        return leaf_obs, leaf_mask, fresh
