"""numpy restatement of the PUCT player with several leaves per row and evaluation (test helper; the rule is stated in
include/mnk_hip.h, mnk_puct_step_leaves).  The trees and their backup are those of tests/puct_rule.py, the match against a
kept tree and its rebase those of tests/puct_reuse_rule.py.

A round backs up the L pending slots of every row in slot order, then selects L new ones: slot j walks from the root by
the PUCT score under virtual visits -- vl(x) = how many earlier non-void slots of the round have node x on their path;
a child counts as n + vl visits of value sum w - vl, its parent as n + vl -- creates its leaf or lands on a terminal child
again, and is VOID (the root's view, nothing pending) when its walk reaches a node that is not terminal and was created
earlier in the same round, when the tree is full or when the root has no legal cell.  Every slot after a void one is void.
Slot j of row i is batch row i * L + j of every evaluation; evaluation 0 is the root in slot 0 and void slots behind it.

``LeavesPuct.act`` records every evaluation's (leaf_obs, leaf_mask) in ``leaves`` and returns, in ``self.trace``, one
dict per row of the last act: ``void`` (void slots after evaluation 0), ``shared`` (slots with a leaf whose path shares a
node below the root with an earlier slot of their round), ``repeat`` (slots whose leaf is a terminal node that an earlier
slot of their round has as its leaf too) and ``live`` (the root has a legal cell).
"""
import numpy as np

import puct_ops
from oracle import philox
from playout_rule import has_run
from puct_reuse_rule import descend, match, rebase
from puct_rule import _Tree, _backup, _canonical
from tactical_rule import _as_bool


def _select_vl(tree, root, m, n, k, c, vl, nodes0):
    """one walk from the root under the virtual visits ``vl`` (node -> count): (path, leaf position [2, C], depth), or
    None when it reaches a node of id >= nodes0 that is not terminal"""
    pos = root.copy()
    v, d, path = 0, 0, [0]
    while True:
        legal = np.flatnonzero(~(pos[0] | pos[1]))
        kids = [tree.kids[v].get(int(a)) for a in legal]
        va = np.array([0 if ch is None else vl.get(ch, 0) for ch in kids], np.int64)
        na = np.array([0 if ch is None else tree.n[ch] for ch in kids], np.int64) + va
        wa = np.array([0 if ch is None else tree.w[ch] for ch in kids], np.float32) + (-va.astype(np.float32))
        q = np.where(na > 0, wa / np.maximum(na, 1).astype(np.float32), np.float32(0)).astype(np.float32)
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
            return path, pos, d
        ch = tree.kids[v][a]
        path.append(ch)
        if tree.term[ch]:
            return path, pos, d
        if ch >= nodes0:
            return None
        v = ch


class LeavesPuct:
    """``act(obs, step=0, deterministic=False) -> (actions int64 [N], visits int32 [N, C], root_value f32 [N], carried
    int32 [N, 2])``.  ``reuse``: the trees are kept between acts as ``puct_reuse_rule.ReusePuct`` keeps them (``tree_nodes``
    nodes per row, default 2 * iterations + 1); otherwise every act starts fresh and ``carried`` is zeros."""

    def __init__(self, k, iterations, c, evaluator, L, reuse=False, tree_nodes=None, seed=0, env_id0=0, temperature=0,
                 leaves=None):
        assert 1 <= L <= 16 and iterations % L == 0
        self.k, self.iterations, self.c, self.L = k, iterations, np.float32(c), L
        self.evaluator, self.reuse = evaluator, reuse
        self.tree_nodes = (2 * iterations + 1 if tree_nodes is None else tree_nodes) if reuse else iterations + 1
        assert iterations + 1 <= self.tree_nodes
        self.seed, self.env_id0, self.temperature, self.leaves = seed, env_id0, temperature, leaves
        self.trace = None
        self.reset()

    def reset(self):
        self.trees, self.roots, self.live = None, None, None

    def act(self, obs, step=0, deterministic=False):
        obs = _as_bool(obs)
        N, _, m, n = obs.shape
        C, L, k, J, c = m * n, self.L, self.k, self.iterations, self.c
        roots = obs.reshape(N, 2, C).copy()
        if self.trees is None or len(self.trees) != N or not self.reuse:
            self.trees, self.roots, self.live = [None] * N, [None] * N, np.zeros(N, bool)
        carried = np.zeros((N, 2), np.int32)
        cont = np.zeros(N, bool)
        for i in range(N):
            v = None
            if self.trees[i] is not None and self.live[i]:
                path = match(self.roots[i], roots[i])
                if path is not None:
                    v = descend(self.trees[i], path)
            if v is None:
                self.trees[i] = _Tree()
            else:
                self.trees[i], _ = rebase(self.trees[i], v, self.tree_nodes - J)
                carried[i] = len(self.trees[i].n), self.trees[i].n[0]
                cont[i] = True
            self.roots[i] = roots[i]
        live = ~(roots[:, 0] | roots[:, 1]).all(axis=1)
        self.live = live
        trees = self.trees
        root_view = [_canonical(roots[i], 0, m, n) for i in range(N)]
        root_mask = ~(roots[:, 0] | roots[:, 1])
        leaf_obs = np.stack([root_view[i] for i in range(N) for _ in range(L)])
        leaf_mask = np.repeat(root_mask, L, axis=0)
        paths = [[[0]] + [None] * (L - 1) for _ in range(N)]  # per row and slot: the pending path, None = void
        self.trace = [dict(void=0, shared=0, repeat=0, live=bool(live[i])) for i in range(N)]
        rounds = J // L
        for it in range(rounds + 1):
            if self.leaves is not None:
                self.leaves.append((leaf_obs.copy(), leaf_mask.copy()))
            priors, values = self.evaluator(leaf_obs.copy(), leaf_mask.copy())
            priors = np.asarray(priors, np.float32).reshape(N * L, C)
            values = np.asarray(values, np.float32).reshape(N * L)
            for i in range(N):
                for j in puct_ops.backup_order(L):
                    if paths[i][j] is None:
                        continue
                    if it == 0 and cont[i]:
                        trees[i].prior[0] = priors[i * L + j].copy()  # the root's priors again and nothing else
                    else:
                        _backup(trees[i], paths[i][j], priors[i * L + j], values[i * L + j])
            if it == rounds:
                break
            for i in range(N):
                t, tr = trees[i], self.trace[i]
                nodes0, vl, done, open_ = len(t.n), {}, [], bool(live[i])
                for j in range(L):
                    got = None
                    if open_ and len(t.n) <= self.tree_nodes - 1:
                        got = _select_vl(t, roots[i], m, n, k, c, vl, nodes0)
                    if got is None:
                        open_ = False
                        paths[i][j] = None
                        tr["void"] += 1
                        leaf_obs[i * L + j], leaf_mask[i * L + j] = root_view[i], root_mask[i]
                        continue
                    path, pos, d = got
                    tr["shared"] += any(len(p) > 1 and p[1] == path[1] for p in done)
                    tr["repeat"] += bool(t.term[path[-1]]) and any(p[-1] == path[-1] for p in done)
                    done.append(path)
                    for x in path:
                        vl[x] = vl.get(x, 0) + 1
                    paths[i][j] = path
                    leaf_obs[i * L + j] = _canonical(pos, d, m, n)
                    leaf_mask[i * L + j] = ~(pos[0] | pos[1])
            assert all(len(t.n) <= self.tree_nodes for t in trees)

        env = np.uint64(self.env_id0) + np.arange(N, dtype=np.uint64)
        x = philox.rand_u32(self.seed, env, step, philox.STREAM_SAMPLE)
        if deterministic:
            x = np.zeros(N, np.uint64)
        actions = np.zeros(N, np.int64)
        visits = np.zeros((N, C), np.int32)
        root_value = np.zeros(N, np.float32)
        for i in range(N):
            t = trees[i]
            for a, ch in t.kids[0].items():
                visits[i, a] = t.n[ch]
            root_value[i] = np.float32(-t.w[0]) / np.float32(t.n[0])
            top = visits[i].max()
            if not live[i] or top == 0:
                actions[i] = philox.mulhi32(x[i], C)
                continue
            S = np.flatnonzero(visits[i] == top)
            if self.temperature == 1 and not deterministic:
                r = philox.mulhi32(x[i], int(visits[i].sum()))
                actions[i] = int(np.flatnonzero(np.cumsum(visits[i]) > r)[0])
            else:
                actions[i] = int(S[philox.mulhi32(x[i], len(S))])
        return actions, visits, root_value, carried


def puct_leaves(obs, k, iterations, c, evaluator, L, seed=0, step=0, env_id0=0, temperature=0, deterministic=False,
                leaves=None, trace=None):
    """one act of a fresh ``LeavesPuct``: (actions, visits, root_value); ``trace``: an optional list that receives the
    per-row trace"""
    rule = LeavesPuct(k, iterations, c, evaluator, L, seed=seed, env_id0=env_id0, temperature=temperature, leaves=leaves)
    out = rule.act(obs, step=step, deterministic=deterministic)
    if trace is not None:
        trace.extend(rule.trace)
    return out[:3]
