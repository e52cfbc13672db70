"""numpy restatement of the PUCT player that keeps its tree between calls (test helper; the rule is stated in
include/mnk_hip.h, mnk_puct_rebase).  The trees, their walk and their backup are those of tests/puct_rule.py.

``ReusePuct`` keeps one tree and one stored root per row.  ``act`` matches every row of the new observation against its
stored root BY POSITION: the same position, one ply on or two plies on, through children that exist and are not terminal,
continues the tree -- the subtree of the node that was reached is kept, its nodes in creation order, the first
``tree_nodes - iterations`` of them when there are more -- and any other row starts fresh.  Evaluation 0 is the roots for
every row; on a row that continues it only replaces the root's priors.  Then ``iterations`` selections and backups and
the move, as ``puct_rule.puct``.
"""
import numpy as np

from oracle import philox
from puct_rule import _Tree, _backup, _canonical, _select
from tactical_rule import _as_bool


def match(stored, new):
    """the path (list of cells) from the stored root [2, C] (plane 0 = its side to move) to the new position [2, C]
    (plane 0 = ITS side to move) when the new position is 0, 1 or 2 plies on; else None"""
    R0, R1 = stored
    O0, O1 = new
    if (O0 == R0).all() and (O1 == R1).all():
        return []
    if not (R0 & ~O1).any() and (O1 & ~R0).sum() == 1 and (O0 == R1).all():
        return [int(np.flatnonzero(O1 & ~R0)[0])]
    if not (R0 & ~O0).any() and (O0 & ~R0).sum() == 1 and not (R1 & ~O1).any() and (O1 & ~R1).sum() == 1:
        return [int(np.flatnonzero(O0 & ~R0)[0]), int(np.flatnonzero(O1 & ~R1)[0])]
    return None


def descend(tree, path):
    """the node the path ends in, or None when a step has no child or reaches a terminal one"""
    v = 0
    for a in path:
        if a not in tree.kids[v]:
            return None
        v = tree.kids[v][a]
        if tree.term[v]:
            return None
    return v


def rebase(tree, v, keep):
    """the subtree of node v as a new tree: creation order kept, at most ``keep`` nodes, children of dropped nodes gone.
    Returns (tree, old ids of the kept nodes)."""
    inside = [False] * len(tree.n)
    parent = {}
    for u, kids in enumerate(tree.kids):
        for ch in kids.values():
            parent[ch] = u
    order = []
    for u in range(v, len(tree.n)):  # (a parent's id is below its children's)
        inside[u] = u == v or (u in parent and inside[parent[u]])
        if inside[u]:
            order.append(u)
    order = order[:keep]
    new_id = {u: j for j, u in enumerate(order)}
    out = _Tree()
    out.n, out.w, out.move, out.term, out.prior, out.kids = [], [], [], [], [], []
    for u in order:
        out.n.append(tree.n[u])
        out.w.append(tree.w[u])
        out.move.append(tree.move[u] if u != v else 0)
        out.term.append(tree.term[u] if u != v else 0)
        out.prior.append(None if tree.prior[u] is None else tree.prior[u].copy())
        out.kids.append({a: new_id[ch] for a, ch in tree.kids[u].items() if ch in new_id})
    return out, order


class ReusePuct:
    """``act(obs, step=0, deterministic=False) -> (actions int64 [N], visits int32 [N, C], root_value f32 [N], carried
    int32 [N, 2])``; ``leaves``: an optional list that receives (leaf_obs, leaf_mask) of every evaluation; ``reset``
    forgets the trees.  ``self.kept`` holds, after an act, the old ids of the nodes each row kept (None: fresh)."""

    def __init__(self, k, iterations, c, evaluator, tree_nodes=None, seed=0, env_id0=0, temperature=0, leaves=None):
        self.k, self.iterations, self.c = k, iterations, np.float32(c)
        self.evaluator = evaluator
        self.tree_nodes = 2 * iterations + 1 if tree_nodes is None else tree_nodes
        assert iterations + 1 <= self.tree_nodes
        self.seed, self.env_id0, self.temperature, self.leaves = seed, env_id0, temperature, leaves
        self.reset()

    def reset(self):
        self.trees, self.roots, self.live, self.kept = None, None, None, None

    def act(self, obs, step=0, deterministic=False):
        obs = _as_bool(obs)
        N, _, m, n = obs.shape
        C = m * n
        k, J, c = self.k, self.iterations, self.c
        roots = obs.reshape(N, 2, C).copy()
        if self.trees is None or len(self.trees) != N:
            self.trees, self.roots, self.live = [None] * N, [None] * N, np.zeros(N, bool)
        carried = np.zeros((N, 2), np.int32)
        cont = np.zeros(N, bool)
        self.kept = [None] * N
        for i in range(N):
            v = None
            if self.trees[i] is not None and self.live[i]:
                path = match(self.roots[i], roots[i])
                if path is not None:
                    v = descend(self.trees[i], path)
            if v is None:
                self.trees[i] = _Tree()
            else:
                self.trees[i], self.kept[i] = rebase(self.trees[i], v, self.tree_nodes - J)
                carried[i] = len(self.trees[i].n), self.trees[i].n[0]
                cont[i] = True
            self.roots[i] = roots[i]
        live = ~(roots[:, 0] | roots[:, 1]).all(axis=1)
        self.live = live
        trees = self.trees
        paths = [[0] for _ in range(N)]
        leaf_obs = np.stack([_canonical(roots[i], 0, m, n) for i in range(N)])
        leaf_mask = ~(roots[:, 0] | roots[:, 1])
        pending = np.ones(N, bool)
        for it in range(J + 1):
            if self.leaves is not None:
                self.leaves.append((leaf_obs.copy(), leaf_mask.copy()))
            priors, values = self.evaluator(leaf_obs.copy(), leaf_mask.copy())
            priors = np.asarray(priors, np.float32).reshape(N, C)
            values = np.asarray(values, np.float32).reshape(N)
            for i in range(N):
                if it == 0 and cont[i]:
                    trees[i].prior[0] = priors[i].copy()  # the root's priors again: no visit, no value, no child
                elif pending[i]:
                    _backup(trees[i], paths[i], priors[i], values[i])
            if it == J:
                break
            for i in range(N):
                if live[i]:
                    paths[i], pos, d = _select(trees[i], roots[i], m, n, k, c)
                else:
                    paths[i], pos, d = [0], roots[i], 0
                    pending[i] = False
                leaf_obs[i] = _canonical(pos, d, m, n)
                leaf_mask[i] = ~(pos[0] | pos[1])
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
