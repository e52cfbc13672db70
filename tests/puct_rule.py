"""numpy restatement of the PUCT search player (test helper; the rule is stated in include/mnk_hip.h, mnk_puct_step).

One tree per row, kept as Python lists: per node the visit count n, the value sum w (numpy float32, from the view of the
player who moved into the node), the move into it, its terminal kind (0: not terminal, 1: the move won, 2: it filled the
board), its priors once evaluated and its children by cell.  Depth d of a node = moves from the root; the side to move at
depth d is "me" (channel 0 of the row) when d is even.

Evaluation 0 is the roots; then iterations 1 .. I each back up the previous evaluation and select the next leaf of every
row; a last backup precedes the move.  The evaluator is called once per evaluation on the whole batch:
``evaluator(leaf_obs f32 [N, 2, m, n], leaf_mask bool [N, C]) -> (priors [N, C], values [N])``, read as float32.  Every
float operation is a numpy float32 operation, rounded on its own.
"""
import numpy as np

import puct_ops
from oracle import philox
from playout_rule import has_run
from tactical_rule import _as_bool


class _Tree:
    def __init__(self):
        self.n, self.w, self.move, self.term, self.prior, self.kids = [0], [np.float32(0)], [0], [0], [None], [{}]

    def add(self, move, term):
        self.n.append(0)
        self.w.append(np.float32(0))
        self.move.append(move)
        self.term.append(term)
        self.prior.append(None)
        self.kids.append({})
        return len(self.n) - 1


def _canonical(pos, d, m, n):
    """the leaf's view: channel 0 = the side to move at depth d"""
    s = d & 1
    return np.stack([pos[s], pos[1 - s]]).reshape(2, m, n).astype(np.float32)


def _select(tree, root, m, n, k, c):
    """one walk from the root: (path, leaf position [2, C], depth)"""
    pos = root.copy()
    C = pos.shape[1]
    v, d, path = 0, 0, [0]
    while True:
        legal = np.flatnonzero(~(pos[0] | pos[1]))
        na = np.array([tree.n[tree.kids[v][a]] if a in tree.kids[v] else 0 for a in legal], np.int64)
        wa = np.array([tree.w[tree.kids[v][a]] if a in tree.kids[v] else 0 for a in legal], np.float32)
        q = np.where(na > 0, wa / np.maximum(na, 1).astype(np.float32), np.float32(0)).astype(np.float32)
        s = puct_ops.score(q, c, tree.prior[v][legal], puct_ops.sqrt(tree.n[v]), na)
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
        v = ch
        assert d <= C


def _backup(tree, path, prior, value):
    d = len(path) - 1
    leaf = path[-1]
    term = tree.term[leaf]
    if term:
        v = np.float32(-1.0 if term == 1 else 0.0)
    else:
        v = np.float32(value)
        tree.prior[leaf] = np.asarray(prior, np.float32).copy()
    for j, node in enumerate(path):
        tree.n[node] += 1
        tree.w[node] = np.float32(tree.w[node] + (v if (d - j) & 1 else -v))


def puct(obs, k, iterations, c, evaluator, seed=0, step=0, env_id0=0, temperature=0, deterministic=False, leaves=None):
    """obs: [N, 2, m, n] (a cell is a stone when non-zero).  Returns (actions int64 [N], visits int32 [N, C],
    root_value f32 [N]).  ``leaves``: an optional list that receives (leaf_obs, leaf_mask) of every evaluation."""
    obs = _as_bool(obs)
    N, _, m, n = obs.shape
    C = m * n
    c = np.float32(c)
    roots = obs.reshape(N, 2, C)
    live = ~(roots[:, 0] | roots[:, 1]).all(axis=1)
    trees = [_Tree() for _ in range(N)]
    paths = [[0] for _ in range(N)]
    leaf_obs = np.stack([_canonical(roots[i], 0, m, n) for i in range(N)])
    leaf_mask = ~(roots[:, 0] | roots[:, 1])
    pending = np.ones(N, bool)
    for it in range(iterations + 1):
        if leaves is not None:
            leaves.append((leaf_obs.copy(), leaf_mask.copy()))
        priors, values = evaluator(leaf_obs.copy(), leaf_mask.copy())
        priors = np.asarray(priors, np.float32).reshape(N, C)
        values = np.asarray(values, np.float32).reshape(N)
        for i in range(N):
            if pending[i]:
                _backup(trees[i], paths[i], priors[i], values[i])
        if it == iterations:
            break
        for i in range(N):
            if live[i]:
                paths[i], pos, d = _select(trees[i], roots[i], m, n, k, c)
            else:
                paths[i], pos, d = [0], roots[i], 0
                pending[i] = False
            leaf_obs[i] = _canonical(pos, d, m, n)
            leaf_mask[i] = ~(pos[0] | pos[1])

    env = np.uint64(env_id0) + np.arange(N, dtype=np.uint64)
    x = philox.rand_u32(seed, env, step, philox.STREAM_SAMPLE)
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
        if temperature == 1 and not deterministic:
            r = philox.mulhi32(x[i], int(visits[i].sum()))
            actions[i] = int(np.flatnonzero(np.cumsum(visits[i]) > r)[0])
        else:
            actions[i] = int(S[philox.mulhi32(x[i], len(S))])
    return actions, visits, root_value
