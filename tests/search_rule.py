"""numpy restatement of the tree-search player (test helper; the rule is stated in include/mnk_hip.h, mnk_sample_search).

A tree per row, kept as Python lists: per node the move into it, whether it is terminal (and how), how many of its legal
cells are children already, its children in action order, and n / W / Lo from the view of the player who moved into
it.  Depth d of a node = number of moves from the root; the mover into a node of odd depth is "me" (channel 0).

Iteration it: every row walks from its root -- expanding the first untried legal cell of the first node that has one,
else descending to the child of maximal ``q + c * sqrt(n_v / n_child)`` in numpy float32 (each operation rounded on its
own), ties to the lowest cell -- then all rows' non-terminal leaves play their B random games together, vectorised over
(row, playout), by ``playout_rule.random_games`` with the u32 of ``u = (((step * I + it) * B + j) * C4) + t`` on stream
SEARCH.  Backup adds B visits and the outcomes to every node of the path.
"""
import numpy as np

from oracle import philox
from playout_rule import has_run, random_games
from tactical_rule import _as_bool

STREAM_SEARCH = 5  # MNK_STREAM_SEARCH of include/mnk_hip.h


class _Tree:
    def __init__(self):
        self.move, self.term, self.nexp, self.kids = [0], [0], [0], [[]]
        self.n, self.w, self.lo = [0], [0], [0]

    def add(self, move, term):
        self.move.append(move)
        self.term.append(term)
        self.nexp.append(0)
        self.kids.append([])
        self.n.append(0)
        self.w.append(0)
        self.lo.append(0)
        return len(self.move) - 1


def _score(w, lo, nc, nv, c):
    q = np.float32(w - lo) / np.float32(nc)
    return q + c * np.sqrt(np.float32(nv) / np.float32(nc))


def _select(tree, root, m, n, k, c):
    """one walk from the root: (path of node ids, leaf position [2, C], leaf terminal?)"""
    pos = root.copy()
    C = pos.shape[1]
    stones = int(root.sum())
    v, d, path = 0, 0, [0]
    while True:
        if tree.term[v]:
            return path, pos, True
        free = np.flatnonzero(~(pos[0] | pos[1]))
        side = d & 1                                    # d even: "me" (plane 0) to move
        if tree.nexp[v] < C - stones - d:               # expand the first untried legal cell
            cell = int(free[tree.nexp[v]])
            pos[side, cell] = True
            won = bool(has_run(pos[side].reshape(1, m, n), k)[0])
            full = stones + d + 1 >= C
            ch = tree.add(cell, 1 if won else (2 if full else 0))
            tree.kids[v].append(ch)
            tree.nexp[v] += 1
            path.append(ch)
            return path, pos, won or full
        best, bc = None, 0
        for ch in tree.kids[v]:                         # action order: strict ">" keeps the lowest cell on a tie
            s = _score(tree.w[ch], tree.lo[ch], tree.n[ch], tree.n[v], c)
            if best is None or s > best:
                best, bc = s, ch
        v = bc
        pos[side, tree.move[v]] = True
        d += 1
        path.append(v)


def _playouts(leaves, B, m, n, k, seed, env, base):
    """leaves: list of (position [2, C], depth); env / base: uint64 per leaf (base = the u of ply 0 of playout 0).
    Returns (wins of "me", wins of the other side) per leaf."""
    L = len(leaves)
    wm, wo = np.zeros(L, np.int64), np.zeros(L, np.int64)
    if L == 0:
        return wm, wo
    C = m * n
    C4 = (C + 3) // 4 * 4
    g_leaf = np.repeat(np.arange(L), B)
    g_j = np.tile(np.arange(B, dtype=np.uint64), L)
    G = L * B
    flat = np.stack([leaves[i][0] for i in g_leaf])     # [G, 2, C]
    side0 = np.array([leaves[i][1] & 1 for i in g_leaf])
    g_base = base[g_leaf] + g_j * np.uint64(C4)
    outcome, _ = random_games(flat, side0, np.arange(G), m, n, k, seed, env[g_leaf], g_base, STREAM_SEARCH)
    np.add.at(wm, g_leaf, outcome == 1)
    np.add.at(wo, g_leaf, outcome == 2)
    return wm, wo


def search(obs, k: int, I: int, B: int, c: float, seed: int, step: int = 0, env_id0: int = 0,
           deterministic: bool = False):
    """obs: [N, 2, m, n] canonical view (channel 0 = the side to move; non-zero = stone), numpy or torch.
    Returns (actions int64 [N], stats int64 [N, 3, C]: the root children's n, W, Lo per cell)."""
    obs = _as_bool(obs)
    N, _, m, n = obs.shape
    C = m * n
    C4 = (C + 3) // 4 * 4
    c = np.float32(c)
    roots = obs.reshape(N, 2, C)
    trees = [_Tree() for _ in range(N)]
    active = [i for i in range(N) if roots[i].sum() < C]  # a full board runs no iterations
    env_all = (np.int64(env_id0) + np.arange(N, dtype=np.int64)).astype(np.uint64)
    for it in range(I):
        walks = [(i,) + _select(trees[i], roots[i], m, n, k, c) for i in active]
        open_ = [wk for wk in walks if not wk[3]]
        leaves = [(wk[2], len(wk[1]) - 1) for wk in open_]
        rows = np.array([wk[0] for wk in open_], dtype=np.int64)
        base = np.full(len(open_), ((np.uint64(step) * np.uint64(I) + np.uint64(it)) * np.uint64(B)) * np.uint64(C4),
                       np.uint64)
        wm, wo = _playouts(leaves, B, m, n, k, seed, env_all[rows] if len(rows) else env_all[:0], base)
        counts = {wk[0]: (int(a), int(b)) for wk, a, b in zip(open_, wm, wo)}
        for i, path, _, terminal in walks:
            tree = trees[i]
            if terminal:
                leaf, depth = path[-1], len(path) - 1
                won = B if tree.term[leaf] == 1 else 0
                a, b = (won, 0) if depth & 1 else (0, won)
            else:
                a, b = counts[i]
            for d, v in enumerate(path):
                tree.n[v] += B
                tree.w[v] += a if d & 1 else b
                tree.lo[v] += b if d & 1 else a
    stats = np.zeros((N, 3, C), np.int64)
    for i, tree in enumerate(trees):
        for ch in tree.kids[0]:
            stats[i, :, tree.move[ch]] = (tree.n[ch], tree.w[ch], tree.lo[ch])
    visits = stats[:, 0]
    best = np.where(visits.max(axis=1, keepdims=True) > 0, visits == visits.max(axis=1, keepdims=True), False)
    x = np.zeros(N, np.uint64) if deterministic else philox.rand_u32(seed, env_all, step, philox.STREAM_SAMPLE)
    return philox.pick_legal(best, x), stats
