"""numpy restatement of the PUCT player that proves wins, draws and losses in its tree (test helper; the rule is stated
in include/mnk_hip.h, mnk_puct_step_solver), and a brute-force negamax to hold its proofs against.  The trees, the
canonical view and the match against a kept tree are those of tests/puct_rule.py and tests/puct_reuse_rule.py; the rounds
and their virtual visits those of tests/puct_leaves_rule.py, whose ``LeavesPuct`` this class equals with ``solver=False``.

Every node has a ``proof`` from the point of view of the player who moved into it (its ``w``'s): 0 unknown, WIN, DRAW,
LOSS.  A new node whose move won is WIN, one whose move filled the board DRAW.  The selection leaves out the children
proven LOSS (unless every child is), and ends in a child with a proof as it ends in a terminal one; the backup of a proven
leaf then proves what it can along the path, leaf side first; the move is made from the adjusted counts.  A root with a
proof selects nothing more.
"""
import functools

import numpy as np

import puct_ops
from oracle import philox
from playout_rule import has_run
from puct_reuse_rule import descend, match, rebase
from puct_rule import _Tree, _canonical
from tactical_rule import _as_bool

WIN, DRAW, LOSS = 1, 2, 3
PROOF_UNKNOWN = -128  # MNK_PROOF_UNKNOWN
_VALUE = {WIN: -1.0, DRAW: 0.0, LOSS: 1.0}  # of a proven node for its own side to move


class _ProofTree(_Tree):
    def __init__(self):
        super().__init__()
        self.proof = [0]

    def add(self, move, term):
        self.proof.append(term)  # (term 1: the move won = WIN; term 2: it filled the board = DRAW)
        return super().add(move, term)


def _rebase(tree, v, keep):
    """``puct_reuse_rule.rebase`` with the proofs of the kept nodes; the new root's is unknown, as a fresh root's"""
    out, order = rebase(tree, v, keep)
    out.__class__ = _ProofTree
    out.proof = [tree.proof[u] if u != v else 0 for u in order]
    return out


def _select(tree, root, m, n, k, c, vl, nodes0, solver):
    """one walk from the root under the virtual visits ``vl``: (path, leaf position [2, C], depth, the leaf's pending
    kind: its terminal kind, with the solver its proof), or None when it reaches a node of id >= nodes0 that needs an
    evaluation"""
    pos = root.copy()
    v, d, path = 0, 0, [0]
    while True:
        legal = np.flatnonzero(~(pos[0] | pos[1]))
        kids = [tree.kids[v].get(int(a)) for a in legal]
        if solver:
            held = np.array([ch is None or tree.proof[ch] != LOSS for ch in kids])
            if held.any():
                legal, kids = legal[held], [ch for ch, h in zip(kids, held) if h]
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
            return path, pos, d, tree.term[ch]
        ch = tree.kids[v][a]
        path.append(ch)
        kind = tree.proof[ch] if solver else tree.term[ch]
        if kind:
            return path, pos, d, kind
        if ch >= nodes0:
            return None
        v = ch


def decided(tree, x, occupied):
    """what the proofs of node x's children make of x (``occupied``: bool [C], the stones at x), 0: nothing yet"""
    kids = [tree.kids[x].get(int(a)) for a in np.flatnonzero(~occupied)]
    proofs = [0 if ch is None else tree.proof[ch] for ch in kids]
    if WIN in proofs:
        return LOSS
    if 0 in proofs or not proofs:
        return 0
    return WIN if all(pf == LOSS for pf in proofs) else DRAW


def _backup(tree, root, path, kind, prior, value, solver):
    d = len(path) - 1
    leaf = path[-1]
    if kind:
        v = np.float32(_VALUE[kind])
    else:
        v = np.float32(value)
        tree.prior[leaf] = np.asarray(prior, np.float32).copy()
    for j, node in enumerate(path):
        tree.n[node] += 1
        tree.w[node] = np.float32(tree.w[node] + (v if (d - j) & 1 else -v))
    if not (solver and kind):
        return
    for p in range(d - 1, -1, -1):
        x = path[p]
        if tree.proof[x]:
            break
        occupied = root[0] | root[1]
        occupied[[tree.move[y] for y in path[1:p + 1]]] = True
        tree.proof[x] = decided(tree, x, occupied)
        if not tree.proof[x]:
            break


class SolverPuct:
    """``act(obs, step=0, deterministic=False) -> (actions int64 [N], visits int32 [N, C], root_value f32 [N], carried
    int32 [N, 2], proof int8 [N])``; the arguments are ``puct_leaves_rule.LeavesPuct``'s and ``solver``.  ``self.proven``
    holds, after an act, which rows arrived at a carried root that the proofs of its kept children decide (the root
    itself starts unknown: the first visit to the deciding child proves it again)."""

    def __init__(self, k, iterations, c, evaluator, L=1, reuse=False, tree_nodes=None, seed=0, env_id0=0, temperature=0,
                 leaves=None, solver=True):
        assert 1 <= L <= 16 and iterations % L == 0
        self.k, self.iterations, self.c, self.L = k, iterations, np.float32(c), L
        self.evaluator, self.reuse, self.solver = evaluator, reuse, solver
        self.tree_nodes = (2 * iterations + 1 if tree_nodes is None else tree_nodes) if reuse else iterations + 1
        assert iterations + 1 <= self.tree_nodes
        self.seed, self.env_id0, self.temperature, self.leaves = seed, env_id0, temperature, leaves
        self.reset()

    def reset(self):
        self.trees, self.roots, self.live, self.proven = None, None, None, None

    def act(self, obs, step=0, deterministic=False):
        obs = _as_bool(obs)
        N, _, m, n = obs.shape
        C, L, k, J, c, solver = m * n, self.L, self.k, self.iterations, self.c, self.solver
        roots = obs.reshape(N, 2, C).copy()
        if self.trees is None or len(self.trees) != N or not self.reuse:
            self.trees, self.roots, self.live = [None] * N, [None] * N, np.zeros(N, bool)
        carried = np.zeros((N, 2), np.int32)
        cont = np.zeros(N, bool)
        self.proven = np.zeros(N, bool)
        for i in range(N):
            v = None
            if self.trees[i] is not None and self.live[i]:
                path = match(self.roots[i], roots[i])
                if path is not None:
                    v = descend(self.trees[i], path)
            if v is None:
                self.trees[i] = _ProofTree()
            else:
                self.trees[i] = _rebase(self.trees[i], v, self.tree_nodes - J)
                carried[i] = len(self.trees[i].n), self.trees[i].n[0]
                cont[i] = True
                self.proven[i] = bool(decided(self.trees[i], 0, roots[i][0] | roots[i][1]))
            self.roots[i] = roots[i]
        live = ~(roots[:, 0] | roots[:, 1]).all(axis=1)
        self.live = live
        trees = self.trees
        root_view = [_canonical(roots[i], 0, m, n) for i in range(N)]
        root_mask = ~(roots[:, 0] | roots[:, 1])
        leaf_obs = np.stack([root_view[i] for i in range(N) for _ in range(L)])
        leaf_mask = np.repeat(root_mask, L, axis=0)
        pending = [[([0], 0)] + [None] * (L - 1) for _ in range(N)]  # per row and slot: (path, kind), None = void
        rounds = J // L
        for it in range(rounds + 1):
            if self.leaves is not None:
                self.leaves.append((leaf_obs.copy(), leaf_mask.copy()))
            priors, values = self.evaluator(leaf_obs.copy(), leaf_mask.copy())
            priors = np.asarray(priors, np.float32).reshape(N * L, C)
            values = np.asarray(values, np.float32).reshape(N * L)
            for i in range(N):
                for j in puct_ops.backup_order(L):
                    if pending[i][j] is None:
                        continue
                    if it == 0 and cont[i]:
                        trees[i].prior[0] = priors[i * L + j].copy()  # the root's priors again and nothing else
                    else:
                        _backup(trees[i], roots[i], *pending[i][j], priors[i * L + j], values[i * L + j], solver)
            if it == rounds:
                break
            for i in range(N):
                t = trees[i]
                nodes0, vl = len(t.n), {}
                open_ = bool(live[i]) and not (solver and t.proof[0])
                for j in range(L):
                    got = None
                    if open_ and len(t.n) <= self.tree_nodes - 1:
                        got = _select(t, roots[i], m, n, k, c, vl, nodes0, solver)
                    if got is None:
                        open_ = False
                        pending[i][j] = None
                        leaf_obs[i * L + j], leaf_mask[i * L + j] = root_view[i], root_mask[i]
                        continue
                    path, pos, d, kind = got
                    for x in path:
                        vl[x] = vl.get(x, 0) + 1
                    pending[i][j] = (path, kind)
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
        proof = np.full(N, PROOF_UNKNOWN, np.int8)
        for i in range(N):
            t = trees[i]
            kinds = np.zeros(C, np.int64)
            for a, ch in t.kids[0].items():
                visits[i, a] = t.n[ch]
                kinds[a] = t.proof[ch]
            root_value[i] = np.float32(-t.w[0]) / np.float32(t.n[0])
            if solver:
                adjusted = np.where(kinds == WIN, visits[i], 0) if (kinds == WIN).any() else np.where(kinds == LOSS, 0, visits[i])
                if adjusted.any():
                    visits[i] = adjusted
                if t.proof[0]:
                    proof[i] = int(_VALUE[t.proof[0]])
                    root_value[i] = np.float32(_VALUE[t.proof[0]])
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
        return actions, visits, root_value, carried, proof


def puct_solver(obs, k, iterations, c, evaluator, L=1, seed=0, step=0, env_id0=0, temperature=0, deterministic=False,
                leaves=None, solver=True):
    """one act of a fresh ``SolverPuct``: (actions, visits, root_value, proof)"""
    rule = SolverPuct(k, iterations, c, evaluator, L, seed=seed, env_id0=env_id0, temperature=temperature, leaves=leaves,
                      solver=solver)
    out = rule.act(obs, step=step, deterministic=deterministic)
    return out[0], out[1], out[2], out[4]


# ----------------------------------------------------------------------------- brute force
@functools.lru_cache(maxsize=None)
def _lines(m, n, k):
    """every run of k cells in a row, column or diagonal of the board, as a bit set over the cells"""
    out = []
    for r in range(m):
        for c in range(n):
            for dr, dc in ((0, 1), (1, 0), (1, 1), (1, -1)):
                cells = [(r + j * dr, c + j * dc) for j in range(k)]
                if all(0 <= y < m and 0 <= x < n for y, x in cells):
                    out.append(sum(1 << (y * n + x) for y, x in cells))
    return tuple(out)


def _bits(plane):
    return sum(1 << int(a) for a in np.flatnonzero(plane))


def _after(me, other, a, m, n, k, value):
    """the value for the mover of playing cell a: me, other = the mover's and the other side's stones as bit sets"""
    mine = me | (1 << a)
    if any(mine & line == line for line in _lines(m, n, k)):
        return 1
    if (mine | other) == (1 << m * n) - 1:
        return 0
    return -value(other, mine)


def _negamax(m, n, k):
    @functools.lru_cache(maxsize=None)
    def value(me, other):
        return max(_after(me, other, a, m, n, k, value) for a in range(m * n) if not (me | other) >> a & 1)

    return value


def negamax(pos, m, n, k):
    """the game-theoretic value (+1 win, 0 draw, -1 loss) of ``pos`` (bool [2, C], plane 0 = the side to move; no run on
    the board, a free cell) for its side to move, by exhaustive search; for positions of at most 7 free cells"""
    assert 1 <= (~(pos[0] | pos[1])).sum() <= 7
    return _negamax(m, n, k)(_bits(pos[0]), _bits(pos[1]))


def value_after(pos, a, m, n, k):
    """the value for the side to move of ``pos`` of playing the free cell ``a``"""
    assert not pos[0][a] and not pos[1][a] and (~(pos[0] | pos[1])).sum() <= 8
    return _after(_bits(pos[0]), _bits(pos[1]), int(a), m, n, k, _negamax(m, n, k))
