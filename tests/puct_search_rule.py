"""numpy restatement of the PUCT player with every option it has (test helper; the rules are stated in
include/mnk_hip.h: mnk_puct_rebase, mnk_puct_step_leaves, mnk_puct_step_solver, mnk_puct_step_fpu, mnk_puct_step_forced).
The search with its options is stated HERE, once; tests/puct_reuse_rule.py, puct_leaves_rule.py, puct_solver_rule.py,
puct_fpu_rule.py and puct_forced_rule.py keep the names the tests know as constructors of ``PuctSearch``.  The plain search
of tests/puct_rule.py stays on its own, as the anchor this one is held against with every option off.

One tree type (``Tree``): per node the visit count n, the value sum w (float32, from the view of the player who moved into
the node), the move into it, its terminal kind (0, 1: the move won, 2: it filled the board), its ``proof`` from the same
point of view (0 unknown, WIN, DRAW, LOSS: a new node's is its terminal kind, and without the solver nothing else is ever
written there or read as a proof), its priors once evaluated and its children by cell.

One walk (``select``) with the options as arguments:
  ``vl``, ``nodes0``  the virtual visits of the round's earlier slots (node -> count) and the tree's size when the round
                      began: a walk that reaches a node created in its own round that needs an evaluation is void (None).
                      ``vl={}`` and ``nodes0=len(tree.n)`` give the walk of a single leaf
  ``solver``          the children proven LOSS are left out (unless every child is), and a child with a proof ends the walk
                      as a terminal one does; off, nothing is filtered and the terminal kinds are read
  ``fpu``             None: a free cell without a visit scores with q = 0; (fpu, fpu_root): with
                      ``q = max(q_v - r * mass, -1)``, ``q_v`` the node's own mean value, ``mass`` the square root of the
                      prior mass of its visited cells, ``r`` = ``fpu_root`` at the root and ``fpu`` below it
  ``forced``          None or k: at the root a free cell whose child has a stored visit, is not proven LOSS and has
                      ``n'^2 < k * P * S'`` is FORCED, and where a cell is FORCED only those are candidates
One ``backup``, which with the solver proves what a proven leaf lets it along the path, leaf side first.  One ``draw_move``.
One class, ``PuctSearch``: rounds of L slots, a kept tree (``reuse``), the solver's adjusted counts, the pruning of the
policy target (``prune``) ahead of the one draw.

THE PATCH POINT.  ``terminal`` (is this new node terminal) and ``decided`` (what do a node's children decide) are module
level functions that ``select``, ``backup`` and ``PuctSearch.act`` look up when they are called, as everyone who walks
looks ``select`` up: a test plants a wrong board in the rule by setting these attributes of this module.

Every float operation is a numpy float32 operation, rounded on its own; those the header pins are ``puct_ops``'s.
"""
import numpy as np

import puct_ops
from oracle import philox
from playout_rule import has_run
from puct_rule import _canonical
from tactical_rule import _as_bool

f32 = np.float32
WIN, DRAW, LOSS = 1, 2, 3
PROOF_UNKNOWN = -128  # MNK_PROOF_UNKNOWN
_VALUE = {WIN: -1.0, DRAW: 0.0, LOSS: 1.0}  # of a proven node for its own side to move


class Tree:
    def __init__(self):
        self.n, self.w, self.move, self.term, self.proof = [0], [f32(0)], [0], [0], [0]
        self.prior, self.kids = [None], [{}]

    def add(self, move, term):
        self.n.append(0)
        self.w.append(f32(0))
        self.move.append(move)
        self.term.append(term)
        self.proof.append(term)  # (term 1: the move won = WIN; term 2: it filled the board = DRAW)
        self.prior.append(None)
        self.kids.append({})
        return len(self.n) - 1


# ----------------------------------------------------------------------------- a kept tree
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
    """the subtree of node v as a new tree: creation order kept, at most ``keep`` nodes, children of dropped nodes gone,
    the proofs of the kept nodes with them; the new root's is unknown, as a fresh root's.  Returns (tree, old ids of the
    kept nodes)."""
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
    out = Tree()
    out.n, out.w, out.move, out.term, out.proof, out.prior, out.kids = [], [], [], [], [], [], []
    for u in order:
        out.n.append(tree.n[u])
        out.w.append(tree.w[u])
        out.move.append(tree.move[u] if u != v else 0)
        out.term.append(tree.term[u] if u != v else 0)
        out.proof.append(tree.proof[u] if u != v else 0)
        out.prior.append(None if tree.prior[u] is None else tree.prior[u].copy())
        out.kids.append({a: new_id[ch] for a, ch in tree.kids[u].items() if ch in new_id})
    return out, order


# ----------------------------------------------------------------------------- the patch point
def terminal(pos, side, m, n, k):
    """the terminal kind of a new node: ``pos`` bool [2, C] with the move on it, ``side`` the plane that made it"""
    if has_run(pos[side].reshape(1, m, n), k)[0]:
        return 1
    return 2 if (pos[0] | pos[1]).all() else 0


def decided(tree, x, occupied):
    """what the proofs of node x's children make of x (``occupied``: bool [C], the stones at x), 0: nothing yet"""
    kids = [tree.kids[x].get(int(a)) for a in np.flatnonzero(~occupied)]
    proofs = [0 if ch is None else tree.proof[ch] for ch in kids]
    if WIN in proofs:
        return LOSS
    if 0 in proofs or not proofs:
        return 0
    return WIN if all(pf == LOSS for pf in proofs) else DRAW


# ----------------------------------------------------------------------------- first-play urgency
def as_pair(fpu):
    """None, or (fpu, fpu_root) as float32: a number r stands for (r, r)"""
    if fpu is None:
        return None
    r, r0 = (fpu, fpu) if np.isscalar(fpu) else fpu
    return f32(r), f32(r0)


def mass_of(priors):
    """fl32(sqrt(T * 2^-32)), T = the sum over ``priors`` (float32, the visited free cells') of the prior clipped to
    [0, 1], times 2^32, truncated: Python integers, so no order of summation can matter"""
    clipped = np.minimum(np.maximum(np.asarray(priors, f32), f32(0)), f32(1))
    T = sum(int(np.float64(p) * 4294967296.0) for p in clipped)  # (p * 2^32 is exact in f64; int() truncates)
    return f32(np.sqrt(np.float64(T) * 2.0 ** -32))


def untried_q(tree, v, visited_priors, fpu):
    """the q of node v's free cells without a visit; ``fpu`` = (fpu, fpu_root) as float32"""
    qv = f32(-f32(tree.w[v])) / f32(tree.n[v])  # (the stored counts: no virtual visits)
    r = fpu[1] if v == 0 else fpu[0]
    return np.maximum(puct_ops.fpu_q(qv, r, mass_of(visited_priors)), f32(-1))


# ----------------------------------------------------------------------------- forced playouts
def short_of_floor(tree, legal, kids, vl, k_forced):
    """bool over ``legal`` (the root's free cells, ``kids`` their children or None): the cells whose child has a stored
    visit and n'^2 < k * P * S' -- clauses (1) and (3) of the rule, whatever the child's proof"""
    S = f32(tree.n[0] + vl.get(0, 0) - 1)
    out = np.zeros(len(legal), bool)
    for j, (a, ch) in enumerate(zip(legal, kids)):
        if ch is None or tree.n[ch] == 0:
            continue
        n1 = f32(tree.n[ch] + vl.get(ch, 0))
        out[j] = f32(n1 * n1) < puct_ops.forcing_bound(k_forced, tree.prior[0][a], S)
    return out


def forced_cells(tree, legal, kids, vl, solver, k_forced):
    """bool over ``legal``: which are FORCED -- ``short_of_floor`` and, with the solver, not proven LOSS (clause (2))"""
    out = short_of_floor(tree, legal, kids, vl, k_forced)
    if solver:
        out &= np.array([ch is None or tree.proof[ch] != LOSS for ch in kids], bool)
    return out


# ----------------------------------------------------------------------------- the walk and the backup
def select(tree, root, m, n, k, c, vl, nodes0, *, solver=False, fpu=None, forced=None, log=None, shunned=None):
    """one walk from the root under the virtual visits ``vl``: (path, leaf position [2, C], depth, the leaf's pending
    kind: its terminal kind, with the solver its proof), or None when it reaches a node of id >= nodes0 that needs an
    evaluation.  ``log`` (a list) takes, for every root selection with a FORCED cell, (the cell taken, the cell the plain
    score would have taken); ``shunned`` (a list) takes, for every root selection with the solver at which a child proven
    LOSS is short of its floor -- FORCED but for clause (2) --, (those cells, the cell taken, whether some free cell's
    child is not proven LOSS)"""
    pos = root.copy()
    v, d, path = 0, 0, [0]
    while True:
        legal = np.flatnonzero(~(pos[0] | pos[1]))
        kids = [tree.kids[v].get(int(a)) for a in legal]
        qu = f32(0)
        if fpu is not None:
            # the mass is over every free cell with a visit (virtual ones included), the children proven LOSS too
            seen = np.array([ch is not None and tree.n[ch] + vl.get(ch, 0) > 0 for ch in kids], bool)
            qu = untried_q(tree, v, tree.prior[v][legal[seen]], fpu)
        lost = ()  # the root's cells proven LOSS that are short of their floor (counted ahead of the filter below)
        if solver and v == 0 and forced is not None:
            short = short_of_floor(tree, legal, kids, vl, forced)
            lost = tuple(int(a) for a, ch, sh in zip(legal, kids, short) if sh and tree.proof[ch] == LOSS)
        if solver:
            held = np.array([ch is None or tree.proof[ch] != LOSS for ch in kids])
            if held.any():
                legal, kids = legal[held], [ch for ch, h in zip(kids, held) if h]
        va = np.array([0 if ch is None else vl.get(ch, 0) for ch in kids], np.int64)
        na = np.array([0 if ch is None else tree.n[ch] for ch in kids], np.int64) + va
        wa = np.array([0 if ch is None else tree.w[ch] for ch in kids], f32) + (-va.astype(f32))
        q = np.where(na > 0, wa / np.maximum(na, 1).astype(f32), qu).astype(f32)
        s = puct_ops.score(q, c, tree.prior[v][legal], puct_ops.sqrt(tree.n[v] + vl.get(v, 0)), na)
        a = int(legal[int(np.argmax(s))])  # (the first maximum: ties go to the lowest cell)
        if v == 0 and forced is not None:
            on = forced_cells(tree, legal, kids, vl, solver, forced)
            if on.any():
                plain = a
                a = int(legal[on][int(np.argmax(s[on]))])
                if log is not None:
                    log.append((a, plain))
            if lost and shunned is not None:
                shunned.append((lost, a, bool(held.any())))
        side = d & 1
        pos[side, a] = True
        d += 1
        if a not in tree.kids[v]:
            ch = tree.add(a, terminal(pos, side, m, n, k))
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


def backup(tree, root, path, kind, prior, value, solver):
    d = len(path) - 1
    leaf = path[-1]
    if kind:
        v = f32(_VALUE[kind])
    else:
        v = f32(value)
        tree.prior[leaf] = np.asarray(prior, f32).copy()
    for j, node in enumerate(path):
        tree.n[node] += 1
        tree.w[node] = f32(tree.w[node] + (v if (d - j) & 1 else -v))
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


# ----------------------------------------------------------------------------- the counts the move is made from
def adjusted_counts(visits, kinds):
    """the root children's visits (int64 [C]; ``kinds``: their proofs) as mnk_puct_step_solver adjusts them: only the WIN
    children's when there is one, else all but the LOSS children's; the raw ones when that leaves nothing"""
    adjusted = np.where(kinds == WIN, visits, 0) if (kinds == WIN).any() else np.where(kinds == LOSS, 0, visits)
    return adjusted if adjusted.any() else visits


def root_counts(tree, C, solver):
    """(n' int64 [C], whether the solver keeps the WIN children alone) of a tree's root"""
    visits, kinds = np.zeros(C, np.int64), np.zeros(C, np.int64)
    for a, ch in tree.kids[0].items():
        visits[a], kinds[a] = tree.n[ch], tree.proof[ch]
    if not solver:
        return visits, False
    wins_only = bool((kinds == WIN).any()) and bool(np.where(kinds == WIN, visits, 0).any())
    return adjusted_counts(visits, kinds), wins_only


def score(tree, a, j, c):
    """s_a(j) of the root's child through cell a"""
    ch = tree.kids[0][a]
    q = np.array([f32(tree.w[ch]) / f32(tree.n[ch])], f32)
    return puct_ops.score(q, f32(c), tree.prior[0][[a]], puct_ops.sqrt(tree.n[0]), np.array([j], np.int64))[0]


def floor_of(tree, a, n1, k_forced):
    """min(n'_a, F_a): F_a the least integer F >= 0 with fl(F * F) >= t_a"""
    t = puct_ops.floor_bound(k_forced, tree.prior[0][a], f32(tree.n[0] - 1))
    for F in range(n1):
        if f32(f32(F) * f32(F)) >= t:
            return F
    return n1


def prune(tree, counts, c, k_forced, info=None):
    """the pruned counts n'' (int64 [C]) of the root of ``tree`` from n' = ``counts``, by the rule's walk.  ``info`` (a
    dict) takes c*, s* and, per pruned cell, (lo, n', n'' before the single-visit rule)"""
    out = np.asarray(counts, np.int64).copy()
    if out.max() == 0:
        return out
    cstar = int(np.argmax(out))  # (the first maximum: ties to the lowest cell)
    sstar = score(tree, cstar, int(out[cstar]), c)
    if info is not None:
        info.update(cstar=cstar, sstar=sstar, cells={})
    for a in np.flatnonzero(out):
        a, n1 = int(a), int(out[a])
        if a == cstar or tree.prior[0][a] <= 0:
            continue
        lo = n1 - floor_of(tree, a, n1, k_forced)
        j = next((j for j in range(lo, n1 + 1) if score(tree, a, j, c) < sstar), n1)
        if info is not None and j != n1:
            info["cells"][a] = (lo, n1, j)
        out[a] = 0 if j == 1 and n1 > 1 else j
    return out


def draw_move(counts, x, C, live, temperature, deterministic):
    """the move of a row from its counts [C] and its Philox word ``x``: a row that is not ``live`` or has no count draws
    over all C cells; else in proportion to the counts (temperature 1) or among the cells of the most counts"""
    if not live or counts.max() == 0:
        return philox.mulhi32(x, C)
    if temperature == 1 and not deterministic:
        r = philox.mulhi32(x, int(counts.sum()))
        return int(np.flatnonzero(np.cumsum(counts) > r)[0])
    S = np.flatnonzero(counts == counts.max())
    return int(S[philox.mulhi32(x, len(S))])


# ----------------------------------------------------------------------------- the search
class PuctSearch:
    """``act(obs, step=0, deterministic=False) -> (actions int64 [N], visits int32 [N, C], root_value f32 [N], carried
    int32 [N, 2], proof int8 [N])``.  ``obs``: [N, 2, m, n] (a cell is a stone when non-zero); the evaluator is called once
    per evaluation on the whole batch, ``evaluator(leaf_obs f32 [N * L, 2, m, n], leaf_mask bool [N * L, C]) -> (priors,
    values)``, and ``leaves`` (a list) receives every evaluation's (leaf_obs, leaf_mask).

    A round backs up the L pending slots of every row in slot order, then selects L new ones: slot j walks under the
    virtual visits of the slots before it, and is VOID (the root's view, nothing pending) when its walk is, when the tree
    is full, when the root has no legal cell or, with the solver, has a proof.  Every slot after a void one is void.  Slot
    j of row i is batch row i * L + j; evaluation 0 is the root in slot 0 and void slots behind it.

    ``reuse``: ``act`` matches every row against its stored root BY POSITION (``match``, ``descend``) and continues the
    tree from the node reached (``rebase``: the first ``tree_nodes - iterations`` nodes of its subtree; ``tree_nodes``
    defaults to 2 * iterations + 1); evaluation 0 then only renews that root's priors.  Any other row, and every row
    without ``reuse``, starts fresh and has ``carried`` zero.

    After an act: ``trees``; ``kept`` (the old ids of the nodes each row kept, None: fresh); ``proven`` (the rows that
    arrived at a carried root which the proofs of its kept children decide -- the root itself starts unknown: the first
    visit to the deciding child proves it again); ``trace``, one dict per row: ``void`` (void slots after evaluation 0),
    ``shared`` (slots whose path shares a node below the root with an earlier slot of their round), ``repeat`` (slots whose
    leaf is a terminal node that an earlier slot of their round has as its leaf too), ``live``; ``raw_visits`` (n', the
    counts ahead of the pruning), ``picks`` and ``shunned`` (``select``'s ``log`` and ``shunned``) and ``pruned_info`` (the
    per-row ``info`` of ``prune``)."""

    def __init__(self, k, iterations, c, evaluator, L=1, reuse=False, tree_nodes=None, seed=0, env_id0=0, temperature=0,
                 leaves=None, solver=False, fpu=None, forced=None):
        assert 1 <= L <= 16 and iterations % L == 0
        self.k, self.iterations, self.c, self.L = k, iterations, f32(c), L
        self.evaluator, self.reuse, self.solver, self.fpu, self.forced = evaluator, reuse, solver, as_pair(fpu), forced
        self.tree_nodes = (2 * iterations + 1 if tree_nodes is None else tree_nodes) if reuse else iterations + 1
        assert iterations + 1 <= self.tree_nodes
        self.seed, self.env_id0, self.temperature, self.leaves = seed, env_id0, temperature, leaves
        self.trace, self.raw_visits, self.picks, self.shunned, self.pruned_info = None, None, [], [], []
        self.reset()

    def reset(self):
        self.trees, self.roots, self.live, self.proven, self.kept = None, None, None, None, None

    def act(self, obs, step=0, deterministic=False):
        obs = _as_bool(obs)
        N, _, m, n = obs.shape
        C, L, k, J, c, solver = m * n, self.L, self.k, self.iterations, self.c, self.solver
        roots = obs.reshape(N, 2, C).copy()
        if self.trees is None or len(self.trees) != N or not self.reuse:
            self.trees, self.roots, self.live = [None] * N, [None] * N, np.zeros(N, bool)
        carried = np.zeros((N, 2), np.int32)
        cont = np.zeros(N, bool)
        self.proven, self.kept = np.zeros(N, bool), [None] * N
        self.picks, self.shunned, self.pruned_info = [], [], [{} for _ in range(N)]
        for i in range(N):
            v = None
            if self.trees[i] is not None and self.live[i]:
                path = match(self.roots[i], roots[i])
                if path is not None:
                    v = descend(self.trees[i], path)
            if v is None:
                self.trees[i] = Tree()
            else:
                self.trees[i], self.kept[i] = rebase(self.trees[i], v, self.tree_nodes - J)
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
        self.trace = [dict(void=0, shared=0, repeat=0, live=bool(live[i])) for i in range(N)]
        rounds = J // L
        for it in range(rounds + 1):
            if self.leaves is not None:
                self.leaves.append((leaf_obs.copy(), leaf_mask.copy()))
            priors, values = self.evaluator(leaf_obs.copy(), leaf_mask.copy())
            priors = np.asarray(priors, f32).reshape(N * L, C)
            values = np.asarray(values, f32).reshape(N * L)
            for i in range(N):
                for j in puct_ops.backup_order(L):
                    if pending[i][j] is None:
                        continue
                    if it == 0 and cont[i]:
                        trees[i].prior[0] = priors[i * L + j].copy()  # the root's priors again and nothing else
                    else:
                        backup(trees[i], roots[i], *pending[i][j], priors[i * L + j], values[i * L + j], solver)
            if it == rounds:
                break
            for i in range(N):
                t, tr = trees[i], self.trace[i]
                nodes0, vl, done = len(t.n), {}, []
                open_ = bool(live[i]) and not (solver and t.proof[0])
                for j in range(L):
                    got = None
                    if open_ and len(t.n) <= self.tree_nodes - 1:
                        got = select(t, roots[i], m, n, k, c, vl, nodes0, solver=solver, fpu=self.fpu, forced=self.forced,
                                     log=self.picks, shunned=self.shunned)
                    if got is None:
                        open_ = False
                        pending[i][j] = None
                        tr["void"] += 1
                        leaf_obs[i * L + j], leaf_mask[i * L + j] = root_view[i], root_mask[i]
                        continue
                    path, pos, d, kind = got
                    tr["shared"] += any(len(p) > 1 and p[1] == path[1] for p in done)
                    tr["repeat"] += bool(t.term[path[-1]]) and any(p[-1] == path[-1] for p in done)
                    done.append(path)
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
        root_value = np.zeros(N, f32)
        proof = np.full(N, PROOF_UNKNOWN, np.int8)
        self.raw_visits = np.zeros((N, C), np.int32)
        for i in range(N):
            t = trees[i]
            counts, wins_only = root_counts(t, C, solver)
            visits[i] = self.raw_visits[i] = counts
            root_value[i] = f32(-t.w[0]) / f32(t.n[0])
            if solver and t.proof[0]:
                proof[i] = int(_VALUE[t.proof[0]])
                root_value[i] = f32(_VALUE[t.proof[0]])
            if self.forced is not None and not wins_only and live[i] and counts.max() > 0:
                visits[i] = prune(t, counts, c, self.forced, self.pruned_info[i])
            actions[i] = draw_move(visits[i], x[i], C, live[i], self.temperature, deterministic)
        return actions, visits, root_value, carried, proof
