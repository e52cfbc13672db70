"""numpy restatement of the PUCT player's Gumbel root (test helper; the rule is stated in include/mnk_hip.h,
mnk_puct_step_gumbel).

``schedule`` is the table of considered visits, ``gumbel_scores`` what mnk_puct_gumbel_root writes, ``gumbel_puct`` one act:
the tree, the backup and the walk below the root are tests/puct_rule.py's (imported, not restated); the root's choice, the
move and the improved policy are here.  ``GumbelSelfPlayRule`` is tests/search_selfplay_rule.py's ``SelfPlayRule`` with
the ply of mnk_search_selfplay_step_moves.  float32 operations are numpy float32 operations, rounded one by one; what the
header says is f64 is numpy float64.
"""
import numpy as np

import puct_ops
from oracle import philox
from playout_rule import has_run
from puct_rule import _backup, _canonical, _Tree
from search_selfplay_rule import ERR_ACTION_RANGE, Z_UNKNOWN, SelfPlayRule
from oracle.packing import pack_cells
from tactical_rule import _as_bool

STREAM_GUMBEL = 8
ERR_ILLEGAL_MOVE = 2
TINY = np.float32(2.0 ** -126)


def schedule(considered, iterations):
    """uint16 [considered + 1, iterations]: row m' = the considered visits of a root with m' moves to consider"""
    I = iterations
    out = np.zeros((considered + 1, I), np.uint16)
    for mp in range(considered + 1):
        if mp <= 1:
            out[mp] = np.arange(I)
            continue
        l2 = int(np.ceil(np.log2(mp)))
        visits, nc, row = [0] * mp, mp, []
        while len(row) < I:
            extra = max(1, I // (l2 * nc))
            for _ in range(extra):
                row += visits[:nc]
                for j in range(nc):
                    visits[j] += 1
            nc = max(2, nc // 2)
        out[mp] = row[:I]
    return out


def gumbel_scores(priors, mask, gumbel_scale=1.0, seed=0, step=0, env_id0=0):
    """(gscore float32 [N, C], -inf on occupied cells; the Gumbel variables g float64 [N, C])"""
    priors = np.asarray(priors, np.float32)
    mask = np.asarray(mask).astype(bool)
    N, C = mask.shape
    C4 = (C + 3) & ~3
    env = (np.uint64(env_id0) + np.arange(N, dtype=np.uint64))[:, None]
    s = np.uint64(step) * np.uint64(C4) + np.arange(C, dtype=np.uint64)[None, :]
    env, s = np.broadcast_arrays(env, s)
    x = philox.rand_u32(seed, env, s, STREAM_GUMBEL)
    U = (x.astype(np.float64) + 0.5) * 2.0 ** -32
    g = -np.log(-np.log(U))
    l = np.log(np.maximum(priors, TINY).astype(np.float64))
    scale = float(np.float32(gumbel_scale))
    gs = (scale * g + l).astype(np.float32)
    return np.where(mask, gs, np.float32(-np.inf)).astype(np.float32), g


def _root_stats(tree, free):
    """(n int64, w float32, q float32) of the root's children through the cells ``free``"""
    kids = tree.kids[0]
    n = np.array([tree.n[kids[a]] if a in kids else 0 for a in free], np.int64)
    w = np.array([tree.w[kids[a]] if a in kids else 0 for a in free], np.float32)
    q = np.where(n > 0, w / np.maximum(n, 1).astype(np.float32), np.float32(0)).astype(np.float32)
    return n, w, q


def _keys(gs, n, q, c_visit, c_scale):
    sigma = np.float32(np.float32(c_visit + np.float32(n.max())) * c_scale)
    return np.where(n > 0, (gs + (sigma * q).astype(np.float32)).astype(np.float32), gs).astype(np.float32)


def _pick(tree, free, gs, want, c_visit, c_scale):
    """the free cell of maximal key among those of ``want`` visits (None: of the most), else among all; the lowest of a tie"""
    n, _, q = _root_stats(tree, free)
    key = _keys(gs[free], n, q, c_visit, c_scale)
    cand = n == (n.max() if want is None else want)
    if not cand.any():
        cand[:] = True
    return int(free[np.flatnonzero(cand)[int(np.argmax(key[cand]))]])


def _walk(tree, root, m, n, k, c, first):
    """tests/puct_rule.py's _select with the root's cell given"""
    pos = root.copy()
    v, d, path = 0, 0, [0]
    while True:
        if v == 0:
            a = first
        else:
            legal = np.flatnonzero(~(pos[0] | pos[1]))
            na = np.array([tree.n[tree.kids[v][a]] if a in tree.kids[v] else 0 for a in legal], np.int64)
            wa = np.array([tree.w[tree.kids[v][a]] if a in tree.kids[v] else 0 for a in legal], np.float32)
            q = np.where(na > 0, wa / np.maximum(na, 1).astype(np.float32), np.float32(0)).astype(np.float32)
            a = int(legal[int(np.argmax(puct_ops.score(q, c, tree.prior[v][legal], puct_ops.sqrt(tree.n[v]), na)))])
        side = d & 1
        pos[side, a] = True
        d += 1
        if a not in tree.kids[v]:
            won = bool(has_run(pos[side].reshape(1, m, n), k)[0])
            ch = tree.add(a, 1 if won else (2 if bool((pos[0] | pos[1]).all()) else 0))
            tree.kids[v][a] = ch
            return path + [ch], pos, d
        ch = tree.kids[v][a]
        path.append(ch)
        if tree.term[ch]:
            return path, pos, d
        v = ch


def improved_policy(prior, free, n, q, vroot, c_visit, c_scale):
    """float32 [C] from the root's float32 priors, its free cells and their (n, q); all float64"""
    out = np.zeros(len(prior), np.float32)
    if len(free) == 0:
        return out
    p = np.maximum(np.asarray(prior, np.float32)[free], TINY).astype(np.float64)
    pi = p / p.sum()
    q = q.astype(np.float64)
    seen = n > 0
    sv, sq, ns = pi[seen].sum(), (pi[seen] * q[seen]).sum(), float(n.sum())
    vmix = (float(vroot) + ns * sq / sv) / (1.0 + ns) if sv > 0 else float(vroot)
    K = (float(c_visit) + float(n.max())) * float(c_scale)
    y = np.log(p) + K * np.where(seen, q, vmix)
    e = np.exp(y - y.max())
    out[free] = (e / e.sum()).astype(np.float32)
    return out


def gumbel_puct(obs, k, iterations, c, evaluator, considered, c_visit=50.0, c_scale=0.5, gumbel_scale=1.0, seed=0, step=0,
                env_id0=0, deterministic=False, gscore=None, leaves=None):
    """obs: [N, 2, m, n].  Returns (actions int64 [N], visits int32 [N, C], root_value f32 [N], policy f32 [N, C], gscore
    f32 [N, C]).  ``gscore``: the scores to search with instead of the rule's own (a kernel's, to compare the search bit
    for bit); ``leaves``: an optional list that receives (leaf_obs, leaf_mask) of every evaluation."""
    obs = _as_bool(obs)
    N, _, m, n = obs.shape
    C, I = m * n, iterations
    c, c_visit, c_scale = np.float32(c), np.float32(c_visit), np.float32(c_scale)
    table = schedule(considered, I)
    roots = obs.reshape(N, 2, C)
    free = [np.flatnonzero(~(roots[i, 0] | roots[i, 1])) for i in range(N)]
    live = np.array([len(f) > 0 for f in free])
    trees = [_Tree() for _ in range(N)]
    paths = [[0] for _ in range(N)]
    leaf_obs = np.stack([_canonical(roots[i], 0, m, n) for i in range(N)])
    leaf_mask = ~(roots[:, 0] | roots[:, 1])
    pending = np.ones(N, bool)
    vroot = np.zeros(N, np.float32)
    for it in range(I + 1):
        if leaves is not None:
            leaves.append((leaf_obs.copy(), leaf_mask.copy()))
        priors, values = evaluator(leaf_obs.copy(), leaf_mask.copy())
        priors = np.asarray(priors, np.float32).reshape(N, C)
        values = np.asarray(values, np.float32).reshape(N)
        if it == 0:
            vroot = values.copy()
            if gscore is None:
                gscore, _ = gumbel_scores(priors, leaf_mask, 0.0 if deterministic else gumbel_scale, seed, step, env_id0)
        for i in range(N):
            if pending[i]:
                _backup(trees[i], paths[i], priors[i], values[i])
        if it == I:
            break
        for i in range(N):
            if live[i]:
                t = trees[i].n[0] - 1
                want = int(table[min(considered, len(free[i])), t])
                first = _pick(trees[i], free[i], gscore[i], want, c_visit, c_scale)
                paths[i], pos, d = _walk(trees[i], roots[i], m, n, k, c, first)
            else:
                paths[i], pos, d = [0], roots[i], 0
                pending[i] = False
            leaf_obs[i] = _canonical(pos, d, m, n)
            leaf_mask[i] = ~(pos[0] | pos[1])

    x = philox.rand_u32(seed, np.uint64(env_id0) + np.arange(N, dtype=np.uint64), step, philox.STREAM_SAMPLE)
    if deterministic:
        x = np.zeros(N, np.uint64)
    actions = np.zeros(N, np.int64)
    visits = np.zeros((N, C), np.int32)
    root_value = np.zeros(N, np.float32)
    policy = np.zeros((N, C), np.float32)
    for i in range(N):
        t = trees[i]
        root_value[i] = np.float32(-t.w[0]) / np.float32(t.n[0])
        if not live[i]:
            actions[i] = philox.mulhi32(x[i], C)
            continue
        na, _, q = _root_stats(t, free[i])
        visits[i, free[i]] = na
        actions[i] = _pick(t, free[i], gscore[i], None, c_visit, c_scale)
        policy[i] = improved_policy(t.prior[0], free[i], na, q, vroot[i], c_visit, c_scale)
    return actions, visits, root_value, policy, gscore


def ring_counts(policy, free):
    """the ring's u16 visits of a policy row: min(65535, rint(fl32(policy * 65535))) on free cells"""
    v = np.rint((np.asarray(policy, np.float32) * np.float32(65535)).astype(np.float32))
    return np.where(free & (v > 0), np.minimum(v, 65535), 0).astype(np.uint16)


class GumbelSelfPlayRule(SelfPlayRule):
    def step_moves(self, policy, actions, p):
        """one ply of every row from the search's own moves (mnk_search_selfplay_step_moves)"""
        m, n, k, N, T, C = self.m, self.n, self.k, self.N, self.T, self.C
        t = p % T
        for i in range(N):
            s = self.side[i]
            me, other = self.boards[i, s].copy(), self.boards[i, 1 - s].copy()
            occ = me | other
            self.ring_planes[t, 0, :, i] = pack_cells(me[None], m, n)[:, 0]
            self.ring_planes[t, 1, :, i] = pack_cells(other[None], m, n)[:, 0]
            self.ring_visits[t, i] = ring_counts(policy[i], ~occ)
            self.ring_z[t, i] = Z_UNKNOWN
            a = int(actions[i])
            if not 0 <= a < C or occ[a]:
                self.errors.append((ERR_ILLEGAL_MOVE if 0 <= a < C else ERR_ACTION_RANGE, i))
                continue
            g = int(self.moves[i])
            self.boards[i, s, a] = True
            win = bool(has_run(self.boards[i, s].reshape(1, m, n), k)[0])
            done = win or g + 1 >= C
            self.moves[i] = g + 1
            self.side[i] = 1 - s
            if done:
                L = min(g + 1, T)
                for d in range(L):
                    self.ring_z[(t - d) % T, i] = (1 if d % 2 == 0 else -1) if win else 0
                self.stats += [1, int(win and s == 0), int(win and s == 1), int(not win), g + 1]
                self.boards[i] = False
                self.moves[i] = 0
                self.side[i] = 0
        return self.view()
