"""numpy restatement of search self-play (test helper; the rules are stated in include/mnk_hip.h, mnk_search_selfplay_step
and mnk_search_gather).

``SelfPlayRule`` holds N games (absolute planes bool [N, 2, C], plane 0 = black; the move count and the side to move of
every row) and the ring; ``step`` plays one ply of every row from that ply's root visits, exactly as the kernel does.
``gather`` expands ring records under symmetries.  ``sym_perm`` is the cell map of a symmetry.
"""
import numpy as np

from oracle import philox
from oracle.packing import pack_cells, unpack_cells
from playout_rule import has_run

Z_UNKNOWN = -128
STREAM_SELFPLAY = 6
ERR_ACTION_RANGE, ERR_SYMMETRY, ERR_VISITS = 1, 3, 4


def pick_by_visits(n, x, by_count):
    """the move from root visits n (int [C], maximum > 0) and one u32 x: temperature 1 (by_count) or 0"""
    n = np.asarray(n, np.int64)
    if by_count:
        r = int(philox.mulhi32(np.uint64(x), int(n.sum())))
        return int(np.flatnonzero(np.cumsum(n) > r)[0])
    S = np.flatnonzero(n == n.max())
    return int(S[int(philox.mulhi32(np.uint64(x), len(S)))])


def sym_src(s, m, n, r, c):
    """the source cell of output cell (r, c) under symmetry s"""
    if s & 4:
        r, c = c, r
    if s & 1:
        r = m - 1 - r
    if s & 2:
        c = n - 1 - c
    return r, c


def sym_perm(s, m, n):
    """int [C]: output cell a reads source cell perm[a]"""
    out = np.empty(m * n, np.int64)
    for r in range(m):
        for c in range(n):
            rr, cc = sym_src(s, m, n, r, c)
            out[r * n + c] = rr * n + cc
    return out


def sym_ok(s, m, n):
    return 0 <= s < 8 and (s < 4 or m == n)


class SelfPlayRule:
    def __init__(self, m, n, k, N, T):
        self.m, self.n, self.k, self.N, self.T, self.C = m, n, k, N, T, m * n
        self.W = (m * (n + 1) + 63) // 64
        self.boards = np.zeros((N, 2, self.C), bool)
        self.moves = np.zeros(N, np.int64)
        self.side = np.zeros(N, np.int64)
        self.ring_planes = np.zeros((T, 2, self.W, N), np.uint64)
        self.ring_visits = np.zeros((T, N, self.C), np.uint16)
        self.ring_z = np.full((T, N), Z_UNKNOWN, np.int8)
        self.stats = np.zeros(5, np.int64)  # games, black wins, white wins, draws, sum of lengths
        self.errors = []

    def load(self, planes, meta):
        """the env's state: planes u64 [2, W, N], meta u32 [N]"""
        for p in (0, 1):
            self.boards[:, p] = unpack_cells(planes[p], self.m, self.n).astype(bool)
        meta = np.asarray(meta, np.int64) & 0xFFFFFFFF
        self.moves, self.side = meta >> 1, meta & 1

    def meta(self):
        return (self.moves << 1) | self.side

    def planes(self):
        return np.stack([pack_cells(self.boards[:, p], self.m, self.n) for p in (0, 1)])

    def view(self):
        """the next roots: canonical obs f32 [N, 2, m, n] and legal mask bool [N, C]"""
        s = self.side
        idx = np.arange(self.N)
        me, other = self.boards[idx, s], self.boards[idx, 1 - s]
        obs = np.stack([me, other], axis=1).reshape(self.N, 2, self.m, self.n).astype(np.float32)
        return obs, ~(me | other)

    def step(self, visits, temp_plies, seed, p, env_id0=0):
        m, n, k, N, T, C = self.m, self.n, self.k, self.N, self.T, self.C
        t = p % T
        x = philox.rand_u32(seed, np.uint64(env_id0) + np.arange(N, dtype=np.uint64), p, STREAM_SELFPLAY)
        visits = np.asarray(visits, np.int64).reshape(N, C)
        for i in range(N):
            s = self.side[i]
            me, other = self.boards[i, s].copy(), self.boards[i, 1 - s].copy()
            occ = me | other
            na = np.where(occ | (visits[i] <= 0), 0, np.minimum(visits[i], 65535))
            self.ring_planes[t, 0, :, i] = pack_cells(me[None], m, n)[:, 0]
            self.ring_planes[t, 1, :, i] = pack_cells(other[None], m, n)[:, 0]
            self.ring_visits[t, i] = na
            self.ring_z[t, i] = Z_UNKNOWN
            if na.max() == 0:
                self.errors.append((ERR_VISITS, i))
                continue
            g = int(self.moves[i])
            a = pick_by_visits(na, x[i], g < temp_plies)
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


def gather(ring_planes, ring_visits, ring_z, m, n, idx, sym):
    """(obs f32 [B, 2, m, n], mask bool [B, C], policy f32 [B, C], value f32 [B], weight f32 [B], errors)"""
    T, _, W, N = ring_planes.shape
    C = m * n
    B = len(idx)
    obs = np.zeros((B, 2, C), np.float32)
    policy = np.zeros((B, C), np.float32)
    value = np.zeros(B, np.float32)
    weight = np.zeros(B, np.float32)
    errors = []
    for b in range(B):
        flat = int(idx[b])
        if flat < 0:
            flat += T * N
        if not 0 <= flat < T * N:
            errors.append((ERR_ACTION_RANGE, int(idx[b])))
            continue
        s = 0 if sym is None else int(sym[b])
        ok = sym_ok(s, m, n)
        if not ok:
            errors.append((ERR_SYMMETRY, b))
            s = 0
        t, i = divmod(flat, N)
        perm = sym_perm(s, m, n)
        for ch in (0, 1):
            cells = unpack_cells(ring_planes[t, ch, :, i:i + 1], m, n)[0]
            obs[b, ch] = cells[perm]
        v = ring_visits[t, i].astype(np.int64)
        tot = int(v.sum())
        if tot:
            policy[b] = v[perm].astype(np.float32) / np.float32(tot)
        z = int(ring_z[t, i])
        if z != Z_UNKNOWN:
            value[b] = z
            weight[b] = 1.0 if ok else 0.0
    mask = (obs[:, 0] == 0) & (obs[:, 1] == 0)
    return obs.reshape(B, 2, m, n), mask, policy, value, weight, errors
