"""float64 restatement of the masked categorical draw (test helper; the kernel is ``draw_row`` in csrc/mnk_draw.h).

A row of C cells is drawn by LPR lanes, lane s owning the cells s, s + LPR, ..., K of them.  The inverse-CDF walk is
lane-major: cells sorted by ``(c % LPR, c // LPR)``.  The row's uniform u in (0, 1) picks the first cell in that order
whose cumulative probability exceeds u; a deterministic draw is the argmax over the legal cells, ties to the lowest cell.
Every draw is a function of (logits, mask, u), so each one can be checked on its own against the float64 answer here,
with a tolerance built from the f32 error terms of the kernel's arithmetic (``eps_cdf`` / ``logp_bound``).

Inputs are what the kernel sees: f32 logits, bf16 logits widened exactly to f32, or no logits (all zero), plus the mask.
A row without a legal cell is uniform over all C cells (alg/architectures/cnn.py:76-77).
"""
import numpy as np

from oracle.philox import STREAM_SAMPLE, rand_u32, uniform_open01

F32_EPS = 2.0 ** -24  # unit roundoff of f32


def shape(C: int):
    """(LPR, K) of a row of C cells: ``shape_lpr`` / ``shape_k`` of csrc/mnk_draw.h, the buckets of ``dispatch_sample`` in
    csrc/mnk_sample.hip.  The five measured widths (3x3, 9x9, 13x13, 15x15, 19x19) have their own shapes; every other
    width takes ``Shape<32 | 96 | 256 | 512 | 1024>``."""
    measured = {9: (4, 3), 81: (4, 21), 169: (8, 22), 225: (16, 15), 361: (16, 23)}
    if C in measured:
        return measured[C]
    for top, lpr, k in ((32, 4, 8), (96, 8, 12), (256, 16, 16), (512, 32, 16), (1024, 32, 32)):
        if C <= top:
            return lpr, k
    raise ValueError(f"row width {C} above 1024")


def lane_major(C: int, lpr: int) -> np.ndarray:
    """the cells of a row in the order of the inverse-CDF walk: sorted by (c % LPR, c // LPR)"""
    c = np.arange(C)
    return np.lexsort((c // lpr, c % lpr))


def row_uniforms(seed: int, env_id0: int, rows: int, step: int) -> np.ndarray:
    """f32 uniform of each row: stream SAMPLE, Philox row id env_id0 + row, step = the sampler's ``calls``"""
    ids = np.uint64(env_id0) + np.arange(rows, dtype=np.uint64)
    return uniform_open01(rand_u32(seed, ids, step, STREAM_SAMPLE))


def find_row_ids(seed: int, step: int, count: int, near_one: bool, margin=2.0 ** -18, start=0, block=1 << 20):
    """the first ``count`` Philox row ids >= start whose uniform lies within ``margin`` of 1 (``near_one``) or of 0"""
    found = []
    lo = start
    while len(found) < count:
        u = row_uniforms(seed, lo, block, step).astype(np.float64)
        hit = np.flatnonzero(u > 1.0 - margin if near_one else u < margin)
        found.extend((lo + hit).tolist())
        lo += block
        if lo - start > (1 << 26):
            raise RuntimeError("no Philox row ids found at that end of the uniform")
    return np.asarray(found[:count], dtype=np.int64)


class Reference:
    """float64 probabilities, lane-major cumulative bounds and log-probabilities of rows of masked logits.

    logits: f32 [N, C] (bf16 already widened) or None (all zero); mask: bool [N, C]."""

    def __init__(self, logits, mask):
        mask = np.asarray(mask, dtype=bool)
        n, C = mask.shape
        self.C = C
        self.lpr, self.k = shape(C)
        x = np.zeros((n, C)) if logits is None else np.asarray(logits, dtype=np.float32).astype(np.float64)
        self.none_legal = ~mask.any(axis=1)
        self.legal = mask | self.none_legal[:, None]
        x = np.where(mask, x, -np.inf)
        x[self.none_legal] = 0.0
        self.x = x
        self.rowmax = x.max(axis=1)
        d = x - self.rowmax[:, None]                      # <= 0, -inf where masked
        w = np.exp(d)
        total = w.sum(axis=1)
        self.p = w / total[:, None]
        with np.errstate(divide="ignore"):
            self.logp = d - np.log(total)[:, None]         # -inf where masked
        # E_p |l - rowmax|: scales the rounding error of the exponent's argument (see eps)
        self.spread = np.where(self.p > 0, self.p * -np.where(np.isfinite(d), d, 0.0), 0.0).sum(axis=1)
        order = lane_major(C, self.lpr)
        p_ord = self.p[:, order]
        hi_ord = np.cumsum(p_ord, axis=1)
        self.order = order
        self.p_ord, self.hi_ord = p_ord, hi_ord
        self.f_hi = np.empty_like(hi_ord)
        self.f_hi[:, order] = hi_ord
        self.f_lo = self.f_hi - self.p

    def eps_cdf(self) -> np.ndarray:
        """per-row tolerance of the draw on the cumulative axis, relative to the row's total weight.

        (2K + log2 LPR + 8) u: K serial adds of a lane's weights and K more of its running count, log2 LPR scan levels,
        u * total_w, one ulp of v_exp_f32 per weight, and slack.  Plus 3 E_p|l - rowmax| u: every weight is 2 to the
        power of (l - rowmax) * log2 e, whose three roundings (the difference, the product, log2 e itself) move the weight
        by a relative |l - rowmax| u each; summed over a prefix of the walk that is at most E_p|l - rowmax| per rounding.
        No term in |rowmax|: the kernel forms l - rowmax first."""
        return (2 * self.k + np.log2(self.lpr) + 8 + 3 * self.spread) * F32_EPS

    def inverse_cdf(self, u):
        """(exact answer, ambiguous): the float64 inverse-CDF cell for u per row, and whether u lies within eps_cdf of a
        boundary between two cells of positive probability"""
        u = np.asarray(u, dtype=np.float64)[:, None]
        pos = self.p_ord > 0
        last = self.C - 1 - np.argmax(pos[:, ::-1], axis=1)                 # last cell of positive probability, in order
        k = ((self.hi_ord <= u) & pos).sum(axis=1)                          # positive cells that end at or below u
        # the k-th positive cell in order (0-based): the first position whose running count of positive cells is k + 1
        rank = np.cumsum(pos, axis=1)
        at = np.argmax(rank > k[:, None], axis=1)
        at = np.where(k >= rank[:, -1], last, at)
        exact = self.order[at]
        interior = pos & (np.arange(self.C)[None, :] != last[:, None])      # boundaries between two positive cells
        near = interior & (np.abs(self.hi_ord - u) <= self.eps_cdf()[:, None])
        return exact, near.any(axis=1)

    def argmax(self) -> np.ndarray:
        """the deterministic draw: argmax over the legal cells (numpy's first maximum: ties to the lowest cell, -0 == +0)"""
        return np.argmax(self.x, axis=1)

    def logp_bound(self, actions) -> np.ndarray:
        """|logp - log p64(a)| allowed per row: u (|l_a - rowmax| + |log p64(a)| + K + log2 LPR + 20 + 3 E_p|l - rowmax|).
        |l_a - rowmax| for the rounding of that difference, |log p64(a)| for the rounding of the result, K + log2 LPR for
        the lane sums and the butterfly behind total_w, 20 for v_exp_f32, logf and slack, and the exponent arguments'
        roundings as in eps_cdf.  Deliberately no |rowmax| term: the kernel must not carry an error in the size of the
        logits themselves."""
        rows = np.arange(len(actions))
        la = self.x[rows, actions] - self.rowmax
        lp = self.logp[rows, actions]
        return (np.abs(la) + np.abs(lp) + self.k + np.log2(self.lpr) + 20 + 3 * self.spread) * F32_EPS


def check(ref: Reference, actions, logp, u=None):
    """Per-draw check of a kernel's (actions, logp) against ``ref``; ``u`` = the rows' uniforms, None for deterministic
    draws.  Returns (bad bool [N], ambiguous bool [N]); every reason a draw can fail is folded into ``bad``:
    out of range, not legal, float64 probability 0, outside [F_lo - eps, F_hi + eps], not the exact answer while
    unambiguous (deterministic: not the argmax), log-prob outside ``logp_bound`` (when ``logp`` is given)."""
    a = np.asarray(actions).astype(np.int64)
    n, C = ref.p.shape
    rows = np.arange(n)
    ok_range = (a >= 0) & (a < C)
    a_ = np.where(ok_range, a, 0)
    bad = ~ok_range | ~ref.legal[rows, a_] | ~(ref.p[rows, a_] > 0)
    if u is None:
        ambiguous = np.zeros(n, dtype=bool)
        bad |= a_ != ref.argmax()
    else:
        u64 = np.asarray(u, dtype=np.float64)
        eps = ref.eps_cdf()
        exact, ambiguous = ref.inverse_cdf(u64)
        bad |= (u64 < ref.f_lo[rows, a_] - eps) | (u64 > ref.f_hi[rows, a_] + eps)
        bad |= ~ambiguous & (a_ != exact)
    if logp is not None:
        lp = np.asarray(logp, dtype=np.float64)
        want = ref.logp[rows, a_]
        with np.errstate(invalid="ignore"):
            bad |= ~(np.abs(lp - want) <= ref.logp_bound(a_))
    return bad, ambiguous
