"""CPU: the float64 restatement of the masked draw (tests/draw_rule.py) -- its probabilities against the reference's
masked ``Categorical`` (tests/golden/masked_logits.npz), its checker against draws that are right and draws that are wrong
in the ways a kernel goes wrong (neighbouring cell, neighbouring lane, row-major walk, masked cell, the log-prob of an
exponent scaled by a rounded -rowmax * log2 e), and the search for Philox row ids at both ends of the uniform."""
import numpy as np
import pytest

import draw_rule as dr


def _rows(C, n, seed, scale=3.0):
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal((n, C)) * scale).astype(np.float32)
    mask = rng.random((n, C)) < rng.uniform(0.2, 1.0, size=(n, 1))
    mask[::7] = True
    return logits, mask


def _emulate_f32(logits, mask, u, fma_bias=False):
    """the kernel's arithmetic in numpy f32: weights 2^((l - rowmax) * log2 e) (``fma_bias``: 2^fma(l, log2 e, RN(-rowmax *
    log2 e)), the form before the fix), serial sums per lane, lanes in order, the count of a lane's cells at or below
    u * total; log-prob l_a - rowmax - log(total).  (Lane totals are summed serially here, not by the butterfly.)"""
    n, C = mask.shape
    lpr, k = dr.shape(C)
    f = np.float32
    l = np.where(mask, logits, -np.inf).astype(f)
    dead = ~mask.any(axis=1)
    l[dead] = 0.0
    m = l.max(axis=1, keepdims=True)
    log2e = f(1.4426950408889634)
    with np.errstate(invalid="ignore", over="ignore"):
        if fma_bias:
            bias = (-m * log2e).astype(f)
            arg = (l.astype(np.float64) * np.float64(log2e) + bias).astype(f)  # one rounding, like the FMA
        else:
            arg = ((l - m).astype(f) * log2e).astype(f)
        w = np.exp2(arg).astype(f)
    slots = np.full((n, lpr * k), 0.0, dtype=f)
    slots[:, :C] = w
    lanes = slots.reshape(n, k, lpr).transpose(0, 2, 1)        # [row, lane, slot]
    run = np.cumsum(lanes, axis=2, dtype=f)
    mine = run[:, :, -1]
    base = np.concatenate([np.zeros((n, 1), f), np.cumsum(mine, axis=1, dtype=f)[:, :-1]], axis=1)
    total = (base[:, -1] + mine[:, -1]).astype(f)
    target = (np.asarray(u, f) * total).astype(f)
    run = (base[:, :, None] + run).astype(f)
    cnt = (run <= target[:, None, None]).sum(axis=2)
    passes = (run[:, :, -1] > target[:, None]) & (base <= target[:, None]) & (mine > 0)
    owner = np.argmax(passes, axis=1)
    rows = np.arange(n)
    cnt = np.minimum(cnt[rows, owner], k - 1)
    # no lane holds the point (rounding left it at or beyond the total): the last cell with weight of the last such lane
    heavy = mine > 0
    last_lane = np.where(heavy.any(axis=1), lpr - 1 - np.argmax(heavy[:, ::-1], axis=1), 0)  # (no weight at all: cell 0)
    slot_w = lanes[rows, last_lane] > 0
    last_slot = np.where(slot_w.any(axis=1), k - 1 - np.argmax(slot_w[:, ::-1], axis=1), 0)
    none = ~passes.any(axis=1)
    owner, cnt = np.where(none, last_lane, owner), np.where(none, last_slot, cnt)
    act = owner + lpr * cnt
    with np.errstate(divide="ignore"):
        logp = (l[rows, act] - m[:, 0] - np.log(total)).astype(f)
    return act, logp


def test_probabilities_match_the_reference_head(golden_dir):
    """float64 probabilities of the reference nets' masked logits == the probabilities the reference's masked Categorical
    stored (f32), all-masked rows included"""
    g = np.load(f"{golden_dir}/masked_logits.npz")
    for arch in ("cnn_b_s", "resnet_b_s"):
        ref = dr.Reference(g[arch + "_raw_logits"], g[arch + "_mask"])
        want = g[arch + "_probs"].astype(np.float64)
        # torch's f32 softmax: exp (~2 u), a tree sum of 81 terms (~7 u), the division (1 u)
        assert np.allclose(ref.p, want, rtol=16 * dr.F32_EPS, atol=1e-12)
        assert np.allclose(ref.p.sum(axis=1), 1.0, rtol=0, atol=1e-12)


def test_shape_table_and_lane_major_order():
    assert [dr.shape(c) for c in (1, 9, 32, 33, 81, 96, 97, 169, 225, 256, 257, 361, 512, 513, 1024)] == [
        (4, 8), (4, 3), (4, 8), (8, 12), (4, 21), (8, 12), (16, 16), (8, 22), (16, 15), (16, 16), (32, 16), (16, 23),
        (32, 16), (32, 32), (32, 32)]
    for C in range(1, 1025):
        lpr, k = dr.shape(C)
        assert lpr * k >= C
    assert dr.lane_major(9, 4).tolist() == [0, 4, 8, 1, 5, 2, 6, 3, 7]


@pytest.mark.parametrize("C", [9, 33, 81, 361, 1024])
def test_checker_passes_the_exact_answer_and_flags_every_corruption(C):
    n = 20000
    logits, mask = _rows(C, n, C)
    ref = dr.Reference(logits, mask)
    u = dr.row_uniforms(5, 0, n, 3)
    exact, ambiguous = ref.inverse_cdf(u)
    logp = ref.logp[np.arange(n), exact].astype(np.float32)
    bad, amb = dr.check(ref, exact, logp, u)
    assert not bad.any() and np.array_equal(amb, ambiguous)
    rate_amb = amb.mean()
    assert rate_amb < 0.02

    lpr = ref.lpr
    pos = np.argsort(ref.order)                                     # position of each cell in the walk
    # the neighbouring cell of the walk
    p = pos[exact]
    nb = ref.order[np.where(p + 1 < C, p + 1, p - 1)]
    # the neighbouring lane, same slot
    lane = np.where((exact % lpr == lpr - 1) | (exact + 1 >= C), exact - 1, exact + 1)
    # the inverse CDF walked row-major
    cum = np.cumsum(ref.p, axis=1)
    rowmajor = np.minimum((cum <= u[:, None]).sum(axis=1), C - 1)
    # a masked cell (rows that have one and a legal one: on an all-masked row every cell is legal)
    has_masked = ~mask.all(axis=1) & mask.any(axis=1)
    masked = np.argmax(~mask, axis=1)
    for name, wrong, rows in (("walk neighbour", nb, slice(None)), ("lane neighbour", lane, slice(None)),
                              ("row-major", rowmajor, slice(None)), ("masked", masked, has_masked)):
        wrong = np.asarray(wrong)
        differs = (wrong != exact)[rows]
        lp = ref.logp[np.arange(n), np.clip(wrong, 0, C - 1)].astype(np.float32)
        bad, _ = dr.check(ref, wrong, lp, u)
        bad = bad[rows]
        assert bad[differs].mean() > 0.95, name                    # a draw that moved is caught ...
        assert bad.mean() > 20 * rate_amb or rate_amb == 0, name   # ... far more often than draws are ambiguous
        if name == "masked":
            assert bad.all()
    # the deterministic draw: ties to the lowest cell
    tie = np.zeros((4, C), np.float32)
    tie[:, -1] = 1.0
    tie[1, C // 2] = 1.0
    tie[2, 0] = -0.0
    tm = np.ones((4, C), bool)
    tm[3] = False
    tref = dr.Reference(tie, tm)
    want = np.array([C - 1, min(C // 2, C - 1), C - 1, 0])
    assert not dr.check(tref, want, None)[0].any()
    assert dr.check(tref, (want + 1) % C, None)[0][:2].all()


@pytest.mark.parametrize("C", [9, 81, 361, 1024])
def test_checker_passes_the_f32_arithmetic_and_fails_a_scaled_exponent(C):
    """an f32 emulation of the kernel's arithmetic passes, at logits of any size; the form before the fix (an FMA against a
    rounded -rowmax * log2 e) fails the log-prob bound once |rowmax| is large (1e6: off by ~0.015 nats), and at 1e10 its
    weights all vanish or overflow"""
    n = 4000
    logits, mask = _rows(C, n, 7 + C)
    u = dr.row_uniforms(9, 100, n, 0)
    for off in (0.0, -1e3, 1e6, -1e9, 1e10, -3e38):
        lg = (logits + np.float32(off)).astype(np.float32)
        ref = dr.Reference(lg, mask)
        act, lp = _emulate_f32(lg, mask, u)
        bad, amb = dr.check(ref, act, lp, u)
        assert not bad.any(), (off, np.flatnonzero(bad)[:5])
        assert amb.mean() < 0.02
    lg = (logits + np.float32(-1e6)).astype(np.float32)
    act, lp = _emulate_f32(lg, mask, u, fma_bias=True)
    assert dr.check(dr.Reference(lg, mask), act, lp, u)[0].mean() > 0.5
    lg = (logits + np.float32(1e10)).astype(np.float32)
    with np.errstate(invalid="ignore"):
        act, lp = _emulate_f32(lg, mask, u, fma_bias=True)
    live = mask.any(axis=1)  # (an all-masked row draws over zeros: no rowmax to get wrong)
    assert dr.check(dr.Reference(lg, mask), act, lp, u)[0][live].all()


def test_philox_row_ids_at_both_ends_of_the_uniform():
    seed, step = 1234, 5
    top = dr.find_row_ids(seed, step, 6, near_one=True)
    bottom = dr.find_row_ids(seed, step, 6, near_one=False)
    assert len(set(top.tolist())) == 6 and len(set(bottom.tolist())) == 6
    for ids, near_one in ((top, True), (bottom, False)):
        u = np.array([dr.row_uniforms(seed, int(i), 1, step)[0] for i in ids], dtype=np.float64)
        assert ((1.0 - u < 2.0 ** -18) if near_one else (u < 2.0 ** -18)).all()
    # consecutive rows from an env_id0 see consecutive Philox ids
    assert np.array_equal(dr.row_uniforms(seed, int(top[0]) - 3, 5, step)[3:4], dr.row_uniforms(seed, int(top[0]), 1, step))
