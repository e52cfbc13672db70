"""CPU: the PUCT player's Gumbel root -- the host-side table of considered visits (``mnk_puct_gumbel_schedule``) against
the numpy rule (tests/puct_gumbel_rule.py) and as a schedule that can always be followed; the argument checks of the
policy and of the C ABI, none of which needs a GPU; and the rule itself: with one simulation its move is a Gumbel-max
sample of the priors, with exact values it finds the winning move and its improved policy peaks there, and the improved
policy is a distribution over the free cells."""
import numpy as np
import pytest

from player_cases import check_header_and_binding, header_constants, lib  # noqa: F401 (lib: the fixture)
from playout_rule import has_run
from puct_gumbel_rule import gumbel_puct, gumbel_scores, schedule
from puct_solver_rule import negamax, value_after
from tactical_rule import random_positions

M_VALUES, I_VALUES = (1, 2, 3, 4, 8, 16), (1, 5, 8, 16, 50)


# ----------------------------------------------------------------------------- 1. the schedule
def host_schedule(lib, m, I):
    out = np.full((m + 1, I), 0xFFFF, np.uint16)
    lib.call("mnk_puct_gumbel_schedule", m, I, out.ctypes.data)
    return out


@pytest.mark.parametrize("I", I_VALUES)
@pytest.mark.parametrize("m", M_VALUES)
def test_the_host_schedule_equals_the_rule(lib, m, I):
    got = host_schedule(lib, m, I)
    assert np.array_equal(got, schedule(m, I)), (m, I, got)
    assert np.array_equal(got, lib.puct_gumbel_schedule(m, I))
    assert np.array_equal(got[0], np.arange(I)) and np.array_equal(got[1], np.arange(I))


def test_the_worked_example(lib):
    assert host_schedule(lib, 4, 8)[4].tolist() == [0, 0, 0, 0, 1, 1, 2, 2]
    assert schedule(4, 8)[4].tolist() == [0, 0, 0, 0, 1, 1, 2, 2]


@pytest.mark.parametrize("I", I_VALUES)
@pytest.mark.parametrize("m", M_VALUES)
def test_every_row_can_be_followed_whatever_the_tie_break(lib, m, I):
    """a root of F >= m' free cells that visits, in simulation t, ANY cell whose count is table[m'][t] always finds one"""
    table = host_schedule(lib, m, I)
    rng = np.random.default_rng(m * 100 + I)
    for mp in range(1, m + 1):
        for F in (mp, mp + 1, mp + 7):
            for _ in range(4):
                n = np.zeros(F, np.int64)
                for t in range(I):
                    cand = np.flatnonzero(n == table[mp, t])
                    assert len(cand), (mp, F, t, n, table[mp])
                    n[rng.choice(cand)] += 1


def test_the_schedule_rejects_bad_arguments(lib):
    out = np.zeros((1025, 8), np.uint16)
    for m, I, p in ((0, 8, out.ctypes.data), (1025, 8, out.ctypes.data), (4, 0, out.ctypes.data), (4, 2049, out.ctypes.data),
                    (4, 8, None), (-1, 8, out.ctypes.data)):
        with pytest.raises(lib.MnkHipError, match="mnk_puct_gumbel_schedule"):
            lib.call("mnk_puct_gumbel_schedule", m, I, p)
    assert not out.any()


# ----------------------------------------------------------------------------- 2. the C ABI and the policy's checks
def test_header_declares_the_entry_points_and_the_binding_matches(lib):
    for name in ("mnk_puct_gumbel_schedule", "mnk_puct_gumbel_root", "mnk_puct_step_gumbel",
                 "mnk_search_selfplay_step_moves"):
        check_header_and_binding(lib, name)
    consts = header_constants()
    assert consts["MNK_STREAM_GUMBEL"] == "8" == str(lib.STREAM_GUMBEL)
    assert consts["MNK_PUCT_CONSIDERED_MAX"] == "1024" == str(lib.PUCT_CONSIDERED_MAX)
    assert len(lib.SIGNATURES["mnk_puct_step_gumbel"]) == len(lib.SIGNATURES["mnk_puct_step_leaves"]) + 6


def test_the_host_rejects_bad_arguments_and_enqueues_nothing(lib):
    """(the fake device pointers are never dereferenced: nothing is launched when a check fails or N = 0)"""
    p = 0x1000

    def step(ws=p, N=8, m=9, n=9, k=5, I=16, L=1, pr=p, pdt=0, va=p, vdt=0, c=1.25, last=0, cons=4, cv=50.0, cs=0.5, tab=p,
             gs=p, vr=p, lo=p, ldt=0, lm=p, acts=p, pol=None):
        return lib.call("mnk_puct_step_gumbel", ws, N, m, n, k, I, L, pr, pdt, va, vdt, c, last, cons, cv, cs, tab, gs, vr,
                        1, None, 0, None, 0, 0, lo, ldt, lm, acts, None, None, pol, None)

    for bad in (dict(ws=None), dict(pr=None), dict(va=None), dict(N=-1), dict(pdt=2), dict(vdt=-1), dict(I=0), dict(I=2049),
                dict(c=-0.5), dict(c=float("nan")), dict(last=2), dict(L=0), dict(L=2), dict(L=16), dict(cons=0),
                dict(cons=1025), dict(cv=-1.0), dict(cv=float("inf")), dict(cs=float("nan")), dict(cs=-0.5), dict(tab=None),
                dict(gs=None), dict(lo=None), dict(lm=None), dict(ldt=3), dict(last=1, acts=None),
                dict(last=1, pol=p, vr=None), dict(k=10), dict(m=40, n=40)):
        with pytest.raises(lib.MnkHipError, match="mnk_puct_step_gumbel"):
            step(**bad)
    assert step(N=0) == 0 and step(N=0, last=1, lo=None, lm=None, ldt=9, pol=p) == 0

    def root(pr=p, pdt=0, mk=p, va=p, vdt=0, N=8, C=81, scale=1.0, step=0, gs=p, vr=p):
        return lib.call("mnk_puct_gumbel_root", pr, pdt, mk, va, vdt, N, C, scale, 1, None, step, None, 0, gs, vr, None)

    for bad in (dict(pr=None), dict(mk=None), dict(va=None), dict(gs=None), dict(vr=None), dict(N=-1), dict(C=0),
                dict(C=1025), dict(pdt=2), dict(vdt=2), dict(scale=-1.0), dict(scale=float("nan")), dict(step=1 << 60)):
        with pytest.raises(lib.MnkHipError, match="mnk_puct_gumbel_root"):
            root(**bad)
    assert root(N=0) == 0

    def moves(pl=p, me=p, N=8, m=3, n=3, k=3, pol=p, acts=p, T=9, rp=p, rv=p, rz=p, obs=p, odt=0):
        return lib.call("mnk_search_selfplay_step_moves", pl, me, N, m, n, k, pol, acts, 0, None, T, rp, rv, rz, obs, odt,
                        None, None, None, None)

    for bad in (dict(pl=None), dict(me=None), dict(pol=None), dict(acts=None), dict(rp=None), dict(rv=None), dict(rz=None),
                dict(obs=None), dict(N=-1), dict(T=8), dict(odt=3), dict(k=10)):
        with pytest.raises(lib.MnkHipError, match="mnk_search_selfplay_step_moves"):
            moves(**bad)
    assert moves(N=0) == 0


def test_the_policy_refuses_what_gumbel_does_not_combine_with(lib):
    import torch

    from selfplay.policy import PUCTSearchPolicy
    from selfplay.search_selfplay import SearchSelfPlay

    ev = lambda o, msk: (msk.float(), torch.zeros(len(msk)))  # noqa: E731
    for kw in (dict(reuse=True), dict(leaves=2), dict(solver=True), dict(root_noise=(0.3, 0.25)), dict(temperature=1)):
        with pytest.raises(ValueError, match="gumbel"):
            PUCTSearchPolicy(3, evaluator=ev, iterations=16, gumbel=4, **kw)
        PUCTSearchPolicy(3, evaluator=ev, iterations=16, **kw)  # (each is fine without gumbel)
    for kw in (dict(gumbel=0), dict(gumbel=1025), dict(gumbel=2.5), dict(gumbel=True), dict(gumbel=4, gumbel_c=(50.0,)),
               dict(gumbel=4, gumbel_c=(-1.0, 0.5)), dict(gumbel=4, gumbel_c=(50.0, float("nan"))),
               dict(gumbel=4, gumbel_scale=-1.0), dict(gumbel=4, gumbel_scale=float("inf")), dict(gumbel=4, gumbel_scale="x")):
        with pytest.raises(ValueError, match="gumbel"):
            PUCTSearchPolicy(3, evaluator=ev, iterations=16, **kw)
    pol = PUCTSearchPolicy(3, evaluator=ev, iterations=16, gumbel=4)
    assert pol.gumbel == 4 and pol.gumbel_c == (50.0, 0.5) and pol.gumbel_scale == 1.0 and pol.evaluations_per_act == 17
    plain = PUCTSearchPolicy(3, evaluator=ev, iterations=16)
    assert plain.gumbel is None and plain._gumbel_bufs is None
    with pytest.raises(ValueError, match="gumbel"):  # the output needs the search that computes it
        plain.act({"observation": torch.zeros((2, 2, 3, 3))}, policy=torch.zeros((2, 9)))
    with pytest.raises(ValueError, match="gumbel"):
        SearchSelfPlay(3, 3, 3, 4, evaluator=ev, iterations=8, gumbel=4, reuse=True, device="cpu")
    assert "temp_plies`` is then not read" in __import__("selfplay.search_selfplay").search_selfplay.__doc__


# ----------------------------------------------------------------------------- 3. Gumbel-max on the rule
def chi2_critical(df, alpha):
    """the value a chi-square variable of ``df`` degrees exceeds with probability ``alpha``: scipy's survival function
    inverted, else the Wilson-Hilferty cube approximation"""
    try:
        from scipy.stats import chi2

        return float(chi2.isf(alpha, df))
    except ImportError:
        from statistics import NormalDist

        z = NormalDist().inv_cdf(1.0 - alpha)
        return df * (1.0 - 2.0 / (9.0 * df) + z * np.sqrt(2.0 / (9.0 * df))) ** 3


def test_with_one_simulation_the_move_is_a_gumbel_max_sample_of_the_priors():
    """I = 1: the one simulation goes to argmax(g + ln P), which is then the only visited cell and the move -- a sample
    from the normalised priors.  20 000 rows on the empty 3x3x3 board, chi-square at significance 1e-6 (8 degrees)."""
    rows, C = 20000, 9
    prior = np.array([0.30, 0.02, 0.10, 0.05, 0.20, 0.03, 0.15, 0.07, 0.08], np.float32)

    def ev(leaf_obs, leaf_mask):
        return leaf_mask * prior, np.zeros(len(leaf_mask), np.float32)

    obs = np.zeros((rows, 2, 3, 3), np.float32)
    actions, visits, _, policy, gscore = gumbel_puct(obs, 3, 1, 1.25, ev, 4, seed=20221, step=3, env_id0=11)
    assert np.array_equal(actions, np.argmax(gscore, axis=1))
    assert (visits.sum(axis=1) == 1).all() and (visits[np.arange(rows), actions] == 1).all()
    want = prior.astype(np.float64) / prior.astype(np.float64).sum() * rows
    got = np.bincount(actions, minlength=C)
    stat = float(((got - want) ** 2 / want).sum())
    crit = chi2_critical(C - 1, 1e-6)
    print("chi-square %.2f, critical %.2f, counts %s" % (stat, crit, got))
    assert 40.0 < crit < 46.0  # (chi2.isf(1e-6, 8) = 42.70; Wilson-Hilferty gives 42.4)
    assert stat < crit
    # and the draw is keyed: the same key the same moves, another step other moves
    again = gumbel_puct(obs[:64], 3, 1, 1.25, ev, 4, seed=20221, step=3, env_id0=11)[0]
    other = gumbel_puct(obs[:64], 3, 1, 1.25, ev, 4, seed=20221, step=4, env_id0=11)[0]
    assert np.array_equal(again, actions[:64]) and not np.array_equal(other, actions[:64])
    det = gumbel_puct(obs[:4], 3, 1, 1.25, ev, 4, seed=20221, step=3, deterministic=True)
    assert (det[0] == 0).all()  # gumbel_scale = 0: the largest prior


# ----------------------------------------------------------------------------- 4. policy improvement on the rule
def exact_values(m, n, k):
    """uniform priors over the legal cells, and the negamax value of the leaf for its side to move"""
    def ev(leaf_obs, leaf_mask):
        flat = leaf_obs.reshape(len(leaf_obs), 2, -1) != 0
        values = np.zeros(len(flat), np.float32)
        for i, pos in enumerate(flat):
            over = has_run(pos.reshape(2, m, n), k).any() or not leaf_mask[i].any()
            if not over:  # (a terminal leaf's value is never read)
                values[i] = negamax(pos, m, n, k)
        return leaf_mask / np.maximum(leaf_mask.sum(axis=1, keepdims=True), 1).astype(np.float32), values

    return ev


def unique_wins(m, n, k, rows, seed):
    """``rows`` random positions of 2 .. 7 free cells that are won for the side to move by exactly one move, and that move"""
    rng, out, wins = np.random.default_rng(seed), [], []
    while len(out) < rows:
        o = random_positions(m, n, k, 1, rng, max_fill=1.0)[0]
        flat = o.reshape(2, -1) != 0
        free = np.flatnonzero(~(flat[0] | flat[1]))
        if not 2 <= len(free) <= 7:
            continue
        good = [a for a in free if value_after(flat, a, m, n, k) == 1]
        if len(good) == 1:
            out.append(o)
            wins.append(good[0])
    return np.stack(out), np.array(wins)


def test_with_exact_values_the_move_and_the_policy_find_the_one_winning_move():
    """3x3x3, uniform priors, exact values, I = 16, m = 4, gumbel_scale = 0.  Without Gumbel noise and with uniform priors
    every gscore ties, so the root considers its 4 lowest free cells and no other cell is ever visited: the move can be
    the winning cell only where that cell is considered.  The roots are therefore those on which it is -- all roots of at
    most 4 free cells, and the roots of 5 .. 7 free cells whose winning cell is among the 4 lowest (59 of the 64 drawn
    in all)."""
    m, n, k = 3, 3, 3
    obs, wins = unique_wins(m, n, k, 64, 5)
    flat = obs.reshape(len(obs), 2, -1) != 0
    considered = np.array([w in np.flatnonzero(~(f[0] | f[1]))[:4] for f, w in zip(flat, wins)])
    print("roots", len(obs), "with the winning cell considered", int(considered.sum()))
    assert considered.sum() >= 48 and ((~(flat[:, 0] | flat[:, 1])).sum(axis=1) > 4).sum() >= 16
    obs, wins = obs[considered], wins[considered]
    actions, visits, root_value, policy, _ = gumbel_puct(obs, k, 16, 1.25, exact_values(m, n, k), 4, gumbel_scale=0.0)
    assert np.array_equal(actions, wins), (actions, wins)
    assert np.array_equal(np.argmax(policy, axis=1), wins)
    assert (visits.sum(axis=1) == 16).all()


# ----------------------------------------------------------------------------- 5. the improved policy is a distribution
@pytest.mark.parametrize("board,I,cons", [((3, 3, 3), 8, 4), ((4, 6, 3), 16, 8)])
def test_the_policy_sums_to_one_over_the_free_cells(board, I, cons):
    from puct_reuse_cases import exact_np

    m, n, k = board
    obs = random_positions(m, n, k, 12, np.random.default_rng(9), max_fill=0.9)
    obs[0] = 0
    actions, visits, _, policy, gscore = gumbel_puct(obs, k, I, 1.25, exact_np(m * n), cons, seed=3, step=1)
    occ = (obs.reshape(len(obs), 2, -1) != 0).any(axis=1)
    assert (policy[occ] == 0).all() and (policy >= 0).all()
    assert np.isneginf(gscore[occ]).all() and np.isfinite(gscore[~occ]).all()
    assert np.abs(policy.sum(axis=1) - 1.0).max() < 1e-6
    assert (visits[occ] == 0).all() and (visits.sum(axis=1) == I).all()
    assert (~occ[np.arange(len(obs)), actions]).all()
    # at most `cons` root cells are ever visited, and the move is one of the most visited
    assert ((visits > 0).sum(axis=1) <= cons).all()
    assert (visits[np.arange(len(obs)), actions] == visits.max(axis=1)).all()
    g = gumbel_scores(np.full((2, 9), 1 / 9, np.float32), np.ones((2, 9), bool), 1.0, seed=1)[1]
    assert np.isfinite(g).all()


def test_the_gpu_cases_hold_their_six_rows_on_every_board():
    """``positions`` of tests/test_gpu_puct_gumbel.py asserts its own rows (the empty board, a full one, one free cell,
    1 < F < considered, two rows with F > considered): on every case, the sibling boards included"""
    import test_gpu_puct_gumbel as gpu

    assert set(gpu.SIBLINGS) < set(gpu.CASES)
    for name, ((m, n, k), _, _) in gpu.CASES.items():
        obs = gpu.positions(name)
        assert obs.shape == (gpu.ROWS, 2, m, n)
        assert not has_run(obs[:, 0] != 0, k).any() and not has_run(obs[:, 1] != 0, k).any(), name
