"""CPU: the tree-search player -- the numpy restatement of the rule in tests/search_rule.py on hand-built positions (wins
in one, a forced block, the visit total, finished and full rows); the C ABI of ``mnk_sample_search`` (header, binding,
host argument checks, which reject before anything is enqueued); ``SearchPolicy``'s argument checks."""
import numpy as np
import pytest

from oracle import philox
from player_cases import board, check_header_and_binding, header_constants, lib  # noqa: F401 (lib: the fixture)
from search_rule import STREAM_SEARCH, search


def legal_count(obs):
    return int(((obs[:, 0] == 0) & (obs[:, 1] == 0)).sum())


# ----------------------------------------------------------------------------- the rule on hand-built positions
@pytest.mark.parametrize("rows,k,win", [
    (["xx..", "oo.o", "....", "...."], 3, 2),        # 4x4x3: (0, 2) wins now; o wins at (1, 2) otherwise
    (["oo...", "xxxx.", "oo...", ".....", "....."], 5, 9),  # 5x5x5: (1, 4) completes five
])
def test_a_win_in_one_is_played_with_enough_iterations(rows, k, win):
    """with I >= |L| the winning cell is a terminal child with W = n (q = 1, the best any child can have).  The rule does
    not promise more than that -- a child whose playouts all win ties with it in q (e.g. a double threat on 3x3x3) -- but
    where the other cells lose playouts the search puts most visits on the win by I = 4 |L|"""
    obs = board(rows)
    L = legal_count(obs)
    for seed in range(3):
        for I in (L, 4 * L, 8 * L):
            acts, stats = search(obs, k, I, 4, 1.0, seed=seed, step=seed)
            assert stats[0, 1, win] == stats[0, 0, win] > 0 and stats[0, 2, win] == 0  # a terminal win: W = n
            if I > L:
                assert acts[0] == win, (seed, I, stats[0, 0])
    # with I < |L| the winning cell is never expanded (expansion goes in action order): the guarantee needs I >= |L|
    free = np.flatnonzero((obs[0, 0] == 0).reshape(-1) & (obs[0, 1] == 0).reshape(-1))
    rank = int(np.flatnonzero(free == win)[0])
    acts, stats = search(obs, k, rank, 4, 1.0, seed=0)
    assert stats[0, 0, win] == 0 and acts[0] != win


def test_a_single_threat_is_blocked_on_3x3x3():
    obs = board(["o..", ".o.", "x.."])               # o threatens (2, 2); x has no win in one
    for seed in range(3):
        acts, stats = search(obs, 3, 256, 16, 1.0, seed=seed, step=seed)
        assert acts[0] == 8, stats[0, 0]


@pytest.mark.parametrize("I,B", [(1, 1), (7, 3), (40, 5), (100, 2)])
def test_root_visits_sum_to_I_times_B(I, B):
    rng = np.random.default_rng(I)
    obs = np.zeros((3, 2, 4, 4), np.float32)
    obs[1, 0, 0, 0] = obs[1, 1, 3, 3] = 1
    obs[2, 0].reshape(-1)[rng.choice(16, 3, replace=False)] = 1
    _, stats = search(obs, 3, I, B, 1.0, seed=3)
    assert (stats[:, 0].sum(axis=1) == I * B).all()
    assert (stats[:, 1] + stats[:, 2] <= stats[:, 0]).all()
    assert (stats[:, 0][obs.reshape(3, 2, 16).any(axis=1)] == 0).all()  # 0 on occupied cells
    expanded = (stats[:, 0] > 0).sum(axis=1)
    assert (expanded == np.minimum(I, 16 - obs.reshape(3, -1).sum(1))).all()  # one root child per iteration first


def test_full_and_finished_rows():
    full = board(["xox", "oxo", "oxo"])
    acts, stats = search(full, 3, 8, 4, 1.0, seed=1)
    x = philox.rand_u32(1, np.zeros(1, np.uint64), 0, philox.STREAM_SAMPLE)
    assert acts[0] == philox.mulhi32(x, 9)[0] and not stats.any()  # a draw over all C cells, no iterations
    assert search(full, 3, 8, 4, 1.0, seed=1, deterministic=True)[0][0] == 0
    # o already has a run: every child is lost at o's first reply, except x's own completion, which is a terminal win
    done = board(["ooo.", "x...", "x...", "...."])
    acts, stats = search(done, 3, 60, 4, 1.0, seed=2, deterministic=True)
    legal = ((done[0, 0] == 0) & (done[0, 1] == 0)).reshape(-1)
    assert acts[0] == 12 and stats[0, 1, 12] == stats[0, 0, 12]
    others = legal.copy()
    others[12] = False
    assert (stats[0, 1][others] == 0).all() and (stats[0, 2][others] == stats[0, 0][others]).all()


def test_counter_layout_and_stream():
    """one iteration from an empty 4x4 board: the first cell is expanded and playout j's ply t draws its u32 at
    u = (((step * I + 0) * B + j) * C4) + t on stream SEARCH (5)"""
    assert STREAM_SEARCH == 5
    obs = np.zeros((1, 2, 4, 4), np.float32)
    I, B, step = 1, 2, 5
    _, stats = search(obs, 1, I, B, 1.0, seed=9, step=step, env_id0=3)  # k = 1: the expanded child wins at once
    assert stats[0, 0, 0] == B and stats[0, 1, 0] == B and stats[0, 0, 1:].sum() == 0
    # k = 4: the reply of playout 1 is pick_legal over the 15 free cells with u = ((step * 1) * 2 + 1) * 16
    u = ((step * I) * B + 1) * 16
    x = philox.rand_u32(9, np.array([3], np.uint64), np.uint64(u), STREAM_SEARCH)
    free = np.ones((1, 16), bool)
    free[0, 0] = False
    assert philox.pick_legal(free, x)[0] != 0


def test_deterministic_and_sampled_pick_from_the_most_visited():
    obs = board(["x...", "....", "..o.", "...."])
    acts_d, stats = search(obs, 3, 64, 4, 1.0, seed=4, deterministic=True)
    s = stats[0, 0] == stats[0, 0].max()
    assert acts_d[0] == np.flatnonzero(s)[0]
    acts_r, stats_r = search(obs, 3, 64, 4, 1.0, seed=4)
    assert np.array_equal(stats, stats_r)
    x = philox.rand_u32(4, np.zeros(1, np.uint64), 0, philox.STREAM_SAMPLE)
    assert acts_r[0] == philox.pick_legal(s[None], x)[0]


# ----------------------------------------------------------------------------- the C ABI
def test_header_declares_mnk_sample_search_and_the_binding_matches(lib):
    check_header_and_binding(lib, "mnk_sample_search")
    consts = header_constants()
    assert consts["MNK_STREAM_SEARCH"] == "5" == str(lib.STREAM_SEARCH)
    assert consts["MNK_SEARCH_ITERS_MAX"] == "2048" == str(lib.SEARCH_ITERS_MAX)
    assert consts["MNK_SEARCH_PLAYOUTS_MAX"] == "256" == str(lib.SEARCH_PLAYOUTS_MAX)


def test_host_rejects_bad_arguments_and_enqueues_nothing(lib):
    """every host check raises MnkHipError (the fake device pointers are never dereferenced: nothing is launched when a
    check fails, and N = 0 launches nothing either)"""
    p = 0x1000  # a non-NULL pointer that must never be touched

    def sample(obs=p, dtype=0, N=8, m=9, n=9, k=5, I=256, B=32, c=1.0, step=0, acts=p):
        return lib.call("mnk_sample_search", obs, dtype, N, m, n, k, I, B, c, 1, None, step, None, 0, 0, acts, None,
                        None)

    for bad in (dict(obs=None), dict(acts=None), dict(N=-1), dict(dtype=3), dict(dtype=-1), dict(I=0), dict(I=-1),
                dict(I=2049), dict(B=0), dict(B=257), dict(c=-0.5), dict(c=float("nan")), dict(c=float("inf"))):
        with pytest.raises(lib.MnkHipError, match="mnk_sample_search"):
            sample(**bad)
    # the counter range: q = u >> 2 < 2^56, i.e. (step + 1) * I * B * C4 <= 2^58
    per_step = 256 * 32 * 84
    with pytest.raises(lib.MnkHipError):
        sample(step=(1 << 58) // per_step)
    with pytest.raises(lib.MnkHipError):
        sample(step=(1 << 64) - 1)
    with pytest.raises(lib.MnkHipError):
        sample(m=3, n=3, k=3, I=2048, B=256, step=(1 << 58) // (2048 * 256 * 12))
    for geom in (dict(k=10), dict(m=40, n=40), dict(n=1, m=4, k=1)):
        with pytest.raises(lib.MnkHipError, match="geometry|status -2"):
            sample(**geom)
    assert sample(N=0) == 0
    assert sample(N=0, step=(1 << 58) // per_step - 1) == 0
    assert sample(N=0, I=2048, B=256, c=0.0) == 0


def test_search_policy_validates_its_arguments(lib):
    from selfplay.policy import Policy, SearchPolicy

    pol = SearchPolicy(5)
    assert (pol.iterations, pol.playouts, pol.c) == (256, 32, 0.05) and isinstance(pol, Policy)
    assert not getattr(pol, "fused_uniform_random", False) and not getattr(pol, "fused_tactical", False)
    assert not getattr(pol, "fused_logits", False)
    for bad in (dict(iterations=0), dict(iterations=2049), dict(playouts=0), dict(playouts=257), dict(c=-1.0),
                dict(c=float("nan")), dict(c=float("inf"))):
        with pytest.raises(ValueError):
            SearchPolicy(5, **bad)
    SearchPolicy(5, iterations=2048, playouts=256, c=0.0)


def test_search_policy_checks_its_stats_tensor(lib):
    import torch

    from selfplay.policy import SearchPolicy

    pol = SearchPolicy(3, iterations=4, playouts=2)
    obs = {"observation": torch.zeros((2, 2, 3, 3))}
    with pytest.raises((ValueError, RuntimeError)):  # a CPU observation is refused before anything else
        pol.act(obs)
    if torch.cuda.is_available():
        obs = {"observation": torch.zeros((2, 2, 3, 3), device="cuda:0")}
        for bad in (torch.zeros((2, 3, 9), dtype=torch.int32), torch.zeros((2, 2, 9), dtype=torch.int32, device="cuda:0"),
                    torch.zeros((2, 3, 9), device="cuda:0"), torch.zeros((2, 9, 3), dtype=torch.int32,
                                                                         device="cuda:0").transpose(1, 2)):
            with pytest.raises(ValueError):
                pol.act(obs, stats=bad)
