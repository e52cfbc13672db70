"""CPU: the PUCT search player -- the numpy restatement of the rule in tests/puct_rule.py on hand-built positions (a win
in one with an exact evaluator, terminal children backed up without evaluation, the visit total, full rows, the
temperature-1 draw); the C ABI of ``mnk_puct_workspace_bytes`` / ``mnk_puct_begin`` / ``mnk_puct_step`` (header, binding,
host argument checks, which reject before anything is enqueued); ``PUCTSearchPolicy``'s argument checks."""
import numpy as np
import pytest

from oracle import philox
from player_cases import board, check_header_and_binding, header_constants, lib  # noqa: F401 (lib: the fixture)
from puct_rule import puct


def uniform(leaf_obs, leaf_mask):
    """uniform priors over the legal cells, value 0"""
    cnt = np.maximum(leaf_mask.sum(axis=1, keepdims=True), 1)
    return (leaf_mask / cnt).astype(np.float32), np.zeros(len(leaf_mask), np.float32)


class Counting:
    """an evaluator that counts the rows it is asked about (terminal leaves included: the batch has a fixed shape)"""

    def __init__(self, inner=uniform):
        self.inner, self.calls, self.seen = inner, 0, []

    def __call__(self, leaf_obs, leaf_mask):
        self.calls += 1
        self.seen.append(leaf_obs)
        return self.inner(leaf_obs, leaf_mask)


# ----------------------------------------------------------------------------- the rule on hand-built positions
@pytest.mark.parametrize("rows,k,win", [
    (["xx..", "oo.o", "....", "...."], 3, 2),               # 4x4x3: (0, 2) wins now
    (["oo...", "xxxx.", "oo...", ".....", "....."], 5, 9),  # 5x5x5: (1, 4) completes five
])
def test_a_win_in_one_gets_the_visits(rows, k, win):
    """with uniform priors and value 0 (an exact evaluator of a position that is not yet decided) the winning child is a
    terminal with q = 1 on every visit; PUCT puts most of the visits there"""
    obs = board(rows)
    L = int(((obs[0, 0] == 0) & (obs[0, 1] == 0)).sum())
    for I in (4 * L, 8 * L):
        acts, visits, value = puct(obs, k, I, 1.25, uniform, seed=1, deterministic=True)
        assert acts[0] == win and visits[0, win] > I // 2, visits[0]
        assert value[0] > 0.4


def test_a_terminal_child_is_backed_up_without_evaluation():
    """the only legal cell wins: its child is terminal (v = -1 for its side to move) and is the leaf of every iteration;
    the evaluator is still called every time (a fixed batch) but only the roots' evaluation is used"""
    obs = board(["xx.", "oox", "xoo"])  # 3x3x3, x to move: (0, 2) completes the top row
    garbage = Counting(lambda o, msk: (np.full(msk.shape, 7.0, np.float32), np.full(len(msk), 0.25, np.float32)))
    acts, visits, value = puct(obs, 3, 6, 1.0, garbage)
    assert garbage.calls == 7 and acts[0] == 2 and visits[0, 2] == 6 and visits[0].sum() == 6
    # root w: -0.25 from evaluation 0, then -1 per visit of the win (from the view of the root's mover's opponent)
    assert value[0] == np.float32(6.25) / np.float32(7)


@pytest.mark.parametrize("I", [1, 7, 40, 100])
def test_root_visits_sum_to_I_and_zero_on_a_full_row(I):
    rng = np.random.default_rng(I)
    obs = np.zeros((4, 2, 4, 4), np.float32)
    obs[1, 0, 0, 0] = obs[1, 1, 3, 3] = 1
    obs[2, 0].reshape(-1)[rng.choice(16, 3, replace=False)] = 1
    obs[3, 0].reshape(-1)[::2] = 1
    obs[3, 1].reshape(-1)[1::2] = 1                           # full
    acts, visits, value = puct(obs, 3, I, 1.25, uniform, seed=3)
    assert (visits[:3].sum(axis=1) == I).all() and not visits[3].any()
    assert (visits[obs.reshape(4, 2, 16).any(axis=1)] == 0).all()  # 0 on occupied cells
    x = philox.rand_u32(3, np.arange(4, dtype=np.uint64), 0, philox.STREAM_SAMPLE)
    assert acts[3] == philox.mulhi32(x[3], 16)                 # a full row: a draw over all C cells
    assert value[3] == 0.0                                     # (its only backup: eval 0, value 0)


def test_a_full_row_shows_its_root_every_time():
    obs = board(["xox", "oxo", "oxo"])
    seen = []
    puct(obs, 3, 3, 1.0, uniform, leaves=seen)
    assert len(seen) == 4
    for lo, lm in seen:
        assert np.array_equal(lo, obs) and not lm.any()


def test_temperature_one_follows_the_cumulative_counts():
    obs = board(["x...", "....", "..o.", "...."])
    for seed in range(6):
        acts, visits, _ = puct(obs, 3, 50, 1.25, uniform, seed=seed, temperature=1)
        x = philox.rand_u32(seed, np.zeros(1, np.uint64), 0, philox.STREAM_SAMPLE)
        r = philox.mulhi32(x, int(visits[0].sum()))[0]
        cum = np.cumsum(visits[0])
        assert acts[0] == np.flatnonzero(cum > r)[0] and visits[0, acts[0]] > 0
        acts_d, visits_d, _ = puct(obs, 3, 50, 1.25, uniform, seed=seed, temperature=1, deterministic=True)
        assert np.array_equal(visits, visits_d)
        assert acts_d[0] == np.flatnonzero(visits[0] == visits[0].max())[0]


def test_leaves_are_canonical_views():
    """the first leaf is the row; a leaf one move deep shows the other side in channel 0"""
    obs = board(["x...", "....", "..o.", "...."])
    seen = []
    puct(obs, 3, 2, 1.0, uniform, leaves=seen)
    assert np.array_equal(seen[0][0], obs)
    lo, lm = seen[1]
    assert lo[0, 1, 0, 1] == 1 and lo[0, 1, 0, 0] == 1 and lo[0, 0, 2, 2] == 1  # x played (0, 1), first legal cell
    assert not lm[0, 1] and lm.sum() == 13


# ----------------------------------------------------------------------------- the C ABI
def test_header_declares_the_puct_entry_points_and_the_binding_matches(lib):
    check_header_and_binding(lib, "mnk_puct_begin")
    check_header_and_binding(lib, "mnk_puct_step")
    assert "mnk_puct_workspace_bytes" in lib.SIGNATURES and hasattr(lib.load(), "mnk_puct_workspace_bytes")
    assert header_constants()["MNK_PUCT_ITERS_MAX"] == "2048" == str(lib.PUCT_ITERS_MAX)


def test_workspace_bytes(lib):
    one = lib.puct_workspace_bytes(1, 9, 9, 256)
    assert one % 256 == 0 and 257 * 6 * 81 <= one <= 257 * 6 * 81 + 257 * 16 + 1024
    assert lib.puct_workspace_bytes(1024, 9, 9, 256) == 1024 * one
    assert lib.puct_workspace_bytes(0, 9, 9, 256) == 0
    for bad in ((-1, 9, 9, 256), (4, 9, 9, 0), (4, 9, 9, 2049), (4, 40, 40, 8), (4, 4, 1, 8)):
        with pytest.raises(lib.MnkHipError):
            lib.puct_workspace_bytes(*bad)


def test_host_rejects_bad_arguments_and_enqueues_nothing(lib):
    """every host check raises MnkHipError (the fake device pointers are never dereferenced: nothing is launched when a
    check fails, and N = 0 launches nothing either)"""
    p = 0x1000  # a non-NULL pointer that must never be touched

    def begin(obs=p, dtype=0, N=8, m=9, n=9, k=5, I=256, ws=p, lo=p, ldt=0, lm=p):
        return lib.call("mnk_puct_begin", obs, dtype, N, m, n, k, I, ws, lo, ldt, lm, None)

    def step(ws=p, N=8, m=9, n=9, k=5, I=256, pr=p, pdt=0, va=p, vdt=0, c=1.25, last=0, temp=0, lo=p, ldt=0, lm=p,
             acts=p):
        return lib.call("mnk_puct_step", ws, N, m, n, k, I, pr, pdt, va, vdt, c, last, temp, 1, None, 0, None, 0, 0,
                        lo, ldt, lm, acts, None, None, None)

    for bad in (dict(obs=None), dict(ws=None), dict(lo=None), dict(lm=None), dict(N=-1), dict(dtype=3), dict(ldt=-1),
                dict(I=0), dict(I=2049), dict(k=10), dict(m=40, n=40)):
        with pytest.raises(lib.MnkHipError, match="mnk_puct_begin"):
            begin(**bad)
    for bad in (dict(ws=None), dict(pr=None), dict(va=None), dict(N=-1), dict(pdt=2), dict(vdt=-1), dict(I=0),
                dict(I=2049), dict(c=-0.5), dict(c=float("nan")), dict(c=float("inf")), dict(temp=2), dict(temp=-1),
                dict(last=2), dict(lo=None), dict(lm=None), dict(ldt=3), dict(last=1, acts=None), dict(n=1, m=4, k=1)):
        with pytest.raises(lib.MnkHipError, match="mnk_puct_step"):
            step(**bad)
    assert begin(N=0) == 0 and step(N=0) == 0 and step(N=0, last=1, lo=None, lm=None, ldt=9) == 0
    assert step(N=0, I=2048, c=0.0, temp=1, pdt=1, vdt=1) == 0


def test_puct_policy_validates_its_arguments(lib):
    import torch

    from selfplay.policy import Policy, PUCTSearchPolicy

    ev = lambda o, msk: (msk.float(), torch.zeros(len(msk)))  # noqa: E731
    pol = PUCTSearchPolicy(5, evaluator=ev)
    assert (pol.iterations, pol.c, pol.temperature, pol.leaf_dtype) == (256, 1.25, 0, torch.float32)
    assert isinstance(pol, Policy)
    assert not getattr(pol, "fused_uniform_random", False) and not getattr(pol, "fused_tactical", False)
    assert not getattr(pol, "fused_logits", False)
    for bad in (dict(iterations=0), dict(iterations=2049), dict(c=-1.0), dict(c=float("nan")), dict(c=float("inf")),
                dict(temperature=2), dict(temperature=0.5)):
        with pytest.raises(ValueError):
            PUCTSearchPolicy(5, evaluator=ev, **bad)
    with pytest.raises(TypeError):
        PUCTSearchPolicy(5, evaluator=ev, leaf_dtype=torch.float16)
    with pytest.raises(ValueError):
        PUCTSearchPolicy(5)                                       # neither a model nor an evaluator
    with pytest.raises(ValueError):
        PUCTSearchPolicy(5, model=torch.nn.Identity(), evaluator=ev)  # both
    PUCTSearchPolicy(5, evaluator=ev, iterations=2048, c=0.0, temperature=1, leaf_dtype=torch.uint8)
    pol = PUCTSearchPolicy(3, evaluator=ev, iterations=4)
    with pytest.raises((ValueError, RuntimeError)):             # a CPU observation is refused before anything else
        pol.act({"observation": torch.zeros((2, 2, 3, 3))})
