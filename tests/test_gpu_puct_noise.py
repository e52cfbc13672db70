"""GPU: the PUCT player's built-in Dirichlet root noise -- ``mnk_puct_root_noise`` against the numpy rule
(tests/puct_noise_rule.py) under, at, over and far over one pass of the wave, both prior dtypes, several leaves, device key
words; its moments; eps = 0; ``PUCTSearchPolicy(root_noise=...)`` bit for bit against the search rules fed with the
kernel's own noised root priors (fresh, several leaves, a kept tree); determinism and sharding; a captured
``SearchSelfPlay`` ply and a ``state_dict`` round trip with noise; refusals; the example's loop with ``noise="builtin"``.

The kernel's eta is the float32 of a float64 that agrees with numpy's to about 1e-13 (a few ulps of log / exp / cos), so
rtol 1e-6 leaves some 16 float32 ulps over the half ulp of the conversion; the mix adds three correctly rounded float32
operations on non-negative terms.  An accept / reject comparison that differs between the device's and numpy's logarithm
within an ulp would show as a gross mismatch (probability about 1e-12 per cell): the answer then is another seed."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import puct_noise_rule as rule
from player_cases import DEV, check_header_and_binding, hip  # noqa: F401 (hip: the fixture)
from puct_leaves_rule import LeavesPuct, puct_leaves
from puct_reuse_rule import ReusePuct
from puct_rule import puct
from test_gpu_puct_reuse import advance, exact_np, exact_torch, gpu_act, same, start
from test_gpu_search_selfplay import RANDOM_MIN, TACTICAL_LOSS_MAX, TACTICAL_MIN
from test_gpu_search_selfplay import exact_torch as selfplay_evaluator
from test_gpu_search_selfplay import same as same_selfplay

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_PUCT, SEED, ENV_ID0 = 1.25, 47, 3
SENTINEL = -7.0


def noise(lib, priors, mask, N, C, L, alpha, eps, seed=SEED, step=0, env_id0=ENV_ID0, step_dev=None, out=None):
    """one call of the entry point on torch tensors [N * L, C]; returns ``out`` (made of sentinels when not given)"""
    if out is None:
        out = torch.full((N * L, C), SENTINEL, dtype=torch.float32, device=DEV)
    code = lib.LOGITS_BF16 if priors.dtype == torch.bfloat16 else lib.LOGITS_F32
    lib.call("mnk_puct_root_noise", lib.ptr(priors), code, lib.ptr(mask), N, C, L, alpha, eps, seed, None, step,
             lib.ptr(step_dev), env_id0, lib.ptr(out), lib.stream_ptr(DEV))
    return out


def inputs(N, C, L, dtype, seed):
    """priors in (0, 1] of ``dtype`` and a random mask [N * L, C] whose root rows include a full board (row 1: no free
    cell) and a row with one free cell (row 2); the float32 view of the priors"""
    rng = np.random.default_rng(seed)
    priors = torch.from_numpy((1.0 - rng.random((N * L, C))).astype(np.float32)).to(dtype)
    mask = rng.random((N * L, C)) < 0.6
    mask[1 * L] = False
    mask[2 * L] = False
    mask[2 * L, C // 2] = True
    return priors.to(DEV), torch.from_numpy(mask).to(DEV), priors.float().numpy(), mask


# ----------------------------------------------------------------------------- 1. header and binding
def test_header_and_binding_agree(hip):
    check_header_and_binding(hip.lib, "mnk_puct_root_noise")
    assert hip.lib.STREAM_NOISE == rule.STREAM_NOISE == 7 and hip.lib.PUCT_NOISE_TRIES == rule.TRIES == 16
    text = open(os.path.join(ROOT, "include", "mnk_hip.h")).read()
    assert "#define MNK_STREAM_NOISE 7" in text and "#define MNK_PUCT_NOISE_TRIES 16" in text


# ----------------------------------------------------------------------------- 2. the kernel against the rule
@pytest.mark.parametrize("N,L,dtype,through_dev", [(5, 1, torch.float32, False), (7, 4, torch.bfloat16, True),
                                                   (5, 4, torch.float32, True), (7, 1, torch.bfloat16, False)])
@pytest.mark.parametrize("C,alpha", [(9, 0.3), (24, 0.3), (81, 0.3), (361, 0.03), (63, 0.3), (240, 0.1), (342, 0.03),
                                     (289, 0.03), (625, 0.03)])  # (17x17 and 25x25: five and ten trips, odd row sizes)
def test_the_kernel_equals_the_rule(hip, C, alpha, N, L, dtype, through_dev):
    lib = hip.lib
    step = 6
    priors, mask, priors_np, mask_np = inputs(N, C, L, dtype, C + N)
    kept = priors.clone()
    step_dev = torch.tensor([step - 2], dtype=torch.int64, device=DEV) if through_dev else None
    eta = rule.eta(mask_np[::L], alpha, SEED, step, ENV_ID0)
    roots, free = priors_np[::L], mask_np[::L]
    assert not free[1].any() and free[2].sum() == 1 and free[0].sum() > 1
    for eps in (1.0, 0.25):
        out = noise(lib, priors, mask, N, C, L, alpha, eps, step=2 if through_dev else step, step_dev=step_dev)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        want = rule.mix(roots, free, eta, eps)
        some = free & (want > 0)  # (at alpha = 0.03 the smallest eta are 0 as float32, in the rule and on the device)
        err = np.abs(got[::L][some] / want[some] - 1).max()
        print(f"C {C} N {N} L {L} eps {eps}: largest relative deviation {err:.3g}")
        np.testing.assert_allclose(got[::L][free], want[free], rtol=1e-6, atol=0)
        if eps == 1.0:
            np.testing.assert_allclose(got[::L][free], eta.astype(np.float32)[free], rtol=1e-6, atol=0)
            assert got[2 * L, C // 2] == 1.0
        # off the mask and on a full board: the widened priors bit for bit; other rows: untouched; priors: unchanged
        assert np.array_equal(got[::L][~free].view(np.uint32), roots[~free].view(np.uint32))
        assert np.array_equal(got[1 * L].view(np.uint32), roots[1].view(np.uint32))
        others = np.ones(N * L, bool)
        others[::L] = False
        assert (got[others] == SENTINEL).all()
        assert torch.equal(priors, kept)


# ----------------------------------------------------------------------------- 3. moments
def test_moments_on_the_device_are_dirichlets(hip):
    rows, C, alpha = 4096, 9, 0.3
    priors = torch.zeros((rows, C), device=DEV)
    mask = torch.ones((rows, C), dtype=torch.bool, device=DEV)
    out = noise(hip.lib, priors, mask, rows, C, 1, alpha, 1.0, seed=11, step=3, env_id0=0)
    got = out.cpu().numpy()
    np.testing.assert_allclose(got.sum(axis=1), 1.0, rtol=0, atol=1e-6)
    rule.check_moments(got, C, float(np.float32(alpha)))


# ----------------------------------------------------------------------------- 4. eps = 0
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_eps_zero_copies_the_priors(hip, dtype):
    N, C, L = 6, 81, 2
    priors, mask, priors_np, _ = inputs(N, C, L, dtype, 5)
    got = noise(hip.lib, priors, mask, N, C, L, 0.3, 0.0).cpu().numpy()
    assert np.array_equal(got[::L].view(np.uint32), priors_np[::L].view(np.uint32))


def make_policy(hip, k, I, C, L, temperature, step, root_noise, **kw):
    pol = hip.policy.PUCTSearchPolicy(k, evaluator=exact_torch(C), iterations=I, c=C_PUCT, seed=SEED, leaves=L,
                                      temperature=temperature, root_noise=root_noise, **kw)
    pol._sampler.env_id0, pol._sampler.calls = ENV_ID0, step
    return pol


@pytest.mark.parametrize("L", [1, 4])
@pytest.mark.parametrize("board,I", [((3, 3, 3), 16), ((9, 9, 5), 8)])
def test_a_search_with_eps_zero_equals_the_search_without_noise(hip, board, I, L):
    m, n, k = board
    obs = start(m, n, k, 5, 17)
    plain = make_policy(hip, k, I, m * n, L, 0, 2, None)
    zero = make_policy(hip, k, I, m * n, L, 0, 2, (0.3, 0.0))
    assert plain.root_noise is None and plain._buffers(5, m, n, torch.device(DEV))[3] is None
    same(gpu_act(zero, obs), gpu_act(plain, obs), (board, L))
    assert zero._bufs[4].shape == (5 * L, m * n) and zero._bufs[4].dtype == torch.float32


# ----------------------------------------------------------------------------- 5. the noisy search against the rule
def noised_roots(hip, obs, C, L, alpha, eps, step):
    """what mnk_puct_root_noise makes of the exact evaluator's priors on the roots ``obs``: float32 [N, C]"""
    N = len(obs)
    free = (obs[:, 0] + obs[:, 1]).reshape(N, C) == 0
    priors, _ = exact_np(C)(obs.astype(np.float32), free)
    priors = torch.from_numpy(np.repeat(priors.astype(np.float32), L, axis=0)).to(DEV)
    mask = torch.from_numpy(np.repeat(free, L, axis=0)).to(DEV)
    return noise(hip.lib, priors, mask, N, C, L, alpha, eps, step=step).cpu().numpy()[::L]


@pytest.mark.parametrize("L", [1, 4])
@pytest.mark.parametrize("temperature", [0, 1])
@pytest.mark.parametrize("board,I", [((3, 3, 3), 16), ((9, 9, 5), 8)])
def test_a_noisy_act_equals_the_rule_on_the_kernels_priors(hip, board, I, temperature, L):
    m, n, k = board
    C, N, step, alpha, eps = m * n, 5, 3, 0.3, 0.25
    obs = start(m, n, k, N, 29)
    rows = noised_roots(hip, obs, C, L, alpha, eps, step)
    assert not np.array_equal(rows, noised_roots(hip, obs, C, L, alpha, 0.0, step))
    ev = rule.noisy_roots(exact_np(C), I // L + 1, lambda act: rows)
    if L == 1:
        want = puct(obs, k, I, C_PUCT, ev, seed=SEED, step=step, env_id0=ENV_ID0, temperature=temperature)
    else:
        want = puct_leaves(obs, k, I, C_PUCT, ev, L, seed=SEED, step=step, env_id0=ENV_ID0, temperature=temperature)
    got = gpu_act(make_policy(hip, k, I, C, L, temperature, step, (alpha, eps)), obs)
    same(got, want + (np.zeros((N, 2), np.int32),), (board, temperature, L))


@pytest.mark.parametrize("L", [1, 4])
@pytest.mark.parametrize("temperature", [0, 1])
@pytest.mark.parametrize("board,I", [((3, 3, 3), 16), ((9, 9, 5), 8)])
def test_two_noisy_acts_with_a_kept_tree_equal_the_rule(hip, board, I, temperature, L):
    """a carried root takes fresh root priors every act, and so fresh noise"""
    m, n, k = board
    C, N, step, alpha, eps = m * n, 5, 3, 0.3, 0.25
    rows = {}
    ev = rule.noisy_roots(exact_np(C), I // L + 1, lambda act: rows[act])
    if L == 1:
        search = ReusePuct(k, I, C_PUCT, ev, seed=SEED, env_id0=ENV_ID0, temperature=temperature)
    else:
        search = LeavesPuct(k, I, C_PUCT, ev, L, reuse=True, seed=SEED, env_id0=ENV_ID0, temperature=temperature)
    pol = make_policy(hip, k, I, C, L, temperature, step, (alpha, eps), reuse=True)
    obs = start(m, n, k, N, 31)
    resets, carried = np.zeros(N, np.int64), 0
    for act in range(2):
        rows[act] = noised_roots(hip, obs, C, L, alpha, eps, step + act)
        want = search.act(obs, step=step + act)
        same(gpu_act(pol, obs), want, (board, temperature, L, act))
        carried += int((want[3][:, 0] > 1).sum()) if act else 0
        obs = advance(obs, want[0], k, 1, resets)
    assert carried and not np.array_equal(rows[0], rows[1])


# ----------------------------------------------------------------------------- 6. determinism
def test_the_noise_is_a_function_of_seed_step_and_row_id(hip):
    N, C = 8, 81
    priors, mask, _, _ = inputs(N, C, 1, torch.float32, 9)
    a = noise(hip.lib, priors, mask, N, C, 1, 0.3, 0.25, step=5, env_id0=0)
    b = noise(hip.lib, priors, mask, N, C, 1, 0.3, 0.25, step=5, env_id0=0)
    other = noise(hip.lib, priors, mask, N, C, 1, 0.3, 0.25, step=6, env_id0=0)
    lo = noise(hip.lib, priors[:4].contiguous(), mask[:4].contiguous(), 4, C, 1, 0.3, 0.25, step=5, env_id0=0)
    hi = noise(hip.lib, priors[4:].contiguous(), mask[4:].contiguous(), 4, C, 1, 0.3, 0.25, step=5, env_id0=4)
    assert torch.equal(a, b) and not torch.equal(a, other)
    assert torch.equal(a, torch.cat([lo, hi]))


# ----------------------------------------------------------------------------- 7. search self-play
NOISE = (0.3, 0.25)


def new_selfplay(hip, seed=5, root_noise=NOISE, **kw):
    from selfplay.search_selfplay import SearchSelfPlay

    return SearchSelfPlay(3, 3, 3, 8, evaluator=selfplay_evaluator(9), seed=seed, iterations=8, temp_plies=2, capacity=12,
                          root_noise=root_noise, **kw)


def test_a_captured_noisy_ply_replayed_equals_eager_plies(hip):
    P = 23
    eager = new_selfplay(hip)
    eager.play(1 + P)
    sp = new_selfplay(hip)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        sp.play(1)  # the buffers
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sp.play(1)
    sp.buffer.plies_host -= 1  # (the capture itself ran nothing)
    for _ in range(P):
        graph.replay()
    sp.note_replayed(P)
    torch.cuda.synchronize()
    same_selfplay(sp, eager)
    assert eager.pop_game_stats()["games"] > 0
    plain = new_selfplay(hip, root_noise=None)
    plain.play(1 + P)
    assert not torch.equal(plain.buffer.visits, eager.buffer.visits)  # (the noise reached the searches)


def test_a_noisy_state_dict_round_trip_continues_bit_exactly(hip):
    a = new_selfplay(hip, seed=9, reuse=False)
    a.play(7)
    state = a.state_dict()
    a.play(11)
    b = new_selfplay(hip, seed=1, reuse=False)
    b.load_state_dict(state)
    b.play(11)
    same_selfplay(a, b)
    sa, sb = a.pop_game_stats(), b.pop_game_stats()
    assert sa == sb and sa["games"] > 0


# ----------------------------------------------------------------------------- 8. refusals
def test_bad_arguments_are_refused_before_anything_is_enqueued(hip):
    lib = hip.lib
    N, C, L = 4, 9, 2
    priors, mask, _, _ = inputs(N, C, L, torch.float32, 1)
    out = torch.full((N * L, C), SENTINEL, device=DEV)
    nan, inf = float("nan"), float("inf")
    good = dict(priors=priors, mask=mask, C=C, L=L, alpha=0.3, eps=0.25, code=lib.LOGITS_F32, out=out)
    bad = [dict(alpha=0.0), dict(alpha=-1.0), dict(alpha=nan), dict(alpha=inf), dict(eps=-0.1), dict(eps=1.5),
           dict(eps=nan), dict(L=0), dict(L=lib.PUCT_LEAVES_MAX + 1), dict(C=0), dict(C=1025), dict(code=2),
           dict(priors=None), dict(mask=None), dict(out=None)]
    for change in bad:
        a = dict(good, **change)
        with pytest.raises(lib.MnkHipError, match="invalid argument"):
            lib.call("mnk_puct_root_noise", lib.ptr(a["priors"]), a["code"], lib.ptr(a["mask"]), N, a["C"], a["L"],
                     a["alpha"], a["eps"], SEED, None, 0, None, 0, lib.ptr(a["out"]), lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()


@pytest.mark.parametrize("root_noise", [(0.3,), (0.3, 0.25, 1), "ab", 0.3, (0.0, 0.25), (-0.3, 0.25), (float("nan"), 0.25),
                                        (float("inf"), 0.25), (1e-60, 0.25), (0.3, -0.01), (0.3, 1.01), (0.3, float("nan")),
                                        ("x", 0.25)])
def test_the_policy_refuses_a_malformed_root_noise(hip, root_noise):
    with pytest.raises(ValueError, match="root_noise"):
        hip.policy.PUCTSearchPolicy(3, evaluator=exact_torch(9), iterations=8, root_noise=root_noise)
    from selfplay.search_selfplay import SearchSelfPlay

    with pytest.raises(ValueError, match="root_noise"):
        SearchSelfPlay(3, 3, 3, 4, evaluator=exact_torch(9), iterations=8, root_noise=root_noise)


# ----------------------------------------------------------------------------- 9. the example
def test_the_alphazero_loop_learns_tic_tac_toe_with_builtin_noise(hip):
    """the existing loop's bounds (tests/test_gpu_search_selfplay.py): the greedy net over 1 024 games scores at least
    0.8 against RandomPolicy and 0.6 against TacticalPolicy with at most 10 % losses"""
    path = os.path.join(ROOT, "examples", "alphazero_selfplay.py")
    spec = importlib.util.spec_from_file_location("alphazero_selfplay", path)
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    net = ex.train(3, 3, 3, envs=256, iterations=32, rounds=12, updates=40, seed=0, noise="builtin", log=print)
    res = ex.validate(net, 3, 3, 3, episodes=1024)
    print(res)
    assert res["random"]["score_rate"] >= RANDOM_MIN
    assert res["tactical"]["score_rate"] >= TACTICAL_MIN and res["tactical"]["loss_rate"] <= TACTICAL_LOSS_MAX
    with pytest.raises(ValueError, match="noise"):
        ex.train(3, 3, 3, rounds=0, noise="dirichlet")
