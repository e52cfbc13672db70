"""GPU: the flat Monte Carlo player -- ``mnk_sample_playouts`` / ``MonteCarloPolicy.act`` bit for bit against the numpy
rule (tests/playout_rule.py) on built-in and generic boards, finished games included; launch-layout independence; the
device key words; N = 0 and full boards; the player as an opponent of ``TorchSelfPlayWrapper`` (eager and captured),
``validate_gpu`` and ``tournament.play_match``; the strength ladder Random < Tactical < MC(16) < MC(64) < MC(256)."""
import numpy as np
import pytest
import torch

from oracle import philox
from playout_rule import playout_moves
from tactical_rule import completions, random_positions

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OBS_DTYPES = (torch.float32, torch.bfloat16, torch.uint8)


@pytest.fixture(scope="module")
def hip():
    import __graft_entry__ as entry

    entry.build_hip()
    entry._ensure_path()
    import mnk_hip
    from alg.rollout_buffer import RolloutBuffer
    from env.torch_vector_mnk_env import TorchVectorMnkEnv
    from selfplay import graphed, policy, tournament, validation
    from selfplay.torch_self_play_wrapper import TorchSelfPlayWrapper

    mnk_hip.load()
    assert torch.cuda.is_available()

    class NS:
        pass

    ns = NS()
    ns.lib, ns.Env, ns.Wrapper, ns.policy, ns.graphed, ns.validation, ns.tournament = (
        mnk_hip, TorchVectorMnkEnv, TorchSelfPlayWrapper, policy, graphed, validation, tournament)
    ns.Buffer = RolloutBuffer
    return ns


def positions(m, n, k, count, seed):
    """random positions, a quarter of them finished games (a run already on the board), an empty and a full board"""
    rng = np.random.default_rng(seed)
    live = random_positions(m, n, k, count - count // 4, rng)
    done = random_positions(m, n, k, count // 4, rng, stop_at_win=False)
    obs = np.concatenate([live, done])
    obs[0] = 0
    obs[1] = 0
    obs[1, 0].reshape(-1)[::2] = 1
    obs[1, 1].reshape(-1)[1::2] = 1
    return obs


def act(hip, obs_np, k, P, seed, step=0, env_id0=0, dtype=torch.float32, deterministic=False):
    b, _, m, n = obs_np.shape
    pol = hip.policy.MonteCarloPolicy(k, P, seed=seed)
    pol._sampler.calls, pol._sampler.env_id0 = step, env_id0
    counts = torch.full((b, 2, m * n), -7, dtype=torch.int32, device=DEV)
    acts = pol.act({"observation": torch.from_numpy(obs_np).to(DEV).to(dtype)}, deterministic=deterministic, counts=counts)
    return acts.cpu().numpy(), counts.cpu().numpy()


# ----------------------------------------------------------------------------- 1. bit for bit against the rule
@pytest.mark.parametrize("board,rows,ps", [((3, 3, 3), 40, (1, 3, 16)), ((9, 9, 5), 12, (3, 8)), ((19, 19, 5), 4, (3,)),
                                           ((4, 4, 3), 24, (1, 5, 7)), ((7, 9, 7), 8, (3, 4))])
def test_counts_and_actions_equal_the_rule(hip, board, rows, ps):
    """(3x3x3, 9x9x5, 19x19x5: built-in variants; 4x4x3, 7x9x7: the generic NW forms)"""
    m, n, k = board
    obs = positions(m, n, k, rows, m * 100 + n * 10 + k)
    finished = [i for i in range(rows) if completions(obs[i:i + 1, 1], np.ones((1, m, n), bool), k).any()
                or completions(obs[i:i + 1, 0], np.ones((1, m, n), bool), k).any()]
    assert finished  # boards that already hold a run are in the comparison
    for P in ps:
        step, env_id0, seed = 3, 17, 1000 + P
        want_r, w, lo = playout_moves(obs, k, P, seed, step, env_id0)
        want_d, _, _ = playout_moves(obs, k, P, seed, step, env_id0, deterministic=True)
        want_counts = np.stack([w, lo], axis=1)
        for dtype in OBS_DTYPES:
            for det, want in ((False, want_r), (True, want_d)):
                got, counts = act(hip, obs, k, P, seed, step, env_id0, dtype, det)
                assert np.array_equal(counts, want_counts), (P, dtype, det)
                assert np.array_equal(got, want), (P, dtype, det)


def test_rows_do_not_depend_on_the_launch_layout(hip):
    """rows e.. of a batch keyed from env id 0 == the same rows launched alone with env_id0 = e"""
    m, n, k, P = 9, 9, 5, 24
    obs = positions(m, n, k, 40, 5)
    acts, counts = act(hip, obs, k, P, seed=9, step=2)
    for e, length in ((0, 1), (7, 5), (33, 7)):
        a, c = act(hip, obs[e:e + length], k, P, seed=9, step=2, env_id0=e)
        assert np.array_equal(a, acts[e:e + length]) and np.array_equal(c, counts[e:e + length])


def test_device_key_words_act_as_the_host_arguments(hip):
    """seed_dev REPLACES the key, step_dev is ADDED to the host step (what a captured graph re-keys through)"""
    m, n, k, P = 9, 9, 5, 8
    obs = torch.from_numpy(positions(m, n, k, 32, 6)).to(DEV)
    want_a, want_c = act(hip, obs.cpu().numpy(), k, P, seed=0x1234_5678_9ABC, step=11)
    pol = hip.policy.MonteCarloPolicy(k, P, seed=99)
    pol._sampler.seed_dev = torch.tensor([0x1234_5678_9ABC], dtype=torch.int64, device=DEV)
    pol._sampler.step_dev = torch.tensor([8], dtype=torch.int64, device=DEV)
    pol._sampler.calls = 3
    counts = torch.empty((32, 2, m * n), dtype=torch.int32, device=DEV)
    got = pol.act({"observation": obs}, counts=counts)
    assert np.array_equal(got.cpu().numpy(), want_a) and np.array_equal(counts.cpu().numpy(), want_c)
    assert pol._sampler.calls == 3  # the position lives in step_dev


def test_empty_batch_full_boards_and_shapes(hip):
    m, n, k = 3, 3, 3
    pol = hip.policy.MonteCarloPolicy(k, 4, seed=1)
    assert pol.act({"observation": torch.zeros((0, 2, m, n), device=DEV)}).shape == (0,)
    full = np.zeros((3, 2, m, n), np.float32)
    full[:, 0].reshape(3, -1)[:, ::2] = 1
    full[:, 1].reshape(3, -1)[:, 1::2] = 1
    got, counts = act(hip, full, k, 4, seed=1)
    x = philox.rand_u32(1, np.arange(3, dtype=np.uint64), 0, philox.STREAM_SAMPLE)
    assert np.array_equal(got, philox.mulhi32(x, m * n)) and not counts.any()  # a draw over all C cells, no playouts
    one = pol.act({"observation": torch.zeros((2, m, n), device=DEV)}, deterministic=True)  # a 3-D observation, call 1
    want = playout_moves(np.zeros((1, 2, m, n), np.float32), k, 4, seed=1, step=1, deterministic=True)[0]
    assert one.shape == (1,) and int(one[0]) == int(want[0])
    with pytest.raises(ValueError):
        pol.act({"observation": torch.zeros((2, 2, m, n), device=DEV)}, counts=torch.zeros((2, 2, 9), device=DEV))
    with pytest.raises(ValueError):
        pol.act({"observation": torch.zeros((2, 2, m, n), device=DEV)},
                counts=torch.zeros((2, 9), dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        hip.policy.MonteCarloPolicy(k, 0)
    with pytest.raises(ValueError):
        hip.policy.MonteCarloPolicy(k, 4097)


# ----------------------------------------------------------------------------- 2. as an opponent
def test_wrapper_opponent_plays_every_game_to_its_end(hip):
    """the generic pre -> act -> post path with the MC opponent (strict env: every reply is legal) plays every game to its
    end; validate_gpu against it"""
    m, n, k, nenv = 6, 6, 4, 64
    env = hip.Env(m, n, k, nenv, device=DEV, strict=True)
    w = hip.Wrapper(env, seed=3)
    opp = hip.policy.MonteCarloPolicy(k, 8, seed=4)
    w.set_opponent(opp)
    agent = hip.policy.RandomPolicy(m * n, seed=5)
    obs, _ = w.reset()
    ended = torch.zeros(nenv, dtype=torch.bool)
    for _ in range(m * n):
        obs, r, term, _, _ = w.step(agent.act(obs))
        assert w.last_opponent_actions.shape == (nenv,)
        ended |= term.cpu()
        if bool(ended.all()):
            break
    assert bool(ended.all()) and opp._sampler.calls > 0
    res = hip.validation.validate_gpu(hip.policy.RandomPolicy(m * n, seed=1), hip.policy.MonteCarloPolicy(k, 16, seed=2),
                                      (m, n, k), 256)
    key = "validation/vs_benchmark/"
    assert res[key + "games_played"] == 256
    assert res[key + "loss_rate"] > 0.6, res  # the random agent loses most games to MC(16)


def test_a_captured_rollout_plays_the_monte_carlo_opponent(hip):
    """``set_opponent(MonteCarloPolicy(...))`` on a captured wrapper: the graph is recaptured with the policy's act in
    it, keyed through the device words -- the rollouts equal the eager loop that switched at the same point"""
    m, n, k, nenv, steps = 6, 6, 4, 128, 5

    def eager(switch_after):
        w = hip.Wrapper(hip.Env(m, n, k, nenv, device=DEV), seed=8)
        w.set_opponent(hip.policy.RandomPolicy(m * n))
        buf = hip.Buffer(steps, nenv, (2, m, n), m * n, device=DEV)
        w.attach_sink(buf)
        sampler = hip.policy.HipSampler(seed=2)
        obs, _ = w.reset()
        out = []
        for r in range(3):
            if r == switch_after:
                w.set_opponent(hip.policy.MonteCarloPolicy(k, 6, seed=77))
            if r:
                buf.reset()
            for _ in range(steps):
                a, lp = sampler.draw(None, obs["action_mask"], False, want_logp=True)
                nxt, rew, term, _, _ = w.step(a)
                buf.add(obs["observation"], a, rew, torch.zeros(nenv, device=DEV), lp, term, obs["action_mask"])
                obs = nxt
            out.append((buf.observations[:steps].clone(), buf.rewards[:steps].clone(), buf.dones[:steps].clone()))
        return out

    want = eager(switch_after=1)
    w = hip.Wrapper(hip.Env(m, n, k, nenv, device=DEV), seed=8)
    w.set_opponent(hip.policy.RandomPolicy(m * n))
    buf = hip.Buffer(steps, nenv, (2, m, n), m * n, device=DEV)
    roll = hip.graphed.GraphedRollout(w, buf, None, seed=2)
    w.set_opponent(hip.policy.MonteCarloPolicy(k, 6, seed=77))
    assert roll._stale
    for r in range(3):
        if r:
            roll.run()
        got = (buf.observations[:steps], buf.rewards[:steps], buf.dones[:steps])
        assert all(torch.equal(a, b) for a, b in zip(got, want[r])), r
    assert not torch.equal(want[2][0], eager(switch_after=99)[2][0])  # the MC opponent did change the games


# ----------------------------------------------------------------------------- 3. the strength ladder
def _score(hip, p1, p2, board, games=1024):
    res = hip.tournament.play_match(p1, p2, board, games, device=DEV)
    assert res["wins"] + res["losses"] + res["draws"] == games
    return res["score"]


@pytest.mark.parametrize("board", [(9, 9, 5), (3, 3, 3)])
def test_strength_ordering(hip, board):
    """play_match scores of player 1 over 1024 games (half as black) with these seeds, as measured on the MI355X:
        9x9x5:  MC(64) vs Random 1.0000;  MC(64) vs Tactical 0.9697, Random vs Tactical 0.0068;  MC(256) vs MC(16) 0.9902
        3x3x3:  MC(64) vs Random 0.9526;  MC(64) vs Tactical 0.5688, Random vs Tactical 0.1147;  MC(256) vs MC(16) 0.6611
    The thresholds lie at least 5 standard errors below them: a score over 1024 games has a standard error of at most
    0.016 (5 SE: 0.08), a difference of two at most 0.022 (5 SE: 0.11)."""
    m, n, k = board
    pol = hip.policy
    mc64_random = _score(hip, pol.MonteCarloPolicy(k, 64, seed=1), pol.RandomPolicy(m * n, seed=2), board)
    mc64_tactical = _score(hip, pol.MonteCarloPolicy(k, 64, seed=3), pol.TacticalPolicy(k, seed=4), board)
    random_tactical = _score(hip, pol.RandomPolicy(m * n, seed=5), pol.TacticalPolicy(k, seed=6), board)
    mc256_mc16 = _score(hip, pol.MonteCarloPolicy(k, 256, seed=7), pol.MonteCarloPolicy(k, 16, seed=8), board)
    rates = (mc64_random, mc64_tactical, random_tactical, mc256_mc16)
    print(board, "MC64-Random %.4f MC64-Tactical %.4f Random-Tactical %.4f MC256-MC16 %.4f" % rates)
    vs_random, gap, mc256 = {(9, 9, 5): (0.9, 0.5, 0.9), (3, 3, 3): (0.85, 0.3, 0.5)}[board]
    assert mc64_random > vs_random, rates
    assert mc64_tactical > random_tactical + gap, rates  # MC(64) does better against Tactical than Random does
    assert mc256_mc16 > mc256, rates
