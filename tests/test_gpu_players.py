"""GPU: what the Monte Carlo player (``MonteCarloPolicy``, ``mnk_sample_playouts``) and the tree-search player
(``SearchPolicy``, ``mnk_sample_search``) promise alike -- launch-layout independence; the device key words; N = 0, full
boards and shapes; the player as an opponent of ``TorchSelfPlayWrapper`` (eager and captured) and of ``validate_gpu``.
Each player's rule and strength ladder: test_gpu_playout.py, test_gpu_search.py."""
import numpy as np
import pytest
import torch

from oracle import philox
from player_cases import DEV, MC, SEARCH, hip, positions  # noqa: F401 (hip: the fixture)

pytestmark = pytest.mark.gpu
PLAYERS = pytest.mark.parametrize("player", [MC, SEARCH], ids=["mc", "search"])


@PLAYERS
def test_rows_do_not_depend_on_the_launch_layout(hip, player):
    """rows e.. of a batch keyed from env id 0 == the same rows launched alone with env_id0 = e"""
    m, n, k = 9, 9, 5
    obs = positions(m, n, k, 40, 5)
    acts, out = player.act(hip, obs, k, player.layout, seed=9, step=2)
    for e, length in ((0, 1), (7, 5), (33, 7)):
        a, o = player.act(hip, obs[e:e + length], k, player.layout, seed=9, step=2, env_id0=e)
        assert np.array_equal(a, acts[e:e + length]) and np.array_equal(o, out[e:e + length])


@PLAYERS
def test_device_key_words_act_as_the_host_arguments(hip, player):
    """seed_dev REPLACES the key, step_dev is ADDED to the host step (what a captured graph re-keys through)"""
    m, n, k, rows = 9, 9, 5, player.key_rows
    obs = torch.from_numpy(positions(m, n, k, rows, 6)).to(DEV)
    want_a, want_o = player.act(hip, obs.cpu().numpy(), k, player.keys, seed=0x1234_5678_9ABC, step=11)
    pol = player.make(hip, k, player.keys, seed=99)
    pol._sampler.seed_dev = torch.tensor([0x1234_5678_9ABC], dtype=torch.int64, device=DEV)
    pol._sampler.step_dev = torch.tensor([8], dtype=torch.int64, device=DEV)
    pol._sampler.calls = 3
    out = torch.empty((rows, player.planes, m * n), dtype=torch.int32, device=DEV)
    got = pol.act({"observation": obs}, **{player.out: out})
    assert np.array_equal(got.cpu().numpy(), want_a) and np.array_equal(out.cpu().numpy(), want_o)
    assert pol._sampler.calls == 3  # the position lives in step_dev


@PLAYERS
def test_empty_batch_full_boards_and_shapes(hip, player):
    m, n, k = 3, 3, 3
    pol = player.make(hip, k, player.empty, seed=1)
    assert pol.act({"observation": torch.zeros((0, 2, m, n), device=DEV)}).shape == (0,)
    full = np.zeros((3, 2, m, n), np.float32)
    full[:, 0].reshape(3, -1)[:, ::2] = 1
    full[:, 1].reshape(3, -1)[:, 1::2] = 1
    got, out = player.act(hip, full, k, player.full, seed=1)
    x = philox.rand_u32(1, np.arange(3, dtype=np.uint64), 0, philox.STREAM_SAMPLE)
    assert np.array_equal(got, philox.mulhi32(x, m * n)) and not out.any()  # a draw over all C cells, no playouts
    one = pol.act({"observation": torch.zeros((2, m, n), device=DEV)}, deterministic=True)  # a 3-D observation, call 1
    want = player.rule(np.zeros((1, 2, m, n), np.float32), k, *player.full, seed=1, step=1, deterministic=True)[0]
    assert one.shape == (1,) and int(one[0]) == int(want[0])
    obs = {"observation": torch.zeros((2, 2, m, n), device=DEV)}
    planes, other = player.planes, 5 - player.planes  # (the other player's plane count: 2 <-> 3)
    for bad in (torch.zeros((2, planes, 9), device=DEV), torch.zeros((2, 9), dtype=torch.int32, device=DEV),
                torch.zeros((2, other, 9), dtype=torch.int32, device=DEV), torch.zeros((2, planes, 9), dtype=torch.int32),
                torch.zeros((2, 9, planes), dtype=torch.int32, device=DEV).transpose(1, 2)):
        with pytest.raises(ValueError):
            pol.act(obs, **{player.out: bad})
    for budget in player.bad_budgets:
        with pytest.raises(ValueError):
            player.make(hip, k, budget)


# ----------------------------------------------------------------------------- as an opponent
@PLAYERS
def test_wrapper_opponent_plays_every_game_to_its_end(hip, player):
    """the generic pre -> act -> post path with the player as the opponent (strict env: every reply is legal) plays every
    game to its end; validate_gpu against it"""
    m, n, k, nenv = 6, 6, 4, 64
    env = hip.Env(m, n, k, nenv, device=DEV, strict=True)
    w = hip.Wrapper(env, seed=3)
    opp = player.make(hip, k, player.opponent, seed=4)
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
    res = hip.validation.validate_gpu(hip.policy.RandomPolicy(m * n, seed=1), player.make(hip, k, player.validate, seed=2),
                                      (m, n, k), 256)
    key = "validation/vs_benchmark/"
    assert res[key + "games_played"] == 256
    assert res[key + "loss_rate"] > 0.6, res  # the random agent loses most games to the player


@PLAYERS
def test_a_captured_rollout_plays_the_opponent(hip, player):
    """``set_opponent(player)`` on a captured wrapper: the graph is marked stale and recaptured with the policy's act in
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
                w.set_opponent(player.make(hip, k, player.captured, seed=77))
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
    w.set_opponent(player.make(hip, k, player.captured, seed=77))
    assert roll._stale
    for r in range(3):
        if r:
            roll.run()
        got = (buf.observations[:steps], buf.rewards[:steps], buf.dones[:steps])
        assert all(torch.equal(a, b) for a, b in zip(got, want[r])), r
    assert not torch.equal(want[2][0], eager(switch_after=99)[2][0])  # the opponent did change the games
