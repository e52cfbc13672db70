"""GPU: the tree-search player -- ``mnk_sample_search`` / ``SearchPolicy.act`` bit for bit against the numpy rule
(tests/search_rule.py) on the five built-in boards and two generic ones, finished games included, for every observation
dtype, with and without ``deterministic``; launch-layout independence; the device key words; N = 0 and full boards; the
player as an opponent of ``TorchSelfPlayWrapper`` (eager and captured), ``validate_gpu`` and ``tournament.play_match``;
the strength ladder."""
import numpy as np
import pytest
import torch

from oracle import philox
from search_rule import search
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


def positions(m, n, k, count, seed, max_fill=1.0):
    """random positions, a quarter of them finished games (a run already on the board), an empty and a full board"""
    rng = np.random.default_rng(seed)
    live = random_positions(m, n, k, count - count // 4, rng, max_fill=max_fill)
    done = random_positions(m, n, k, count // 4, rng, max_fill=max_fill, stop_at_win=False)
    obs = np.concatenate([live, done])
    obs[0] = 0
    obs[1] = 0
    obs[1, 0].reshape(-1)[::2] = 1
    obs[1, 1].reshape(-1)[1::2] = 1
    return obs


def act(hip, obs_np, k, I, B, c, seed, step=0, env_id0=0, dtype=torch.float32, deterministic=False):
    b, _, m, n = obs_np.shape
    pol = hip.policy.SearchPolicy(k, I, B, c, seed=seed)
    pol._sampler.calls, pol._sampler.env_id0 = step, env_id0
    stats = torch.full((b, 3, m * n), -7, dtype=torch.int32, device=DEV)
    acts = pol.act({"observation": torch.from_numpy(obs_np).to(DEV).to(dtype)}, deterministic=deterministic, stats=stats)
    return acts.cpu().numpy(), stats.cpu().numpy()


def first_most_visited(stats):
    """the deterministic move from the stats: the first cell of maximal n, 0 when nothing was expanded"""
    v = stats[:, 0]
    return np.where(v.max(axis=1) > 0, v.argmax(axis=1), 0)


# ----------------------------------------------------------------------------- 1. bit for bit against the rule
@pytest.mark.parametrize("board,rows,runs", [
    ((3, 3, 3), 24, ((40, 8, 1.0), (128, 3, 0.5))),
    ((9, 9, 5), 8, ((96, 16, 1.0), (24, 64, 1.4))),
    ((13, 13, 5), 4, ((48, 8, 1.0),)),
    ((15, 15, 5), 4, ((40, 8, 1.0),)),
    ((19, 19, 5), 4, ((64, 8, 1.0),)),       # I < |L|: the root is never fully expanded
    ((7, 7, 4), 8, ((80, 16, 1.0),)),        # generic NW forms
    ((12, 12, 5), 4, ((48, 8, 0.7),)),
])
def test_actions_and_stats_equal_the_rule(hip, board, rows, runs):
    """(3x3x3, 9x9x5, 13x13x5, 15x15x5, 19x19x5: built-in variants; 7x7x4, 12x12x5: the generic NW forms)"""
    m, n, k = board
    obs = positions(m, n, k, rows, m * 100 + n * 10 + k, max_fill=0.6 if m > 9 else 1.0)
    finished = [i for i in range(rows) if completions(obs[i:i + 1, 1], np.ones((1, m, n), bool), k).any()
                or completions(obs[i:i + 1, 0], np.ones((1, m, n), bool), k).any()]
    assert finished  # boards that already hold a run are in the comparison
    for I, B, c in runs:
        step, env_id0, seed = 3, 17, 1000 + I
        want_r, want_stats = search(obs, k, I, B, c, seed, step, env_id0)
        want_d = first_most_visited(want_stats)
        for dtype in OBS_DTYPES:
            for det, want in ((False, want_r), (True, want_d)):
                got, stats = act(hip, obs, k, I, B, c, seed, step, env_id0, dtype, det)
                assert np.array_equal(stats, want_stats), (I, B, dtype, det)
                assert np.array_equal(got, want), (I, B, dtype, det)
        if board == (19, 19, 5):
            legal = ((obs[:, 0] == 0) & (obs[:, 1] == 0)).reshape(rows, -1)
            assert ((want_stats[:, 0] > 0).sum(1) < legal.sum(1))[2:].all()


def test_rows_do_not_depend_on_the_launch_layout(hip):
    """rows e.. of a batch keyed from env id 0 == the same rows launched alone with env_id0 = e"""
    m, n, k, I, B = 9, 9, 5, 48, 16
    obs = positions(m, n, k, 40, 5)
    acts, stats = act(hip, obs, k, I, B, 1.0, seed=9, step=2)
    for e, length in ((0, 1), (7, 5), (33, 7)):
        a, s = act(hip, obs[e:e + length], k, I, B, 1.0, seed=9, step=2, env_id0=e)
        assert np.array_equal(a, acts[e:e + length]) and np.array_equal(s, stats[e:e + length])


def test_device_key_words_act_as_the_host_arguments(hip):
    """seed_dev REPLACES the key, step_dev is ADDED to the host step (what a captured graph re-keys through)"""
    m, n, k, I, B = 9, 9, 5, 32, 8
    obs = torch.from_numpy(positions(m, n, k, 16, 6)).to(DEV)
    want_a, want_s = act(hip, obs.cpu().numpy(), k, I, B, 1.0, seed=0x1234_5678_9ABC, step=11)
    pol = hip.policy.SearchPolicy(k, I, B, 1.0, seed=99)
    pol._sampler.seed_dev = torch.tensor([0x1234_5678_9ABC], dtype=torch.int64, device=DEV)
    pol._sampler.step_dev = torch.tensor([8], dtype=torch.int64, device=DEV)
    pol._sampler.calls = 3
    stats = torch.empty((16, 3, m * n), dtype=torch.int32, device=DEV)
    got = pol.act({"observation": obs}, stats=stats)
    assert np.array_equal(got.cpu().numpy(), want_a) and np.array_equal(stats.cpu().numpy(), want_s)
    assert pol._sampler.calls == 3  # the position lives in step_dev


def test_largest_budget_matches_the_rule_on_one_row(hip):
    """I = 2048, B = 4 on one 3x3x3 row (the tree fills its whole LDS budget of I + 1 nodes or runs into terminals)"""
    obs = np.zeros((1, 2, 3, 3), np.float32)
    obs[0, 1, 1, 1] = 1
    want_a, want_s = search(obs, 3, 2048, 4, 1.0, seed=5)
    got, stats = act(hip, obs, 3, 2048, 4, 1.0, seed=5)
    assert np.array_equal(stats, want_s) and np.array_equal(got, want_a)
    assert stats[0, 0].sum() == 2048 * 4


def test_empty_batch_full_boards_and_shapes(hip):
    m, n, k = 3, 3, 3
    pol = hip.policy.SearchPolicy(k, 8, 4, seed=1)
    assert pol.act({"observation": torch.zeros((0, 2, m, n), device=DEV)}).shape == (0,)
    full = np.zeros((3, 2, m, n), np.float32)
    full[:, 0].reshape(3, -1)[:, ::2] = 1
    full[:, 1].reshape(3, -1)[:, 1::2] = 1
    got, stats = act(hip, full, k, 8, 4, 1.0, seed=1)
    x = philox.rand_u32(1, np.arange(3, dtype=np.uint64), 0, philox.STREAM_SAMPLE)
    assert np.array_equal(got, philox.mulhi32(x, m * n)) and not stats.any()  # a draw over all C cells, no search
    one = pol.act({"observation": torch.zeros((2, m, n), device=DEV)}, deterministic=True)  # a 3-D observation, call 1
    want = search(np.zeros((1, 2, m, n), np.float32), k, 8, 4, 1.0, seed=1, step=1, deterministic=True)[0]
    assert one.shape == (1,) and int(one[0]) == int(want[0])
    obs = {"observation": torch.zeros((2, 2, m, n), device=DEV)}
    for bad in (torch.zeros((2, 3, 9), device=DEV), torch.zeros((2, 2, 9), dtype=torch.int32, device=DEV),
                torch.zeros((2, 3, 9), dtype=torch.int32), torch.zeros((2, 9, 3), dtype=torch.int32,
                                                                      device=DEV).transpose(1, 2)):
        with pytest.raises(ValueError):
            pol.act(obs, stats=bad)


# ----------------------------------------------------------------------------- 2. as an opponent
def test_wrapper_opponent_plays_every_game_to_its_end(hip):
    """the generic pre -> act -> post path with the search opponent (strict env: every reply is legal) plays every game
    to its end; validate_gpu against it"""
    m, n, k, nenv = 6, 6, 4, 64
    env = hip.Env(m, n, k, nenv, device=DEV, strict=True)
    w = hip.Wrapper(env, seed=3)
    opp = hip.policy.SearchPolicy(k, 32, 8, seed=4)
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
    res = hip.validation.validate_gpu(hip.policy.RandomPolicy(m * n, seed=1), hip.policy.SearchPolicy(k, 64, 8, seed=2),
                                      (m, n, k), 256)
    key = "validation/vs_benchmark/"
    assert res[key + "games_played"] == 256
    assert res[key + "loss_rate"] > 0.6, res  # the random agent loses most games to the search


def test_a_captured_rollout_plays_the_search_opponent(hip):
    """``set_opponent(SearchPolicy(...))`` on a captured wrapper: the graph is marked stale and recaptured with the
    policy's act in it, keyed through the device words -- the rollouts equal the eager loop that switched at the same
    point"""
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
                w.set_opponent(hip.policy.SearchPolicy(k, 24, 8, seed=77))
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
    w.set_opponent(hip.policy.SearchPolicy(k, 24, 8, seed=77))
    assert roll._stale
    for r in range(3):
        if r:
            roll.run()
        got = (buf.observations[:steps], buf.rewards[:steps], buf.dones[:steps])
        assert all(torch.equal(a, b) for a, b in zip(got, want[r])), r
    assert not torch.equal(want[2][0], eager(switch_after=99)[2][0])  # the search opponent did change the games


# ----------------------------------------------------------------------------- 3. the strength ladder
def _score(hip, p1, p2, board, games=1024):
    res = hip.tournament.play_match(p1, p2, board, games, device=DEV)
    assert res["wins"] + res["losses"] + res["draws"] == games
    return res["score"]


@pytest.mark.parametrize("board", [(9, 9, 5), (3, 3, 3)])
def test_strength_ordering(hip, board):
    """play_match scores of player 1 over 1024 games (half as black) with these seeds and the default c, as measured on
    the MI355X (tools/exp_search.py):
        9x9x5:  Search(256) vs Random 1.0000;  vs Tactical 0.9990 (Random vs Tactical 0.0068);  Search(256) vs Search(16)
                0.9990
        3x3x3:  Search(128) vs Random 0.9785;  vs Tactical 0.6416 (Random vs Tactical 0.1147);  Search(128) vs Search(4)
                0.9565
    A score over 1024 games has a standard error of at most 0.016 (5 SE: 0.08), a difference of two at most 0.022 (5 SE:
    0.11); every threshold in LADDER lies at least 5 SE below the measured rate."""
    m, n, k = board
    pol = hip.policy
    small, large = {(9, 9, 5): (16, 256), (3, 3, 3): (4, 128)}[board]
    s_random = _score(hip, pol.SearchPolicy(k, large, 32, seed=1), pol.RandomPolicy(m * n, seed=2), board)
    s_tactical = _score(hip, pol.SearchPolicy(k, large, 32, seed=3), pol.TacticalPolicy(k, seed=4), board)
    random_tactical = _score(hip, pol.RandomPolicy(m * n, seed=5), pol.TacticalPolicy(k, seed=6), board)
    large_small = _score(hip, pol.SearchPolicy(k, large, 32, seed=7), pol.SearchPolicy(k, small, 32, seed=8), board)
    rates = (s_random, s_tactical, random_tactical, large_small)
    print(board, "Search-Random %.4f Search-Tactical %.4f Random-Tactical %.4f Large-Small %.4f" % rates)
    vs_random, vs_tactical, gap = LADDER[board]
    assert s_random > vs_random, rates
    assert s_tactical > vs_tactical, rates
    assert s_tactical > random_tactical + 0.4, rates  # the search does far better against Tactical than Random does
    assert large_small > gap, rates


# thresholds per board: Search vs Random, Search vs Tactical, Search(large I) vs Search(small I)
LADDER = {(9, 9, 5): (0.9, 0.9, 0.9), (3, 3, 3): (0.88, 0.55, 0.85)}
