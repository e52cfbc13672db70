"""GPU: the one-ply tactical player (take a win, else block one, else play at random) -- ``mnk_sample_tactical`` /
``TacticalPolicy.act`` against the reference's win test (tests/golden/tactical_positions.npz) and the numpy rule
(tests/tactical_rule.py); the one-launch self-play step with it as the opponent (``mnk_selfplay_step_tactical`` and its
``_logits`` form) against ``OracleSelfPlay`` with ``PhiloxTacticalOpponent``, bit for bit; its relation to the random
opponent; the captured rollouts; ``validate_gpu`` against it."""
import os

import numpy as np
import pytest
import torch

from oracle import philox
from oracle.env_torch import OracleVectorEnv
from oracle.packing import pack_boards, unpack_boards
from oracle.selfplay_torch import OracleSelfPlay
from player_cases import DEV, hip  # noqa: F401 (hip: the fixture)
from tactical_rule import PhiloxTacticalOpponent, random_positions, tactical_moves, tactical_sets

pytestmark = pytest.mark.gpu
OBS_DTYPES = (torch.float32, torch.bfloat16, torch.uint8)


@pytest.fixture
def jit_api(hip, monkeypatch):
    """MNK_JIT_API=1 for one test: a board without a built-in variant runs its own run-time compiled kernels at once"""
    monkeypatch.setenv("MNK_JIT_API", "1")
    hip.lib.reload_config()
    yield
    monkeypatch.delenv("MNK_JIT_API")
    hip.lib.reload_config()


def sample_and_check(hip, obs_np, k, seed, dtype, deterministic):
    """TacticalPolicy.act on obs_np (canonical, float32 [P, 2, m, n]): candidates == S of the numpy rule, actions == the
    numpy draw with x = Philox(seed, row, 0, SAMPLE)"""
    p, _, m, n = obs_np.shape
    pol = hip.policy.TacticalPolicy(k, seed=seed)
    cand = torch.full((p, m * n), 7, dtype=torch.uint8, device=DEV)
    acts = pol.act({"observation": torch.from_numpy(obs_np).to(DEV).to(dtype)}, deterministic=deterministic, candidates=cand)
    s, _, _ = tactical_sets(obs_np, k)
    assert np.array_equal(cand.cpu().numpy(), s.astype(np.uint8))
    x = 0 if deterministic else philox.rand_u32(seed, np.arange(p, dtype=np.uint64), 0, philox.STREAM_SAMPLE)
    assert np.array_equal(acts.cpu().numpy(), tactical_moves(obs_np, k, x))
    return s


# ----------------------------------------------------------------------------- 1. the policy form
@pytest.mark.parametrize("tag", ["3x3x3", "4x6x3", "6x7x4", "9x9x5", "19x19x5"])
@pytest.mark.parametrize("dtype", OBS_DTYPES)
def test_candidates_equal_the_reference_fixture(hip, golden_dir, tag, dtype):
    data = np.load(os.path.join(golden_dir, "tactical_positions.npz"))
    m, n, k = (int(v) for v in tag.split("x"))
    obs = unpack_boards(data[tag + "_planes"], m, n)
    for det in (False, True):
        s = sample_and_check(hip, obs, k, 21, dtype, det)
    win, block = data[tag + "_win_mover"] != 0, data[tag + "_win_other"] != 0
    # S is W where W is not empty, else B where that is not empty: straight from the reference's own win test
    has_w, has_b = win.any(1), block.any(1)
    assert np.array_equal(s[has_w], win[has_w]) and np.array_equal(s[~has_w & has_b], block[~has_w & has_b])


@pytest.mark.parametrize("board", [(3, 3, 3), (9, 9, 5), (13, 13, 5), (15, 15, 5), (19, 19, 5), (12, 12, 5), (25, 25, 5),
                                   (5, 5, 1), (1, 6, 1), (4, 6, 3)])
def test_actions_equal_the_numpy_rule_on_fuzzed_positions(hip, board):
    m, n, k = board
    rng = np.random.default_rng(m * 100 + n * 10 + k)
    obs = random_positions(m, n, k, 48 if m * n > 200 else 160, rng)
    obs[:4] = 0                                                           # empty boards
    obs[4] = 0
    obs[4, 0].reshape(-1)[::2] = 1                                        # one full board
    obs[4, 1].reshape(-1)[1::2] = 1
    for dtype in OBS_DTYPES:
        for det in (False, True):
            sample_and_check(hip, obs, k, 5, dtype, det)
    # 3-D observation, as NNPolicy accepts
    one = hip.policy.TacticalPolicy(k, seed=5).act({"observation": torch.from_numpy(obs[7]).to(DEV)})
    assert one.shape == (1,) and int(one[0]) == int(tactical_moves(obs[7:8], k, philox.rand_u32(5, np.zeros(1, np.uint64), 0, philox.STREAM_SAMPLE))[0])


def test_run_time_compiled_sampler_equals_the_generic_one(hip, jit_api):
    m, n, k = 12, 12, 5
    obs = random_positions(m, n, k, 160, np.random.default_rng(12))
    for dtype in OBS_DTYPES:
        sample_and_check(hip, obs, k, 8, dtype, False)
    assert hip.lib.jit_api_ready(m, n, k, hip.lib.JIT_API_SAMPLE_TACTICAL)


# ----------------------------------------------------------------------------- 2. the one-launch step against the oracle
def agent_moves(mask, seed, step, nenv):
    """a row-local agent: uniform legal cell from Philox(seed, env, step, MOVE) over the row's own mask"""
    x = philox.rand_u32(seed, np.arange(nenv, dtype=np.uint64), step, philox.STREAM_MOVE)
    return philox.pick_legal(mask, x)


def run_against_oracle(hip, m, n, k, nenv, steps, logits_form, check_every=1):
    seed, id0 = 77, 1000
    env = hip.Env(m, n, k, nenv, device=DEV)
    wrap = hip.Wrapper(env, seed=seed)
    wrap.env_id0 = id0
    wrap.set_opponent(hip.policy.TacticalPolicy(k, seed=1))
    ids = np.arange(id0, id0 + nenv, dtype=np.uint64)
    state = {"step": 0, "resetting": None}

    def sides(count):
        s = torch.from_numpy(philox.draw_side(philox.rand_u32(seed, ids, state["step"], philox.STREAM_SIDE)))
        return s if count == nenv else s[torch.nonzero(state["resetting"]).squeeze(1)]

    ora = OracleSelfPlay(OracleVectorEnv(m, n, k, nenv), side_source=sides)
    opp = PhiloxTacticalOpponent(k, seed, id0)
    ora.set_opponent(opp)

    def same(o_hip, o_ora, t):
        assert torch.equal(o_hip["observation"].cpu(), o_ora["observation"]), f"obs {t}"
        assert torch.equal(o_hip["action_mask"].cpu(), o_ora["action_mask"]), f"mask {t}"
        assert torch.equal(wrap.agent_side.cpu(), ora.agent_side), f"sides {t}"
        assert torch.equal(wrap.pending_resets.cpu(), ora.pending_resets), f"pending {t}"
        assert np.array_equal(pack_boards(env.boards.cpu().numpy(), m, n), pack_boards(ora.env.boards.numpy(), m, n)), t
        assert torch.equal(env.current_player.cpu(), ora.env.current_player) and torch.equal(env.move_counts.cpu(), ora.env.move_counts)

    o1, _ = wrap.reset()
    o2, _ = ora.reset()
    same(o1, o2, "reset")
    sampler = hip.policy.HipSampler(seed=31)
    twin = hip.policy.HipSampler(seed=31)
    logits = torch.randn((nenv, m * n), generator=torch.Generator().manual_seed(3)).to(DEV)
    for t in range(steps):
        state["step"] = opp.step = t + 1
        state["resetting"] = ora.pending_resets.clone()
        if logits_form:
            want = twin.draw(logits, o1["action_mask"], False)     # mnk_sample_logits on the same stream
            o1, r1, t1, _, info = wrap.step_logits(logits, o1["action_mask"], sampler)
            assert torch.equal(info["actions"], want), f"agent draw {t}"
            acts = want.cpu()
        else:
            acts = torch.from_numpy(agent_moves(o2["action_mask"].numpy(), 9, t, nenv))
            o1, r1, t1, _, _ = wrap.step(acts.to(DEV))
        o2, r2, t2, _, _ = ora.step(acts)
        assert torch.equal(r1.cpu(), r2) and torch.equal(t1.cpu(), t2), f"rewards / terminated {t}"
        if t % check_every == 0 or t == steps - 1:
            same(o1, o2, t)
    return wrap


@pytest.mark.parametrize("logits_form", [False, True])
@pytest.mark.parametrize("m,n,k,nenv,steps", [(3, 3, 3, 200, 30), (19, 19, 5, 64, 60), (4, 6, 3, 65, 40),
                                              (7, 9, 4, 70, 40)])
def test_one_launch_tactical_step_equals_the_oracle(hip, m, n, k, nenv, steps, logits_form):
    run_against_oracle(hip, m, n, k, nenv, steps, logits_form)


@pytest.mark.parametrize("logits_form", [False, True])
def test_one_launch_tactical_step_at_full_size(hip, logits_form):
    """9x9x5 at 65 536 envs (the benchmark's size): games end from the fifth step on, later steps cover resets"""
    run_against_oracle(hip, 9, 9, 5, 65536, 14, logits_form, check_every=3)


def test_run_time_compiled_tactical_step_equals_the_oracle(hip, jit_api):
    wrap = run_against_oracle(hip, 6, 7, 4, 100, 30, False)
    run_against_oracle(hip, 6, 7, 4, 100, 30, True)
    assert hip.lib.jit_api_ready(6, 7, 4, hip.lib.JIT_API_SP_TACTICAL)
    assert hip.lib.jit_api_ready(6, 7, 4, hip.lib.jit_api_tactical_draw_kind(torch.float32))
    assert wrap.last_opponent_actions is None  # one launch: no opponent call on the host


def test_overridden_act_is_not_folded(hip):
    """a subclass that overrides act goes through pre -> act -> post (its own moves), not the built-in opponent"""
    class Lowest(hip.policy.TacticalPolicy):
        def act(self, obs, deterministic=False):
            return torch.argmax(obs["action_mask"].to(torch.uint8), dim=1)

    w = hip.Wrapper(hip.Env(3, 3, 3, 8, device=DEV), seed=2)
    w.set_opponent(Lowest(3))
    w.reset()
    assert w.last_opponent_actions is not None


# ----------------------------------------------------------------------------- 3. against the random opponent
def test_same_trajectories_as_the_random_opponent_until_s_differs(hip):
    """same wrapper seed, same (row-local) agent: every env's trajectory equals the one against RandomPolicy up to the
    step in which the tactical opponent first faces a position where S is not the legal set"""
    m, n, k, nenv, steps, seed = 6, 6, 4, 512, 24, 13
    ids = np.arange(nenv, dtype=np.uint64)
    state = {"step": 0, "resetting": None}

    def sides(count):
        s = torch.from_numpy(philox.draw_side(philox.rand_u32(seed, ids, state["step"], philox.STREAM_SIDE)))
        return s if count == nenv else s[torch.nonzero(state["resetting"]).squeeze(1)]

    first = np.full(nenv, 1 << 30)

    class Recording(PhiloxTacticalOpponent):
        def act_indexed(self, obs, idx):
            s, _, _ = tactical_sets(obs["observation"], self.k)
            differs = ~np.all(s == obs["action_mask"].numpy(), axis=1)
            rows = idx.numpy()[differs]
            first[rows] = np.minimum(first[rows], self.step)
            return super().act_indexed(obs, idx)

    ora = OracleSelfPlay(OracleVectorEnv(m, n, k, nenv), side_source=sides)
    opp = Recording(k, seed)
    ora.set_opponent(opp)
    wt, wr = hip.Wrapper(hip.Env(m, n, k, nenv, device=DEV), seed=seed), hip.Wrapper(hip.Env(m, n, k, nenv, device=DEV), seed=seed)
    wt.set_opponent(hip.policy.TacticalPolicy(k))
    wr.set_opponent(hip.policy.RandomPolicy(m * n))
    ot, _ = wt.reset()
    orr, _ = wr.reset()
    o2, _ = ora.reset()
    outs = [(ot["observation"].cpu(), orr["observation"].cpu(), None, None)]
    for t in range(steps):
        state["step"] = opp.step = t + 1
        state["resetting"] = ora.pending_resets.clone()
        at = torch.from_numpy(agent_moves(ot["action_mask"].cpu().numpy(), 4, t, nenv))
        ar = torch.from_numpy(agent_moves(orr["action_mask"].cpu().numpy(), 4, t, nenv))
        ot, rt, tt, _, _ = wt.step(at.to(DEV))
        orr, rr, tr, _, _ = wr.step(ar.to(DEV))
        o2, r2, t2, _, _ = ora.step(at)
        assert torch.equal(ot["observation"].cpu(), o2["observation"]) and torch.equal(rt.cpu(), r2), t
        outs.append((ot["observation"].cpu(), orr["observation"].cpu(), (rt.cpu(), tt.cpu()), (rr.cpu(), tr.cpu())))
    for t, (a, b, ra, rb) in enumerate(outs):
        keep = torch.from_numpy(first > t)  # step t (0 = the reset) ran before the first differing S
        assert torch.equal(a[keep], b[keep]), t
        if ra is not None:
            assert torch.equal(ra[0][keep], rb[0][keep]) and torch.equal(ra[1][keep], rb[1][keep]), t
    assert (first <= steps).sum() > nenv // 4 and (first > 3).sum() > nenv // 4  # long common prefixes, and divergence
    assert not torch.equal(outs[-1][0], outs[-1][1])


# ----------------------------------------------------------------------------- 4. captured rollouts
def eager_rollouts(hip, m, n, k, nenv, steps, rollouts, opponent, sink=True):
    w = hip.Wrapper(hip.Env(m, n, k, nenv, device=DEV), seed=5)
    w.set_opponent(opponent)
    w.track_episodes()
    buf = hip.Buffer(steps, nenv, (2, m, n), m * n, device=DEV)
    if sink:
        w.attach_sink(buf)
    sampler = hip.policy.HipSampler(seed=11)
    obs, _ = w.reset()
    got, host = [], {"episodes": 0, "wins": 0, "losses": 0, "draws": 0}
    for r in range(rollouts):
        if r:
            buf.reset()
        for _ in range(steps):
            actions, logp = sampler.draw(None, obs["action_mask"], False, want_logp=True)
            nxt, r, term, trunc, _ = w.step(actions)
            buf.add(obs["observation"], actions, r, torch.zeros(nenv, device=DEV), logp, term | trunc, obs["action_mask"])
            done = term.cpu()
            host["episodes"] += int(done.sum())
            host["wins"] += int((r.cpu()[done] > 0).sum())
            host["losses"] += int((r.cpu()[done] < 0).sum())
            host["draws"] += int((r.cpu()[done] == 0).sum())
            obs = nxt
        got.append({f: getattr(buf, f)[:steps].clone() for f in ("observations", "action_masks", "actions", "rewards", "dones")})
    return got, w, host


def test_graphed_rollout_with_the_tactical_opponent_equals_the_eager_loop(hip):
    m, n, k, nenv, steps, rollouts = 6, 6, 4, 300, 7, 3
    want, w_eager, host = eager_rollouts(hip, m, n, k, nenv, steps, rollouts, hip.policy.TacticalPolicy(k))
    plain, _, _ = eager_rollouts(hip, m, n, k, nenv, steps, rollouts, hip.policy.TacticalPolicy(k), sink=False)
    for a, b in zip(want, plain):  # the sink changes where the step writes, not what
        for f in a:
            assert torch.equal(a[f], b[f]), f
    stats = w_eager.pop_episode_stats()
    assert stats["episodes"] == host["episodes"] > 0
    assert (stats["wins"], stats["losses"], stats["draws"]) == (host["wins"], host["losses"], host["draws"])

    w = hip.Wrapper(hip.Env(m, n, k, nenv, device=DEV), seed=5)
    w.set_opponent(hip.policy.TacticalPolicy(k))
    buf = hip.Buffer(steps, nenv, (2, m, n), m * n, device=DEV)
    roll = hip.graphed.GraphedRollout(w, buf, None, seed=11)  # the warm-up is rollout 0 (board without built-in variant:
    assert hip.lib.jit_api_ready(m, n, k, hip.lib.jit_api_tactical_draw_kind(None))  # its kernel is prepared for capture)
    for r in range(rollouts):
        if r:
            roll.run()
        for f in want[r]:
            assert torch.equal(getattr(buf, f)[:steps], want[r][f]), (r, f)


def test_switching_opponents_on_a_captured_rollout_recaptures(hip):
    """RandomPolicy -> TacticalPolicy on a captured wrapper marks the graph stale; the recaptured rollout equals the
    eager loop that switched at the same point"""
    m, n, k, nenv, steps = 9, 9, 5, 256, 6

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
                w.set_opponent(hip.policy.TacticalPolicy(k))
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
    w.set_opponent(hip.policy.TacticalPolicy(k))
    assert roll._stale
    for r in range(3):
        if r:
            roll.run()
        got = (buf.observations[:steps], buf.rewards[:steps], buf.dones[:steps])
        assert all(torch.equal(a, b) for a, b in zip(got, want[r])), r
    assert not torch.equal(want[2][0], eager(switch_after=99)[2][0])  # the tactical opponent did change the games


# ----------------------------------------------------------------------------- 5. a fixed benchmark
def test_validate_against_random_scores_higher_and_takes_every_win(hip):
    m, n, k, episodes = 3, 3, 3, 4096
    rnd = hip.validation.validate_gpu(hip.policy.RandomPolicy(9, seed=1), hip.policy.RandomPolicy(9, seed=2), (m, n, k), episodes)
    tac = hip.validation.validate_gpu(hip.policy.TacticalPolicy(3, seed=1), hip.policy.RandomPolicy(9, seed=2), (m, n, k), episodes)
    key = "validation/vs_benchmark/score_rate"
    assert tac[key] >= rnd[key] + 0.1, (tac, rnd)

    # every game in which the tactical agent had a winning cell ended on that move with its win
    w = hip.Wrapper(hip.Env(m, n, k, episodes, device=DEV), seed=3)
    w.set_opponent(hip.policy.RandomPolicy(9, seed=4))
    agent = hip.policy.TacticalPolicy(3, seed=5)
    obs, _ = w.reset(options={"agent_side": (torch.arange(episodes, device=DEV) >= episodes // 2).long()})
    open_games = torch.ones(episodes, dtype=torch.bool)
    had_win = 0
    for _ in range(6):
        _, win, _ = tactical_sets(obs["observation"], k)
        can_win = torch.from_numpy(win.any(1)) & open_games
        obs, r, term, _, _ = w.step(agent.act(obs))
        r, term = r.cpu(), term.cpu()
        assert bool((term[can_win] & (r[can_win] == 1.0)).all())
        had_win += int(can_win.sum())
        open_games &= ~term
    assert had_win > episodes // 4 and not bool(open_games.any())
