"""GPU: search self-play -- ``mnk_search_selfplay_step`` bit for bit against the numpy rule (tests/search_selfplay_rule.py)
over more than two laps of the ring on built-in and generic boards, every observation dtype, three temperature switches
and the device key words (the visits are the real ``PUCTSearchPolicy.act`` output of each ply, recorded and replayed into
the rule); ``mnk_search_gather`` against the rule for every symmetry and dtype, wrapped, out-of-range and refused ids, and
against ``mnk_gather_obs``; a captured ply; a ``state_dict`` round trip; a short AlphaZero loop's strength."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from player_cases import DEV, hip  # noqa: F401 (hip: the fixture)
from search_selfplay_async_fpu_cases import late_start
from search_selfplay_rule import SelfPlayRule, gather

pytestmark = pytest.mark.gpu
DTYPES = (torch.float32, torch.bfloat16, torch.uint8)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def exact_torch(C):
    """a capturable evaluator of plain torch ops: dyadic per-cell priors on the legal cells, a value from stone counts"""
    table = (((torch.arange(C) * 37) % 16 + 1).float() / 16).to(DEV)

    def evaluate(leaf_obs, leaf_mask):
        cnt = leaf_obs.float().reshape(len(leaf_obs), 2, -1).sum(dim=2)
        return leaf_mask.float() * table, (torch.remainder(cnt[:, 0] - 2 * cnt[:, 1], 5) - 2) / 4

    return evaluate


def run(hip, m, n, k, N, plies, dtype, temp_plies, keys, I=6, seed=7, env_id0=3, start=None):
    """plays ``plies`` plies through the entry point, replaying each ply's visits into the rule; compares the next roots
    every ply and returns (rule, ring tensors).  ``start``: the env state (planes, meta) both begin from"""
    lib = hip.lib
    C, T = m * n, m * n  # the smallest ring: wraps every C plies
    env = hip.Env(m, n, k, N, device=DEV)
    env.reset()
    if start is not None:
        env._planes.copy_(torch.from_numpy(start[0].view(np.int64)))
        env._meta.copy_(torch.from_numpy(start[1].astype(np.int64)).to(env._meta.dtype))
    pol = hip.policy.PUCTSearchPolicy(k, evaluator=exact_torch(C), iterations=I, seed=seed + 1)
    W = lib.state_words(m, n)
    ring_planes = torch.zeros((T, 2, W, N), dtype=torch.int64, device=DEV)
    ring_visits = torch.zeros((T, N, C), dtype=torch.int16, device=DEV)
    ring_z = torch.full((T, N), lib.Z_UNKNOWN, dtype=torch.int8, device=DEV)
    stats = torch.zeros((lib.STATS_REPLICAS, lib.STATS_STRIDE), dtype=torch.int64, device=DEV)
    err = torch.zeros(2, dtype=torch.int32, device=DEV)
    obs = torch.zeros((N, 2, m, n), dtype=dtype, device=DEV)
    mask = torch.zeros((N, C), dtype=torch.bool, device=DEV)
    env.observe_into(obs=obs, mask=mask)
    visits = torch.zeros((N, C), dtype=torch.int32, device=DEV)
    seed_dev = torch.tensor([seed], dtype=torch.int64, device=DEV) if keys else None
    step_dev = torch.zeros(1, dtype=torch.int64, device=DEV) if keys else None
    rule = SelfPlayRule(m, n, k, N, T)
    if start is not None:
        rule.load(*start)
    for p in range(plies):
        pol.act({"observation": obs, "action_mask": mask}, visits=visits)
        if keys:
            step_dev.fill_(p - 1)
        lib.call("mnk_search_selfplay_step", lib.ptr(env._planes), lib.ptr(env._meta), N, m, n, k, lib.ptr(visits),
                 temp_plies, 0 if keys else seed, lib.ptr(seed_dev), 1 if keys else p, lib.ptr(step_dev), env_id0, T,
                 lib.ptr(ring_planes), lib.ptr(ring_visits), lib.ptr(ring_z), lib.ptr(obs), lib.obs_code(obs),
                 lib.ptr(mask), lib.ptr(stats), lib.ptr(err), lib.stream_ptr(DEV))
        r_obs, r_mask = rule.step(visits.cpu().numpy(), temp_plies, seed, p, env_id0)
        assert np.array_equal(obs.float().cpu().numpy(), r_obs), f"next roots, ply {p}"
        assert np.array_equal(mask.cpu().numpy(), r_mask), f"next mask, ply {p}"
    assert err.tolist() == [0, 0] and not rule.errors
    assert np.array_equal(ring_planes.cpu().numpy().view(np.uint64), rule.ring_planes)
    assert np.array_equal(ring_visits.cpu().numpy().view(np.uint16), rule.ring_visits)
    assert np.array_equal(ring_z.cpu().numpy(), rule.ring_z)
    assert np.array_equal(env._planes.cpu().numpy().view(np.uint64), rule.planes())
    assert np.array_equal(env._meta.cpu().numpy().astype(np.int64) & 0xFFFFFFFF, rule.meta())
    assert stats.sum(dim=0)[:5].tolist() == rule.stats.tolist()
    assert rule.stats[0] > 0  # games ended (and were labelled) inside the run
    return rule, ring_planes, ring_visits, ring_z


CASES = [  # board, rows, obs dtype, temp_plies ("C": the whole game), key words
    ((3, 3, 3), 6, 0, 0, False),
    ((3, 3, 3), 5, 1, 3, True),
    ((3, 3, 3), 7, 2, "C", False),
    ((9, 9, 5), 5, 0, 3, True),
    ((9, 9, 5), 4, 2, "C", False),
    ((19, 19, 5), 3, 1, 0, False),
    ((7, 7, 4), 5, 2, 3, True),
    ((12, 12, 5), 3, 0, "C", False),
    ((12, 12, 5), 3, 1, 0, True),
]


@pytest.mark.parametrize("board,N,dt,temp,keys", CASES)
def test_the_step_equals_the_rule(hip, board, N, dt, temp, keys):
    m, n, k = board
    C = m * n
    run(hip, m, n, k, N, 2 * C + 5, DTYPES[dt], C if temp == "C" else temp, keys)


# the generic forms of sixteen and of thirty-two words (ten and 21 words a plane: the ring's rows of 64-bit words hold
# five, and ten and a half), a few plies from ``late_start``: five rows three to eight stones short of a drawn board, so
# every row's game ends, is labelled and starts again inside the run
LATE_PLIES = 12
LATE_CASES = [((17, 17, 5), 5, 2, 3, True), ((25, 25, 5), 5, 1, 0, False)]


@pytest.mark.parametrize("board,N,dt,temp,keys", LATE_CASES)
def test_the_step_equals_the_rule_from_a_late_start(hip, board, N, dt, temp, keys):
    m, n, k = board
    rule, _, _, _ = run(hip, m, n, k, N, LATE_PLIES, DTYPES[dt], temp, keys, start=late_start(m, n, k, N))
    assert rule.stats[0] >= N and rule.ring_planes.shape[2] == (m * (n + 1) + 63) // 64


def test_a_row_without_visits_is_reported_and_left_alone(hip):
    lib = hip.lib
    m, n, k, N = 3, 3, 3, 4
    env = hip.Env(m, n, k, N, device=DEV)
    env.reset()
    visits = torch.zeros((N, 9), dtype=torch.int32, device=DEV)
    visits[:, 4] = 3
    visits[2] = -1
    ring = [torch.zeros((9, 2, 1, N), dtype=torch.int64, device=DEV), torch.zeros((9, N, 9), dtype=torch.int16, device=DEV),
            torch.zeros((9, N), dtype=torch.int8, device=DEV)]
    obs, err = torch.zeros((N, 2, 3, 3), device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV)
    lib.call("mnk_search_selfplay_step", lib.ptr(env._planes), lib.ptr(env._meta), N, m, n, k, lib.ptr(visits), 0, 1, None,
             0, None, 0, 9, *(lib.ptr(t) for t in ring), lib.ptr(obs), 0, None, None, lib.ptr(err), lib.stream_ptr(DEV))
    assert err.tolist() == [lib.ERR_VISITS, 2]
    assert env._meta.tolist() == [3, 3, 0, 3] and ring[2][0].tolist() == [lib.Z_UNKNOWN] * N
    assert obs[2].sum().item() == 0 and obs[0, 1, 1, 1].item() == 1


@pytest.mark.parametrize("board", [(3, 3, 3), (9, 9, 5), (5, 7, 4), (17, 17, 5), (25, 25, 5)])
def test_the_gather_equals_the_rule(hip, board):
    lib = hip.lib
    m, n, k = board
    C, N = m * n, 5
    late = C > 256  # (the large generic boards: LATE_PLIES plies from a late start; the written slots are sampled most)
    rule, planes, visits, z = run(hip, m, n, k, N, LATE_PLIES if late else C + 7, torch.float32, 2, False,
                                  start=late_start(m, n, k, N) if late else None)
    T = C
    count = 8 if m == n else 4
    rng = np.random.default_rng(C)
    B = 300
    idx = rng.integers(-T * N, T * N, B)
    if late:
        idx[3:250] = rng.integers(0, LATE_PLIES * N, 247) - T * N * rng.integers(0, 2, 247)
    idx[:3] = [T * N, -T * N - 1, 10 ** 9]  # out of range
    sym = rng.integers(0, count, B).astype(np.int8)
    idx_t = torch.from_numpy(idx).to(DEV)  # (held: a temporary's block could be handed to the next tensor)
    for dtype in DTYPES:
        out = {"observation": torch.empty((B, 2, m, n), dtype=dtype, device=DEV),
               "action_mask": torch.empty((B, C), dtype=torch.bool, device=DEV),
               "policy": torch.empty((B, C), device=DEV), "value": torch.empty(B, device=DEV),
               "weight": torch.empty(B, device=DEV)}
        for s_np in (sym, None):
            err = torch.zeros(2, dtype=torch.int32, device=DEV)
            s_t = None if s_np is None else torch.from_numpy(s_np).to(DEV)
            lib.call("mnk_search_gather", lib.ptr(planes), lib.ptr(visits), lib.ptr(z), T, N, m, n,
                     lib.ptr(idx_t), lib.ptr(s_t), B, lib.ptr(out["observation"]),
                     lib.obs_code(out["observation"]), lib.ptr(out["action_mask"]), lib.ptr(out["policy"]),
                     lib.ptr(out["value"]), lib.ptr(out["weight"]), lib.ptr(err), lib.stream_ptr(DEV))
            r = gather(rule.ring_planes, rule.ring_visits, rule.ring_z, m, n, idx, s_np)
            assert np.array_equal(out["observation"].float().cpu().numpy(), r[0])
            assert np.array_equal(out["action_mask"].cpu().numpy(), r[1])
            for key, ref in zip(("policy", "value", "weight"), r[2:5]):
                assert np.array_equal(out[key].cpu().numpy().view(np.int32), ref.view(np.int32)), key
            assert err[0].item() == lib.ERR_ACTION_RANGE and err[1].item() in (T * N, -T * N - 1, 10 ** 9 % 2 ** 32)
            if s_np is None:  # the identity equals mnk_gather_obs on the same planes
                ref_o, ref_m = torch.empty_like(out["observation"]), torch.empty_like(out["action_mask"])
                ok = torch.from_numpy(idx[3:]).to(DEV)
                lib.call("mnk_gather_obs", lib.ptr(planes), T, N, m, n, lib.ptr(ok), B - 3, lib.ptr(ref_o[3:]),
                         lib.obs_code(ref_o), lib.ptr(ref_m[3:]), 0, None, lib.stream_ptr(DEV))
                assert torch.equal(ref_o[3:], out["observation"][3:]) and torch.equal(ref_m[3:], out["action_mask"][3:])
    # refused symmetry ids: weight 0, the identity's planes, MNK_ERR_SYMMETRY with the sample's index
    bad = np.array([8, -1, 4 if m != n else 100, 0], np.int8)
    ids = np.array([0, 1, 2, 3], np.int64)
    outs = [torch.empty((4, 2, m, n), device=DEV), torch.empty((4, C), dtype=torch.bool, device=DEV),
            torch.empty((4, C), device=DEV), torch.empty(4, device=DEV), torch.empty(4, device=DEV)]
    err = torch.zeros(2, dtype=torch.int32, device=DEV)
    ids_t, bad_t = torch.from_numpy(ids).to(DEV), torch.from_numpy(bad).to(DEV)
    lib.call("mnk_search_gather", lib.ptr(planes), lib.ptr(visits), lib.ptr(z), T, N, m, n,
             lib.ptr(ids_t), lib.ptr(bad_t), 4, lib.ptr(outs[0]), 0,
             lib.ptr(outs[1]), lib.ptr(outs[2]), lib.ptr(outs[3]), lib.ptr(outs[4]), lib.ptr(err), lib.stream_ptr(DEV))
    r = gather(rule.ring_planes, rule.ring_visits, rule.ring_z, m, n, ids, bad)
    for got, ref in zip(outs, r[:5]):
        assert np.array_equal(got.cpu().numpy(), ref)
    assert outs[4][:3].tolist() == [0, 0, 0] and err[0].item() == lib.ERR_SYMMETRY and err[1].item() in (0, 1, 2)


def new_selfplay(hip, seed=5, **kw):
    from selfplay.search_selfplay import SearchSelfPlay

    args = dict(iterations=8, temp_plies=2, capacity=12)
    args.update(kw)
    return SearchSelfPlay(3, 3, 3, 64, evaluator=exact_torch(9), seed=seed, **args)


def same(a, b):
    assert torch.equal(a.env._planes, b.env._planes) and torch.equal(a.env._meta, b.env._meta)
    for t in ("planes", "visits", "z", "plies"):
        assert torch.equal(getattr(a.buffer, t), getattr(b.buffer, t)), t
    assert torch.equal(a.obs, b.obs) and torch.equal(a.mask, b.mask) and torch.equal(a.stats, b.stats)


def test_a_captured_ply_replayed_equals_eager_plies(hip):
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
    same(sp, eager)
    assert sp.buffer.plies_host == eager.buffer.plies_host == 1 + P
    assert eager.pop_game_stats()["games"] > 0


def test_a_state_dict_round_trip_continues_bit_exactly(hip):
    a = new_selfplay(hip, seed=9)
    a.play(7)
    state = a.state_dict()
    a.play(11)
    b = new_selfplay(hip, seed=1)
    b.load_state_dict(state)
    b.play(11)
    same(a, b)
    sa, sb = a.pop_game_stats(), b.pop_game_stats()
    assert sa == sb and sa["games"] > 0 and sa["black_wins"] + sa["white_wins"] + sa["draws"] == sa["games"]
    batch = a.buffer.sample(256, generator=torch.Generator(device=DEV).manual_seed(3))
    assert set(batch) == {"observation", "action_mask", "policy", "value", "weight"}
    w = batch["weight"] > 0
    assert w.any() and torch.allclose(batch["policy"][w].sum(dim=1), torch.ones(int(w.sum()), device=DEV))
    assert ((batch["policy"] > 0) <= batch["action_mask"]).all()
    a.buffer.check_errors()


# strength of the example's short loop on 3x3x3: score rates of the greedy net over 1 024 games measured 0.912 vs
# RandomPolicy (standard error 0.009) and 0.736 vs TacticalPolicy (0.008, no loss); the thresholds sit more than 5 standard
# errors below
RANDOM_MIN, TACTICAL_MIN, TACTICAL_LOSS_MAX = 0.8, 0.6, 0.1


def test_a_short_alphazero_loop_learns_tic_tac_toe(hip):
    path = os.path.join(ROOT, "examples", "alphazero_selfplay.py")
    spec = importlib.util.spec_from_file_location("alphazero_selfplay", path)
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    net = ex.train(3, 3, 3, envs=256, iterations=32, rounds=12, updates=40, seed=0, log=print)
    res = ex.validate(net, 3, 3, 3, episodes=1024)
    print(res)
    assert res["random"]["score_rate"] >= RANDOM_MIN
    assert res["tactical"]["score_rate"] >= TACTICAL_MIN and res["tactical"]["loss_rate"] <= TACTICAL_LOSS_MAX
