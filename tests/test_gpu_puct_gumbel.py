"""GPU: the PUCT player's Gumbel root -- ``mnk_puct_gumbel_root`` against the numpy rule (tests/puct_gumbel_rule.py);
``PUCTSearchPolicy(gumbel=m).act`` bit for bit against the rule fed with the kernel's own gscore (actions, visits, root
values and every evaluation's leaf rows exactly, the improved policy to 1e-6), on a single-word board whose C is no
multiple of 4, a built-in board of C > 64 and a board without a built-in variant, rows that are no multiple of a
workgroup's four, roots without a free cell, with one and with fewer than ``considered``; sharding and a captured act;
``gumbel=None`` launch for launch the search it was; ``SearchSelfPlay(gumbel=m)`` against the self-play rule;
a guard on the strength of the player; and the example's loop with ``search="gumbel"``.

gscore and the policy are the float32 of float64 values that agree with numpy's to about 1e-15 (a few ulps of log / exp),
so rtol 1e-6 leaves some 16 float32 ulps over the half ulp of the conversion (the reasoning of tests/test_gpu_puct_noise.py).
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

from player_cases import DEV, hip  # noqa: F401 (hip: the fixture)
from puct_gumbel_rule import GumbelSelfPlayRule, gumbel_puct, gumbel_scores
from puct_solver_cases import drawn_board
from tactical_rule import random_positions
from test_gpu_puct_reuse import exact_np, exact_torch, same_leaves

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_PUCT, SEED, ENV_ID0, STEP, ROWS = 1.25, 53, 3, 2, 6
#        name      board      I   considered
CASES = {"3x3x3": ((3, 3, 3), 8, 4),     # NW = 1, C = 9: no multiple of 4
         "9x9x5": ((9, 9, 5), 16, 8),    # C > 64: every per-cell loop takes two trips; a built-in variant
         "5x5x4": ((5, 5, 4), 16, 4),    # the generic form
         # boards that share a built-in variant with a board of another row count (tests/test_gpu_variant_siblings.py):
         # not square, and on the k = 5 ones the Philox layout (C + 3) & ~3 of a cell count the variant's board has not
         "8x3x3": ((8, 3, 3), 16, 4), "7x9x5": ((7, 9, 5), 16, 8), "16x15x5": ((16, 15, 5), 16, 8),
         "12x13x5": ((12, 13, 5), 8, 8), "18x19x5": ((18, 19, 5), 8, 8),
         "7x9x7": ((7, 9, 7), 8, 8),     # generic, three words: the four-word instantiation
         # generic, ten and 21 words: the instantiations of sixteen and of thirty-two; C = 289 and 625, no multiples of 4
         "17x17x5": ((17, 17, 5), 8, 4), "25x25x5": ((25, 25, 5), 8, 4)}
SIBLINGS = ("8x3x3", "7x9x5", "16x15x5", "12x13x5", "18x19x5")
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}


def positions(name):
    """six rows: the empty board, a full one (F = 0), one free cell, three (1 < F < considered), two mid-game positions"""
    (m, n, k), _, cons = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    full = drawn_board(m, n, k)
    obs = np.zeros((ROWS, 2, m, n), np.float32)
    obs[1] = full
    for row, gone in ((2, 1), (3, 3)):
        keep = np.ones(m * n, bool)
        keep[rng.choice(m * n, size=gone, replace=False)] = False
        obs[row] = full[:: 1 if row % 2 else -1] & keep.reshape(m, n)
    obs[4:] = random_positions(m, n, k, 2, rng, max_fill=0.6)
    free = (obs.reshape(ROWS, 2, -1) == 0).all(axis=1).sum(axis=1)
    assert free[0] == m * n and free[1] == 0 and free[2] == 1 and 1 < free[3] < cons and (free[4:] > cons).all(), free
    return obs


def policy(hip, name, out_dtype=torch.float32, record=None, step=STEP, **kw):
    (m, n, k), I, cons = CASES[name]
    pol = hip.policy.PUCTSearchPolicy(k, evaluator=exact_torch(m * n, out_dtype, record), iterations=I, c=C_PUCT, seed=SEED,
                                      gumbel=cons, **kw)
    pol._sampler.env_id0, pol._sampler.calls = ENV_ID0, step
    return pol


def gpu_act(pol, obs_np, **kw):
    """(actions, visits, root_value, policy, the kernel's gscore) of one act"""
    b, _, m, n = obs_np.shape
    visits = torch.full((b, m * n), -7, dtype=torch.int32, device=DEV)
    value = torch.full((b,), -7.0, device=DEV)
    target = torch.full((b, m * n), -7.0, device=DEV)
    a = pol.act({"observation": torch.from_numpy(obs_np).to(DEV)}, visits=visits, root_value=value, policy=target, **kw)
    torch.cuda.synchronize()
    return a.cpu().numpy(), visits.cpu().numpy(), value.cpu().numpy(), target.cpu().numpy(), pol._gumbel_bufs[2].cpu().numpy()


def same_act(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, "actions", got[0], want[0])
    assert np.array_equal(got[1], want[1]), (what, "visits", got[1], want[1])
    assert np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32)), (what, "root_value", got[2], want[2])
    err = np.abs(got[3] - want[3])[want[3] > 0] / want[3][want[3] > 0]
    print(what, "policy: largest relative deviation %.3g" % (err.max() if len(err) else 0.0))
    np.testing.assert_allclose(got[3], want[3], rtol=1e-6, atol=0, err_msg=str(what))


# ----------------------------------------------------------------------------- 1. the prep kernel
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("name", list(CASES))
def test_the_prep_kernel_equals_the_rule(hip, name, dtype):
    lib = hip.lib
    (m, n, k), _, _ = CASES[name]
    C = m * n
    obs = positions(name)
    mask_np = (obs.reshape(ROWS, 2, C) == 0).all(axis=1)
    priors_np, values_np = exact_np(C)(obs, mask_np)
    priors = torch.from_numpy(np.asarray(priors_np, np.float32)).to(DEV).to(DTYPES[dtype])
    values = torch.from_numpy(values_np).to(DEV).to(DTYPES[dtype])
    mask = torch.from_numpy(mask_np).to(DEV)
    before = priors.clone()
    code = lib.LOGITS_BF16 if dtype == "bf16" else lib.LOGITS_F32
    for scale, step in ((1.0, STEP), (0.0, STEP), (2.5, 1 << 33)):
        gscore = torch.full((ROWS, C), 7.0, device=DEV)
        vroot = torch.full((ROWS,), 7.0, device=DEV)
        lib.call("mnk_puct_gumbel_root", lib.ptr(priors), code, lib.ptr(mask), lib.ptr(values), code, ROWS, C, scale, SEED,
                 None, step, None, ENV_ID0, lib.ptr(gscore), lib.ptr(vroot), lib.stream_ptr(DEV))
        torch.cuda.synchronize()
        want, _ = gumbel_scores(priors.float().cpu().numpy(), mask_np, scale, SEED, step, ENV_ID0)
        got = gscore.cpu().numpy()
        assert np.array_equal(np.isneginf(got), ~mask_np) and np.isfinite(got[mask_np]).all()
        err = np.abs(got[mask_np] / want[mask_np] - 1).max()
        print(f"{name} {dtype} scale {scale}: largest relative deviation {err:.3g}")
        np.testing.assert_allclose(got[mask_np], want[mask_np], rtol=1e-6, atol=0)
        assert np.array_equal(vroot.cpu().numpy(), values.float().cpu().numpy())
    assert torch.equal(priors, before)  # the evaluator's tensor is never written
    # device key words: *seed_dev replaces the seed, *step_dev is added to the step
    seed_dev = torch.full((1,), SEED, dtype=torch.int64, device=DEV)
    step_dev = torch.full((1,), STEP - 1, dtype=torch.int64, device=DEV)
    keyed = torch.empty((ROWS, C), device=DEV)
    lib.call("mnk_puct_gumbel_root", lib.ptr(priors), code, lib.ptr(mask), lib.ptr(values), code, ROWS, C, 1.0, 999,
             lib.ptr(seed_dev), 1, lib.ptr(step_dev), ENV_ID0, lib.ptr(keyed), lib.ptr(vroot), lib.stream_ptr(DEV))
    plain = torch.empty((ROWS, C), device=DEV)
    lib.call("mnk_puct_gumbel_root", lib.ptr(priors), code, lib.ptr(mask), lib.ptr(values), code, ROWS, C, 1.0, SEED, None,
             STEP, None, ENV_ID0, lib.ptr(plain), lib.ptr(vroot), lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert torch.equal(keyed, plain)


# ----------------------------------------------------------------------------- 2. the search around it
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("name", list(CASES))
def test_an_act_equals_the_rule_fed_with_the_kernels_gscore(hip, name, dtype):
    """(the evaluator's priors are powers of two and its values eighths: exact in bfloat16)"""
    (m, n, k), I, cons = CASES[name]
    obs = positions(name)
    rec = []
    got = gpu_act(policy(hip, name, DTYPES[dtype], rec), obs)
    seen = []
    want = gumbel_puct(obs, k, I, C_PUCT, exact_np(m * n), cons, seed=SEED, step=STEP, env_id0=ENV_ID0, gscore=got[4],
                       leaves=seen)
    same_leaves(rec, seen, (name, dtype))
    same_act(got, want, (name, dtype))
    occ = (obs.reshape(ROWS, 2, -1) != 0).any(axis=1)
    assert (got[3][occ] == 0).all() and (got[3][1] == 0).all() and (got[1][1] == 0).all()  # row 1: no free cell
    assert np.abs(got[3][[0, 2, 3, 4, 5]].sum(axis=1) - 1).max() < 1e-6
    assert (got[1][[0, 2, 3, 4, 5]].sum(axis=1) == I).all()
    # and the rule's own scores are the kernel's to 1e-6, so the draw is the rule's draw
    own = gumbel_puct(obs, k, I, C_PUCT, exact_np(m * n), cons, seed=SEED, step=STEP, env_id0=ENV_ID0)[4]
    free = ~occ
    np.testing.assert_allclose(got[4][free], own[free], rtol=1e-6, atol=0)


@pytest.mark.parametrize("name", ["3x3x3", "9x9x5"])
def test_a_deterministic_act_and_other_constants(hip, name):
    (m, n, k), I, cons = CASES[name]
    obs = positions(name)
    got = gpu_act(policy(hip, name), obs, deterministic=True)
    want = gumbel_puct(obs, k, I, C_PUCT, exact_np(m * n), cons, seed=SEED, step=STEP, env_id0=ENV_ID0, gscore=got[4],
                       deterministic=True)
    same_act(got, want, (name, "deterministic"))
    zero = gumbel_scores(*exact_np(m * n)(obs, (obs.reshape(ROWS, 2, -1) == 0).all(axis=1))[:1],
                         (obs.reshape(ROWS, 2, -1) == 0).all(axis=1), 0.0)[0]
    free = np.isfinite(zero)
    np.testing.assert_allclose(got[4][free], zero[free], rtol=1e-6, atol=0)  # gumbel_scale = 0: ln P, no draw
    again = gpu_act(policy(hip, name, step=STEP + 5), obs, deterministic=True)
    assert np.array_equal(again[0][[0, 2, 3, 4, 5]], got[0][[0, 2, 3, 4, 5]]) and np.array_equal(again[3], got[3])
    pol = policy(hip, name, gumbel_c=(20.0, 1.0), gumbel_scale=0.5)
    got = gpu_act(pol, obs)
    want = gumbel_puct(obs, k, I, C_PUCT, exact_np(m * n), cons, c_visit=20.0, c_scale=1.0, seed=SEED, step=STEP,
                       env_id0=ENV_ID0, gscore=got[4])
    same_act(got, want, (name, "constants"))


# ----------------------------------------------------------------------------- 3. reproducibility
@pytest.mark.parametrize("name", ["3x3x3", "9x9x5"])
def test_two_shards_equal_one_call(hip, name):
    obs = positions(name)
    whole = gpu_act(policy(hip, name), obs)
    half = ROWS // 2
    lo = gpu_act(policy(hip, name), obs[:half])
    hi_pol = policy(hip, name)
    hi_pol._sampler.env_id0 = ENV_ID0 + half
    hi = gpu_act(hi_pol, obs[half:])
    for j in range(5):
        both = np.concatenate([lo[j], hi[j]])
        assert np.array_equal(both.view(np.uint32) if both.dtype == np.float32 else both,
                              whole[j].view(np.uint32) if whole[j].dtype == np.float32 else whole[j]), (name, j)


def test_a_captured_act_replayed_equals_eager(hip):
    name = "9x9x5"
    (m, n, k), I, cons = CASES[name]
    C = m * n
    obs_np = positions(name)
    want = gpu_act(policy(hip, name), obs_np)
    pol = policy(hip, name, step=0)
    pol._sampler.step_dev = torch.full((1,), STEP, dtype=torch.int64, device=DEV)
    obs = torch.zeros((ROWS, 2, m, n), device=DEV)
    visits = torch.zeros((ROWS, C), dtype=torch.int32, device=DEV)
    value = torch.zeros(ROWS, device=DEV)
    target = torch.zeros((ROWS, C), device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pol.act({"observation": obs})  # eager, on empty boards: the buffers and the table
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        actions = pol.act({"observation": obs}, visits=visits, root_value=value, policy=target)
    obs.copy_(torch.from_numpy(obs_np))
    graph.replay()
    torch.cuda.synchronize()
    got = (actions.cpu().numpy(), visits.cpu().numpy(), value.cpu().numpy(), target.cpu().numpy())
    for j in range(4):
        assert np.array_equal(got[j], want[j]), j


# ----------------------------------------------------------------------------- 4. gumbel=None
@pytest.mark.parametrize("name", ["3x3x3", "9x9x5"])
def test_without_gumbel_an_act_is_launch_for_launch_the_act_it_was(hip, name, monkeypatch):
    (m, n, k), I, _ = CASES[name]
    obs = torch.from_numpy(positions(name)).to(DEV)
    called = []
    call = hip.lib.call
    monkeypatch.setattr(hip.lib, "call", lambda entry, *args: (called.append(entry), call(entry, *args))[1])
    out = []
    for kw in ({}, {"gumbel": None}):
        pol = hip.policy.PUCTSearchPolicy(k, evaluator=exact_torch(m * n), iterations=I, c=C_PUCT, seed=SEED, **kw)
        pol._sampler.env_id0, pol._sampler.calls = ENV_ID0, STEP
        visits = torch.zeros((ROWS, m * n), dtype=torch.int32, device=DEV)
        del called[:]
        a = pol.act({"observation": obs}, visits=visits)
        torch.cuda.synchronize()
        assert called == ["mnk_puct_begin"] + ["mnk_puct_step"] * (I + 1), called
        assert pol.gumbel is None and pol._gumbel_bufs is None and len(pol._bufs) == 5 and pol._bufs[4] is None
        out.append((a.cpu().numpy(), visits.cpu().numpy()))
        with pytest.raises(ValueError, match="gumbel"):
            pol.act({"observation": obs}, policy=torch.zeros((ROWS, m * n), device=DEV))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    gum = policy(hip, name)
    launches = ["mnk_puct_begin_leaves", "mnk_puct_gumbel_root"] + ["mnk_puct_step_gumbel"] * (I + 1)
    for first in (["mnk_puct_gumbel_schedule"], []):  # (a host function, once per (considered, iterations): the table)
        del called[:]
        gpu_act(gum, positions(name))
        assert called == first + launches, called


# ----------------------------------------------------------------------------- 5. search self-play
def run_selfplay(hip, board, N, I, cons, plies):
    """``plies`` plies of ``SearchSelfPlay(gumbel=cons)`` with a T = C ring against the self-play rule; returns it"""
    from selfplay.search_selfplay import SearchSelfPlay

    m, n, k = board
    C, T, seed = m * n, m * n, 13
    sp = SearchSelfPlay(m, n, k, N, evaluator=exact_torch(C), iterations=I, c=C_PUCT, capacity=T, seed=seed, device=DEV,
                        gumbel=cons)
    assert sp.policy.gumbel == cons and sp.target is not None
    sp.play(plies)
    torch.cuda.synchronize()
    rule = GumbelSelfPlayRule(m, n, k, N, T)
    obs, mask = rule.view()
    for p in range(plies):
        actions, _, _, target, _ = gumbel_puct(obs, k, I, C_PUCT, exact_np(C), cons, seed=seed, step=p)
        obs, mask = rule.step_moves(target, actions, p)
    assert not rule.errors and rule.stats[0] >= 1
    assert np.array_equal(sp.buffer.planes.cpu().numpy().view(np.uint64), rule.ring_planes)
    assert np.array_equal(sp.buffer.z.cpu().numpy(), rule.ring_z)
    assert np.array_equal(sp.obs.cpu().numpy(), obs) and np.array_equal(sp.mask.cpu().numpy(), mask)
    assert sp.stats.sum(dim=0)[:5].tolist() == rule.stats.tolist()
    got = sp.buffer.visits.cpu().numpy().view(np.uint16).astype(np.int64)
    dev = np.abs(got - rule.ring_visits.astype(np.int64)).max()
    print("ring visits: largest deviation", dev, "counts; row sums", got.sum(axis=2).min(), "..", got.sum(axis=2).max())
    assert dev <= 1
    # the gather gives the target back to 1.5e-5
    b = sp.buffer.sample(64, generator=torch.Generator(device=DEV).manual_seed(1))
    assert torch.all((b["policy"].sum(dim=1) - 1).abs() < 1e-4)
    sp.env.check_errors()
    return sp


def test_search_selfplay_with_a_gumbel_root_equals_the_rule(hip):
    m, n, k, N, I, cons, plies = 3, 3, 3, 8, 8, 4, 12
    C, T = m * n, m * n
    sp = run_selfplay(hip, (m, n, k), N, I, cons, plies)

    # an occupied action sets the error and the row is not played; so does one out of range
    lib = hip.lib
    env = sp.env
    planes, meta = env._planes.clone(), env._meta.clone()
    occupied = (~sp.mask).float().argmax(dim=1)
    even = torch.arange(N, device=DEV) % 2 == 0
    has_stone = (~sp.mask).any(dim=1) & even  # these rows are sent to an occupied cell, the others to a free one
    legal = sp.mask.float().argmax(dim=1)
    assert bool(has_stone.any())
    actions = torch.where(has_stone, occupied, legal).to(torch.int64)
    obs_before = sp.obs.clone()
    lib.call("mnk_search_selfplay_step_moves", lib.ptr(env._planes), lib.ptr(env._meta), N, m, n, k, lib.ptr(sp.target),
             lib.ptr(actions), plies, None, T, lib.ptr(sp.buffer.planes), lib.ptr(sp.buffer.visits), lib.ptr(sp.buffer.z),
             lib.ptr(sp.obs), lib.OBS_F32, lib.ptr(sp.mask), lib.ptr(sp.stats), lib.ptr(env._err), lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    rows = has_stone.cpu().numpy()
    assert np.array_equal(env._meta.cpu().numpy()[rows], meta.cpu().numpy()[rows])
    assert np.array_equal(env._planes.cpu().numpy()[..., rows], planes.cpu().numpy()[..., rows])
    assert np.array_equal(sp.obs.cpu().numpy()[rows], obs_before.cpu().numpy()[rows])
    assert not np.array_equal(env._meta.cpu().numpy()[~rows], meta.cpu().numpy()[~rows])  # the other rows were played
    assert int(env._err[0]) == lib.ERR_ILLEGAL_MOVE
    with pytest.raises(Exception):
        env.check_errors()


def test_a_captured_ply_and_a_restored_state_continue_bit_exactly(hip):
    from selfplay.search_selfplay import SearchSelfPlay

    m, n, k, N, I, cons = 3, 3, 3, 8, 8, 4
    C = m * n

    def new():
        return SearchSelfPlay(m, n, k, N, evaluator=exact_torch(C), iterations=I, c=C_PUCT, capacity=2 * C, seed=21,
                              device=DEV, gumbel=cons)

    def ring(sp):
        torch.cuda.synchronize()
        return [t.cpu().numpy().copy() for t in (sp.buffer.planes, sp.buffer.visits, sp.buffer.z, sp.obs)]

    eager = new()
    eager.play(10)
    want = ring(eager)
    saved = new()
    saved.play(4)
    state = saved.state_dict()
    restored = new()
    restored.load_state_dict(state)
    restored.play(6)
    for g, w in zip(ring(restored), want):
        assert np.array_equal(g, w)
    cap = new()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        cap.play(1)  # eager: the buffers
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap.play(1)
    cap.buffer.plies_host -= 1  # (the capture enqueued nothing)
    for _ in range(9):
        graph.replay()
    cap.note_replayed(9)
    for g, w in zip(ring(cap), want):
        assert np.array_equal(g, w)


# ----------------------------------------------------------------------------- 6. strength
GUMBEL_MIN = 0.5 - 5 * 0.03125


def test_gumbel_does_not_weaken_the_player_at_sixteen_simulations_on_9x9x5(hip):
    """Gumbel(I = 16, m = 8) against PUCT(I = 16), both on the heuristic evaluator of tests/test_gpu_puct.py, 256 games
    (half as black).  The standard error is at most 0.5 / sqrt(256) = 0.03125 and the threshold lies 5 of them below one
    half: a guard against a Gumbel root that weakens the player.  Measured on the MI355X: 0.6387 (163 W / 1 D / 92 L), 4.4
    standard errors above one half; against PUCT(64) 0.5293 (134 / 3 / 119) and against PUCT(256) 0.2422 (62 / 0 / 194),
    neither asserted"""
    from test_gpu_puct import heuristic_evaluator

    pol = hip.policy
    gumbel = pol.PUCTSearchPolicy(5, evaluator=heuristic_evaluator(5), iterations=16, seed=14, gumbel=8)
    plain = pol.PUCTSearchPolicy(5, evaluator=heuristic_evaluator(5), iterations=16, seed=15)
    res = hip.tournament.play_match(gumbel, plain, (9, 9, 5), 256, device=DEV)
    print("Gumbel(16, 8)-PUCT(16) %.4f (%d W / %d D / %d L)" % (res["score"], res["wins"], res["draws"], res["losses"]))
    assert res["wins"] + res["losses"] + res["draws"] == 256
    assert res["score"] > GUMBEL_MIN, res


# ----------------------------------------------------------------------------- 7. the example
# strength of the example's short loop on 3x3x3 with a Gumbel root at I = 16, m = 4: score rates of the greedy net over
# 1 024 games measured 0.8867 vs RandomPolicy (799 W / 218 D / 7 L, standard error 0.0068) and 0.5601 vs TacticalPolicy
# (145 W / 857 D / 22 L, standard error 0.0060); the thresholds sit 5 standard errors below
RANDOM_MIN, TACTICAL_MIN = 0.8867 - 5 * 0.0068, 0.5601 - 5 * 0.0060


def test_the_examples_loop_learns_tic_tac_toe_with_a_gumbel_root(hip):
    path = os.path.join(ROOT, "examples", "alphazero_selfplay.py")
    spec = importlib.util.spec_from_file_location("alphazero_selfplay", path)
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    net = ex.train(3, 3, 3, envs=256, iterations=16, rounds=12, updates=40, seed=0, search="gumbel", log=print)
    res = ex.validate(net, 3, 3, 3, episodes=1024)
    print(res)
    assert res["random"]["score_rate"] >= RANDOM_MIN
    assert res["tactical"]["score_rate"] >= TACTICAL_MIN
