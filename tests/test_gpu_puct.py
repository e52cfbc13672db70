"""GPU: the PUCT search player -- ``mnk_puct_begin`` / ``mnk_puct_step`` through ``PUCTSearchPolicy.act`` bit for bit against
the numpy rule (tests/puct_rule.py): actions, root visits, root values and every leaf the kernel wrote, with an exact
evaluator on five built-in and two generic boards, every observation / leaf / prior dtype, both temperatures, finished
and full rows and the device key words; a conv net replayed from its recorded outputs; the largest budget; a captured
act() and a captured rollout with the player as the opponent; the strength ladder."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from player_cases import DEV, _score, hip, positions  # noqa: F401 (hip: the fixture)
from puct_rule import puct
from search_selfplay_async_rule import exact_np  # (the table and the value of ``exact_torch`` below, in numpy)

pytestmark = pytest.mark.gpu
DTYPES = (torch.float32, torch.bfloat16, torch.uint8)


def prior_table(C):
    """a per-cell table of dyadic f32 values (exact in bfloat16 too)"""
    return ((np.arange(C) * 37) % 16 + 1).astype(np.float32) / 16


def exact_torch(C, out_dtype=torch.float32, record=None):
    """the same on the GPU, in plain torch ops (capturable); ``record``: a list that receives each call's inputs"""
    table = torch.from_numpy(prior_table(C)).to(DEV)

    def evaluate(leaf_obs, leaf_mask):
        if record is not None:
            record.append((leaf_obs.float().cpu().numpy(), leaf_mask.cpu().numpy()))
        cnt = leaf_obs.float().reshape(len(leaf_obs), 2, -1).sum(dim=2)
        v = (torch.remainder(cnt[:, 0] - 2 * cnt[:, 1], 5) - 2) / 4
        return (leaf_mask.float() * table).to(out_dtype), v.to(out_dtype)

    return evaluate


def act(hip, obs_np, k, I, evaluator, seed, step=0, env_id0=0, dtype=torch.float32, leaf_dtype=torch.float32,
        temperature=0, deterministic=False, c=1.25, keys=False):
    b, _, m, n = obs_np.shape
    pol = hip.policy.PUCTSearchPolicy(k, evaluator=evaluator, iterations=I, c=c, temperature=temperature,
                                      leaf_dtype=leaf_dtype, seed=0 if keys else seed)
    pol._sampler.env_id0 = env_id0
    if keys:  # seed_dev replaces the key, step_dev is added to the host step
        pol._sampler.seed_dev = torch.tensor([seed], dtype=torch.int64, device=DEV)
        pol._sampler.step_dev = torch.tensor([step - 1], dtype=torch.int64, device=DEV)
        pol._sampler.calls = 1
    else:
        pol._sampler.calls = step
    visits = torch.full((b, m * n), -7, dtype=torch.int32, device=DEV)
    value = torch.full((b,), -7.0, device=DEV)
    a = pol.act({"observation": torch.from_numpy(obs_np).to(DEV).to(dtype)}, deterministic=deterministic,
                visits=visits, root_value=value)
    return a.cpu().numpy(), visits.cpu().numpy(), value.cpu().numpy()


# ----------------------------------------------------------------------------- 1. exact evaluators
@pytest.mark.parametrize("board,rows,I", [
    ((3, 3, 3), 24, 40), ((9, 9, 5), 8, 96), ((13, 13, 5), 4, 48), ((15, 15, 5), 4, 40), ((19, 19, 5), 4, 48),
    ((7, 7, 4), 8, 64), ((12, 12, 5), 4, 40), ((7, 9, 7), 4, 40),  # (generic NW forms: two, eight and four words)
    ((17, 17, 5), 3, 8), ((25, 25, 5), 3, 8),  # (10 and 21 words: the forms of sixteen and of thirty-two)
])
def test_exact_evaluator_equals_the_rule(hip, board, rows, I):
    m, n, k = board
    C = m * n
    obs = positions(m, n, k, rows, m * 100 + n * 10 + k, max_fill=0.6 if m > 9 else 1.0)  # finished rows and a full one
    seed, step, env_id0, c = 1000 + I, 3, 17, 1.25
    leaves = []
    want = {}
    for temperature in (0, 1):
        for det in (False, True):
            want[temperature, det] = puct(obs, k, I, c, exact_np(C), seed, step, env_id0, temperature, det,
                                          leaves=leaves if not want else None)
    assert (want[0, False][1].sum(axis=1)[1:] <= I).all() and not want[0, False][1][1].any()  # row 1 is full
    case = 0
    for dtype in DTYPES:
        for leaf_dtype in DTYPES:
            out_dtype = (torch.float32, torch.bfloat16)[case % 2]
            temperature, det = (case // 2) % 2, case % 3 == 0
            rec = []
            got = act(hip, obs, k, I, exact_torch(C, out_dtype, rec), seed, step, env_id0, dtype, leaf_dtype,
                      temperature, det, c, keys=case % 4 == 1)
            w = want[temperature, det]
            what = (dtype, leaf_dtype, out_dtype, temperature, det)
            assert np.array_equal(got[1], w[1]), what
            assert np.array_equal(got[0], w[0]), what
            assert np.array_equal(got[2].view(np.uint32), w[2].view(np.uint32)), what
            assert len(rec) == I + 1
            for e, ((lo, lm), (wo, wm)) in enumerate(zip(rec, leaves)):
                assert np.array_equal(lo, wo) and np.array_equal(lm, wm), (what, e)
            case += 1


def test_device_key_words_and_both_temperatures_on_one_board(hip):
    m, n, k, rows, I = 9, 9, 5, 16, 64
    obs = positions(m, n, k, rows, 7, max_fill=0.5)
    for temperature in (0, 1):
        for keys in (False, True):
            want = puct(obs, k, I, 2.0, exact_np(m * n), 99, 5, 3, temperature)
            got = act(hip, obs, k, I, exact_torch(m * n), 99, 5, 3, temperature=temperature, c=2.0, keys=keys)
            assert all(np.array_equal(g, w) for g, w in zip(got, want)), (temperature, keys)


# ----------------------------------------------------------------------------- 2. a real conv net
class ConvNet(nn.Module):
    def __init__(self, cells):
        super().__init__()
        self.body = nn.Sequential(nn.Conv2d(2, 16, 3, padding=1), nn.ReLU(), nn.Conv2d(16, 16, 3, padding=1), nn.ReLU())
        self.pi = nn.Conv2d(16, 1, 1)
        self.v = nn.Linear(16, 1)

    def forward(self, obs, action_mask=None):
        h = self.body(obs.float())
        logits = self.pi(h).flatten(1)
        if action_mask is not None:
            logits = torch.where(action_mask.bool(), logits, torch.full_like(logits, -torch.inf))
        return (torch.distributions.Categorical(logits=logits, validate_args=False),
                torch.tanh(self.v(h.mean(dim=(2, 3)))))


def test_a_conv_net_is_replayed_from_its_recorded_outputs(hip):
    """the rule, fed the net's recorded outputs call by call, asks for exactly the leaves the kernel wrote and arrives
    at the same actions, visits and root values"""
    m, n, k, rows, I = 9, 9, 5, 32, 64
    torch.manual_seed(0)
    net = ConvNet(m * n).to(DEV).eval()
    rec_in, rec_out = [], []

    def recording(leaf_obs, leaf_mask):
        with torch.no_grad():
            dist, v = net(leaf_obs, leaf_mask)
        p, v = dist.probs, v.reshape(-1)
        rec_in.append((leaf_obs.float().cpu().numpy(), leaf_mask.cpu().numpy()))
        rec_out.append((p.cpu().numpy(), v.cpu().numpy()))
        return p, v

    obs = positions(m, n, k, rows, 11, max_fill=0.7)
    got = act(hip, obs, k, I, recording, seed=4, step=2)
    calls = iter(rec_out)
    leaves = []
    want = puct(obs, k, I, 1.25, lambda o, msk: next(calls), 4, 2, leaves=leaves)
    assert len(leaves) == len(rec_in) == I + 1
    for e, ((lo, lm), (wo, wm)) in enumerate(zip(rec_in, leaves)):
        assert np.array_equal(lo, wo) and np.array_equal(lm, wm), e
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    # the default evaluator of a reference-style model is the same net
    pol = hip.policy.PUCTSearchPolicy(k, model=net, iterations=I, seed=4)
    pol._sampler.calls = 2
    a = pol.act({"observation": torch.from_numpy(obs).to(DEV)})
    assert np.array_equal(a.cpu().numpy(), want[0])


# ----------------------------------------------------------------------------- 3. the largest budget
def test_largest_budget_matches_the_rule_on_one_row(hip):
    obs = np.zeros((1, 2, 3, 3), np.float32)
    obs[0, 1, 1, 1] = 1
    want = puct(obs, 3, 2048, 1.25, exact_np(9), 5)
    got = act(hip, obs, 3, 2048, exact_torch(9), 5)
    assert all(np.array_equal(g, w) for g, w in zip(got, want)) and got[1].sum() == 2048


# ----------------------------------------------------------------------------- 4. capture
def test_a_captured_act_equals_eager(hip):
    m, n, k, rows, I = 9, 9, 5, 64, 32
    obs = {"observation": torch.from_numpy(positions(m, n, k, rows, 5, max_fill=0.5)).to(DEV)}
    eager = hip.policy.PUCTSearchPolicy(k, evaluator=exact_torch(m * n), iterations=I, temperature=1, seed=6)
    eager.act(obs)
    ev, er = torch.zeros((rows, m * n), dtype=torch.int32, device=DEV), torch.zeros(rows, device=DEV)
    ea = eager.act(obs, visits=ev, root_value=er)  # call 1

    pol = hip.policy.PUCTSearchPolicy(k, evaluator=exact_torch(m * n), iterations=I, temperature=1, seed=6)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pol.act(obs)  # call 0: the buffers
    torch.cuda.current_stream().wait_stream(side)
    gv, gr = torch.zeros_like(ev), torch.zeros_like(er)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ga = pol.act(obs, visits=gv, root_value=gr)  # call 1, baked
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(ga, ea) and torch.equal(gv, ev) and torch.equal(gr.view(torch.int32), er.view(torch.int32))


def test_a_captured_rollout_plays_the_opponent(hip):
    """``set_opponent(PUCTSearchPolicy)`` on a captured wrapper: the graph is marked stale and recaptured with the
    policy's act (and its evaluator) in it, keyed through the device words -- the rollouts equal the eager loop that
    switched at the same point"""
    m, n, k, nenv, steps = 6, 6, 4, 128, 5

    def player():
        return hip.policy.PUCTSearchPolicy(k, evaluator=exact_torch(m * n), iterations=12, temperature=1, seed=77)

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
                w.set_opponent(player())
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
    w.set_opponent(player())
    assert roll._stale
    for r in range(3):
        if r:
            roll.run()
        got = (buf.observations[:steps], buf.rewards[:steps], buf.dones[:steps])
        assert all(torch.equal(a, b) for a, b in zip(got, want[r])), r
    assert not torch.equal(want[2][0], eager(switch_after=99)[2][0])  # the opponent did change the games


def test_wrapper_opponent_plays_every_game_to_its_end(hip):
    m, n, k, nenv = 6, 6, 4, 64
    env = hip.Env(m, n, k, nenv, device=DEV, strict=True)
    w = hip.Wrapper(env, seed=3)
    opp = hip.policy.PUCTSearchPolicy(k, evaluator=exact_torch(m * n), iterations=16, seed=4)
    w.set_opponent(opp)
    agent = hip.policy.RandomPolicy(m * n, seed=5)
    obs, _ = w.reset()
    ended = torch.zeros(nenv, dtype=torch.bool)
    for _ in range(m * n):
        obs, r, term, _, _ = w.step(agent.act(obs))
        ended |= term.cpu()
        if bool(ended.all()):
            break
    assert bool(ended.all()) and opp._sampler.calls > 0


# ----------------------------------------------------------------------------- 5. strength
def solved_3x3x3():
    """the value of every 3x3x3 position for its side to move (+1 win, 0 draw, -1 loss), indexed by sum 3^a * s_a with
    s_a = 1 for a stone of the side to move, 2 for one of the other side (positions already decided: 0)"""
    lines = [(0, 1, 2), (3, 4, 5), (6, 7, 8), (0, 3, 6), (1, 4, 7), (2, 5, 8), (0, 4, 8), (2, 4, 6)]
    memo = {}

    def won(cells, s):
        return any(all(cells[a] == s for a in line) for line in lines)

    def value(cells):  # the side to move owns the 1s
        key = tuple(cells)
        if key in memo:
            return memo[key]
        if won(cells, 2) or won(cells, 1) or all(cells):
            memo[key] = 0
            return 0
        best = -1
        for a in range(9):
            if not cells[a]:
                nxt = [(2 if x == 1 else 1 if x == 2 else 0) for x in cells]
                nxt[a] = 2  # the mover's stone, seen from the other side
                if won(nxt, 2):
                    best = 1
                    break
                best = max(best, -value(nxt) if any(x == 0 for x in nxt) else 0)
        memo[key] = best
        return best

    table = np.zeros(3 ** 9, np.float32)
    for idx in range(3 ** 9):
        cells = [(idx // 3 ** a) % 3 for a in range(9)]
        table[idx] = value(cells)
    return table


def minimax_evaluator():
    table = torch.from_numpy(solved_3x3x3()).to(DEV)
    weights = torch.tensor([3 ** a for a in range(9)], dtype=torch.float32, device=DEV)

    def evaluate(leaf_obs, leaf_mask):
        o = leaf_obs.float().reshape(len(leaf_obs), 2, 9)
        idx = ((o[:, 0] + 2 * o[:, 1]) * weights).sum(dim=1).long()
        cnt = leaf_mask.float().sum(dim=1, keepdim=True).clamp(min=1)
        return leaf_mask.float() / cnt, table[idx]

    return evaluate


def test_strength_with_an_exact_evaluator_on_3x3x3(hip):
    """PUCT(64) with the solved game as its evaluator and uniform priors loses no game of 1024 (half as black) against
    Random, Tactical and SearchPolicy(128).  Measured on the MI355X (W / D / L): 959 / 65 / 0, 561 / 463 / 0, 0 / 1024 / 0"""
    pol = hip.policy
    board = (3, 3, 3)
    for i, opp in enumerate((pol.RandomPolicy(9, seed=2), pol.TacticalPolicy(3, seed=4), pol.SearchPolicy(3, 128, 32,
                                                                                                         seed=6))):
        me = pol.PUCTSearchPolicy(3, evaluator=minimax_evaluator(), iterations=64, seed=10 + i)
        res = hip.tournament.play_match(me, opp, board, 1024, device=DEV)
        print(type(opp).__name__, res)
        assert res["losses"] == 0, (type(opp).__name__, res)


def heuristic_evaluator(k, playouts=4):
    """a network-free evaluator for 9x9x5: priors uniform over TacticalPolicy's candidate set, value = the best
    wins-minus-losses rate of MonteCarloPolicy's playout counts over the legal cells"""
    from selfplay.policy import MonteCarloPolicy, TacticalPolicy

    tac, mc = TacticalPolicy(k, seed=31), MonteCarloPolicy(k, playouts, seed=32)

    def evaluate(leaf_obs, leaf_mask):
        b, C = leaf_mask.shape
        cand = torch.empty((b, C), dtype=torch.uint8, device=leaf_obs.device)
        counts = torch.empty((b, 2, C), dtype=torch.int32, device=leaf_obs.device)
        tac.act({"observation": leaf_obs}, candidates=cand)
        mc.act({"observation": leaf_obs}, counts=counts)
        score = (counts[:, 0] - counts[:, 1]).float() / playouts
        score = torch.where(leaf_mask, score, torch.full_like(score, -2.0)).amax(dim=1).clamp(min=-1.0)
        c = cand.float()
        return c / c.sum(dim=1, keepdim=True).clamp(min=1), score

    return evaluate


def test_strength_ordering_on_9x9x5(hip):
    """on 9x9x5 with the heuristic evaluator: PUCT(256) beats PUCT(16) and the raw prior's policy (uniform over the
    tactical candidates: TacticalPolicy); 256 games each (half as black).  Measured on the MI355X: PUCT(256) vs PUCT(16)
    0.7520, PUCT(256) vs Tactical 0.9160.  A score over 256 games has a standard error of at most 0.031; every threshold
    lies 0.16 (over 5 SE) below the measured score"""
    pol = hip.policy
    board, games = (9, 9, 5), 256
    big = pol.PUCTSearchPolicy(5, evaluator=heuristic_evaluator(5), iterations=256, seed=1)
    small = pol.PUCTSearchPolicy(5, evaluator=heuristic_evaluator(5), iterations=16, seed=2)
    big_small = _score(hip, big, small, board, games)
    big2 = pol.PUCTSearchPolicy(5, evaluator=heuristic_evaluator(5), iterations=256, seed=3)
    big_prior = _score(hip, big2, pol.TacticalPolicy(5, seed=4), board, games)
    print("PUCT(256)-PUCT(16) %.4f PUCT(256)-Tactical %.4f" % (big_small, big_prior))
    assert big_small > STRENGTH["big_small"], big_small
    assert big_prior > STRENGTH["big_prior"], big_prior


STRENGTH = {"big_small": 0.59, "big_prior": 0.75}
