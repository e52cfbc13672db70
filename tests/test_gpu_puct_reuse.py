"""GPU: the PUCT player that keeps its tree -- ``mnk_puct_rebase`` through ``PUCTSearchPolicy(reuse=True).act`` bit for bit
against the numpy rule (tests/puct_reuse_rule.py): actions, root visits, root values, ``carried`` and the leaf observation
and mask of every evaluation, over sequences of plies in which the next root is one ply on (self-play) or two plies on (a
wrapper's opponent), with games that end and are reset inside the sequence, a tree that truncates at every ply, rows that
must start fresh, priors renewed at a carried root, every dtype, a captured act, ``SearchSelfPlay(reuse=True)`` against
the self-play rule driven by the same trees, and the strength of the player that keeps its tree against the one that does
not."""
import numpy as np
import pytest
import torch

from player_cases import DEV, _score, hip  # noqa: F401 (hip: the fixture)
from puct_reuse_cases import advance, exact_np, place, prior_table, start, value_weights  # noqa: F401
from puct_reuse_rule import ReusePuct
from search_selfplay_rule import SelfPlayRule

pytestmark = pytest.mark.gpu
C_PUCT, SEED, ENV_ID0 = 1.25, 41, 5
#         board       rows  J
BOARDS = [((3, 3, 3), 6, 10),    # NW = 1; games end inside the sequence
          ((4, 6, 3), 5, 12),    # generic, not square
          ((9, 9, 5), 6, 16),    # C > 64: every per-cell loop takes two trips; a built-in variant
          ((19, 19, 5), 3, 8),   # C = 361; fewer rows than one workgroup holds
          ((7, 9, 7), 5, 24),    # generic
          ((17, 17, 5), 3, 8),   # generic, ten words: the sixteen-word instantiation
          ((25, 25, 5), 3, 8)]   # generic, 21 words: the 32-word instantiation


def exact_torch(C, out_dtype=torch.float32, record=None, J=None):
    """the same on the GPU, in plain torch ops (capturable when it neither records nor counts)"""
    tables = [torch.from_numpy(prior_table(C, mult)).to(DEV) for mult in (1, 11)]
    weights = torch.from_numpy(value_weights(C)).to(DEV)
    calls = [0]

    def evaluate(leaf_obs, leaf_mask):
        if record is not None:
            record.append((leaf_obs.float().cpu().numpy(), leaf_mask.cpu().numpy()))
        table = tables[1 if J is not None and calls[0] % (J + 1) == 0 else 0]
        calls[0] += 1
        o = leaf_obs.float().reshape(len(leaf_obs), 2, -1)
        s = ((o[:, 0] - o[:, 1]) * weights).sum(dim=1)
        return (leaf_mask.float() * table).to(out_dtype), ((torch.remainder(s, 9) - 4) / 8).to(out_dtype)

    return evaluate


def policy(hip, k, J, C, record=None, tree_nodes=None, leaf_dtype=torch.float32, out_dtype=torch.float32, refresh=False,
           **kw):
    pol = hip.policy.PUCTSearchPolicy(k, evaluator=exact_torch(C, out_dtype, record, J if refresh else None), iterations=J,
                                      c=C_PUCT, leaf_dtype=leaf_dtype, seed=SEED, tree_nodes=tree_nodes, **kw)
    pol._sampler.env_id0 = ENV_ID0
    return pol


def gpu_act(pol, obs_np, dtype=torch.float32):
    b, _, m, n = obs_np.shape
    visits = torch.full((b, m * n), -7, dtype=torch.int32, device=DEV)
    value = torch.full((b,), -7.0, device=DEV)
    carried = torch.full((b, 2), -7, dtype=torch.int32, device=DEV) if pol.reuse else None
    a = pol.act({"observation": torch.from_numpy(obs_np).to(DEV).to(dtype)}, visits=visits, root_value=value,
                **({"carried": carried} if pol.reuse else {}))
    return (a.cpu().numpy(), visits.cpu().numpy(), value.cpu().numpy(),
            carried.cpu().numpy() if pol.reuse else np.zeros((b, 2), np.int32))


def same(got, want, what):
    for name, g, w in zip(("visits", "actions", "root_value", "carried"), (got[1], got[0], got[2], got[3]),
                          (want[1], want[0], want[2], want[3])):
        if name == "root_value":
            g, w = g.view(np.uint32), w.view(np.uint32)
        assert np.array_equal(g, w), (what, name, g, w)


def same_leaves(rec, leaves, what):
    assert len(rec) == len(leaves), what
    for e, ((lo, lm), (wo, wm)) in enumerate(zip(rec, leaves)):
        assert np.array_equal(lo, wo) and np.array_equal(lm, wm), (what, "evaluation", e)


def run_sequence(hip, board, rows, J, plies, distance, tree_nodes=None, dtype=torch.float32, leaf_dtype=torch.float32,
                 out_dtype=torch.float32, refresh=False, forced_reset=True):
    """``plies`` acts of the policy and of the rule on the same roots, everything compared at every act; returns (the
    games that ended per row, the rule's ``carried`` of every act)"""
    m, n, k = board
    C = m * n
    rec, leaves = [], []
    pol = policy(hip, k, J, C, rec, tree_nodes, leaf_dtype, out_dtype, refresh, reuse=True)
    rule = ReusePuct(k, J, C_PUCT, exact_np(C, J if refresh else None), tree_nodes, SEED, ENV_ID0, leaves=leaves)
    obs = start(m, n, k, rows, m * 100 + n * 10 + k + distance)
    resets, carried = np.zeros(rows, np.int64), []
    for ply in range(plies):
        del rec[:], leaves[:]
        want = rule.act(obs, step=ply)
        got = gpu_act(pol, obs, dtype)
        what = (board, distance, "act", ply)
        same_leaves(rec, leaves, what)
        same(got, want, what)
        assert len(rec) == J + 1
        carried.append(want[3])
        obs = advance(obs, want[0], k, distance, resets)
        if forced_reset and ply == plies // 2:  # games abandoned in the middle of the sequence: never a descendant
            obs[1::2] = 0
    return resets, np.stack(carried)


# ----------------------------------------------------------------------------- 1, 2. the next root one and two plies on
@pytest.mark.parametrize("distance", [1, 2])
@pytest.mark.parametrize("board,rows,J", BOARDS)
def test_a_sequence_of_plies_equals_the_rule(hip, board, rows, J, distance):
    resets, carried = run_sequence(hip, board, rows, J, 12, distance, forced_reset=board != (3, 3, 3))
    if board == (3, 3, 3):
        assert (resets >= 1).all(), resets  # every row's game ended, and was reset, inside the sequence
    assert (carried[1:, :, 0] > 1).any() and (carried[1:, :, 0] == 0).any()  # trees were carried, and rows began afresh
    assert not carried[0].any()


# ----------------------------------------------------------------------------- 3. every ply truncates
@pytest.mark.parametrize("board,rows,J", [BOARDS[2], BOARDS[0]])
def test_the_smallest_workspace_truncates_at_every_ply(hip, board, rows, J):
    resets, carried = run_sequence(hip, board, rows, J, 12, 1, tree_nodes=J + 2, forced_reset=False)
    assert carried[:, :, 0].max() == 2 and (carried[1:, :, 1] > 2).any()  # two nodes kept of a child with more visits


# ----------------------------------------------------------------------------- 4. rows that must start fresh
def test_fresh_rows_equal_a_policy_without_reuse(hip):
    """the first act on the zeroed workspace, an act after ``reset_tree()`` and an act on unrelated positions"""
    (m, n, k), rows, J = BOARDS[2][0], 6, 16
    C = m * n
    rec, rec0 = [], []
    pol = policy(hip, k, J, C, rec, reuse=True)
    obs_a, obs_b = start(m, n, k, rows, 3), start(m, n, k, rows, 4)
    obs_b[0, 0, 4, 4] = obs_b[0, 1, 0, 0] = 1  # (row 0 of obs_a is empty: these two stones are not two plies on from it)
    obs_b[0, 0, 0, 1] = obs_b[0, 1, 8, 8] = 1
    for call, (obs, reset) in enumerate(((obs_a, False), (obs_a, True), (obs_b, False))):
        if reset:
            pol.reset_tree()
        del rec[:], rec0[:]
        plain = policy(hip, k, J, C, rec0)
        plain._sampler.calls = call
        got, want = gpu_act(pol, obs), gpu_act(plain, obs)
        same_leaves(rec, rec0, call)
        same(got, want, call)
        assert (got[1][2:].sum(axis=1) == J).all()
    # and the same position again does continue: the whole tree, J + 1 visits at its root
    got = gpu_act(pol, obs_b)
    assert (got[3][:, 1] == J + 1).all() and (got[1].sum(axis=1) == 2 * J).all()


# ----------------------------------------------------------------------------- 5. the roots' priors are renewed
def test_a_carried_root_takes_the_priors_of_evaluation_zero(hip):
    """an evaluator whose roots' call answers with other priors than its later calls on the same leaf: the rule (which
    replaces the carried root's priors and nothing else) is met bit for bit, and the sequence is not the one of an
    evaluator that answers the same every time"""
    board, rows, J = BOARDS[1]
    _, carried = run_sequence(hip, board, rows, J, 8, 1, refresh=True)
    assert (carried[1:, :, 0] > 1).any()
    m, n, k = board
    obs = start(m, n, k, rows, m * 100 + n * 10 + k + 1)
    acts = []
    for refresh in (False, True):
        rule = ReusePuct(k, J, C_PUCT, exact_np(m * n, J if refresh else None), None, SEED, ENV_ID0)
        rule.act(obs, step=0)
        acts.append(rule.act(obs, step=1)[1])
    assert not np.array_equal(*acts)


# ----------------------------------------------------------------------------- 6. dtypes
@pytest.mark.parametrize("dtype,leaf_dtype,out_dtype", [
    (torch.float32, torch.uint8, torch.bfloat16), (torch.bfloat16, torch.float32, torch.float32),
    (torch.uint8, torch.bfloat16, torch.bfloat16)])
def test_every_dtype_on_one_board(hip, dtype, leaf_dtype, out_dtype):
    board, rows, J = BOARDS[2]
    run_sequence(hip, board, rows, J, 6, 1, dtype=dtype, leaf_dtype=leaf_dtype, out_dtype=out_dtype)


# ----------------------------------------------------------------------------- 7. capture
def test_a_captured_act_replayed_equals_eager_acts(hip):
    """one eager act (the buffers, and a tree), the capture of one reusing act, three replays on the next three roots:
    the three eager acts of a second policy.  The draw's step is a device word, so that a replay draws as its eager twin"""
    (m, n, k), rows, J = BOARDS[2][0], 6, 16
    C = m * n
    rule = ReusePuct(k, J, C_PUCT, exact_np(C), None, SEED, ENV_ID0)
    roots, resets = [start(m, n, k, rows, 9)], np.zeros(rows, np.int64)
    for ply in range(4):
        want = rule.act(roots[-1], step=ply)
        roots.append(advance(roots[-1], want[0], k, 1, resets))

    def new():
        pol = policy(hip, k, J, C, reuse=True)
        pol._sampler.step_dev = torch.zeros(1, dtype=torch.int64, device=DEV)
        return pol

    eager, out = new(), []
    for ply in range(4):
        eager._sampler.step_dev.fill_(ply)
        out.append(gpu_act(eager, roots[ply]))
    assert any((o[3][:, 0] > 1).all() for o in out[1:])

    pol = new()
    obs = torch.from_numpy(roots[0]).to(DEV)
    visits = torch.zeros((rows, C), dtype=torch.int32, device=DEV)
    value, carried = torch.zeros(rows, device=DEV), torch.zeros((rows, 2), dtype=torch.int32, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pol.act({"observation": obs})  # ply 0, eager
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        actions = pol.act({"observation": obs}, visits=visits, root_value=value, carried=carried)
    for ply in range(1, 4):
        obs.copy_(torch.from_numpy(roots[ply]))
        pol._sampler.step_dev.fill_(ply)
        graph.replay()
        torch.cuda.synchronize()
        got = (actions.cpu().numpy(), visits.cpu().numpy(), value.cpu().numpy(), carried.cpu().numpy())
        same(got, out[ply], ("replay", ply))


# ----------------------------------------------------------------------------- 8. search self-play
@pytest.mark.parametrize("board,N,J,plies", [((3, 3, 3), 6, 10, 18), ((9, 9, 5), 5, 16, 6)])
def test_search_selfplay_with_reuse_equals_the_rule(hip, board, N, J, plies):
    from selfplay.search_selfplay import SearchSelfPlay

    m, n, k = board
    C, T, temp_plies, seed = m * n, m * n, 2, 13
    sp = SearchSelfPlay(m, n, k, N, evaluator=exact_torch(C), iterations=J, c=C_PUCT, temp_plies=temp_plies, capacity=T,
                        seed=seed, device=DEV, reuse=True)
    assert sp.policy.reuse and sp.policy.tree_nodes == 2 * J + 1
    sp.play(plies)
    rule, search = SelfPlayRule(m, n, k, N, T), ReusePuct(k, J, C_PUCT, exact_np(C), None, seed)
    obs, mask = rule.view()
    kept = 0
    for p in range(plies):
        _, visits, _, carried = search.act(obs, step=p)
        kept += int((carried[:, 0] > 1).sum())
        obs, mask = rule.step(visits, temp_plies, seed, p)
    assert kept and not rule.errors
    assert np.array_equal(sp.buffer.planes.cpu().numpy().view(np.uint64), rule.ring_planes)
    assert np.array_equal(sp.buffer.visits.cpu().numpy().view(np.uint16), rule.ring_visits)
    assert np.array_equal(sp.buffer.z.cpu().numpy(), rule.ring_z)
    assert np.array_equal(sp.obs.cpu().numpy(), obs) and np.array_equal(sp.mask.cpu().numpy(), mask)
    assert sp.stats.sum(dim=0)[:5].tolist() == rule.stats.tolist()
    if board == (3, 3, 3):
        assert rule.stats[0] >= N  # every game ended, was labelled and reset inside the run
    # reset_trees: the next ply searches every row afresh, as a ply of a policy without reuse would
    sp.reset_trees()
    carried = torch.full((N, 2), -1, dtype=torch.int32, device=DEV)
    sp.policy.act({"observation": sp.obs, "action_mask": sp.mask}, carried=carried)
    assert not carried.any()


# ----------------------------------------------------------------------------- 9. strength
REUSE_MIN = 0.35


def test_keeping_the_tree_does_not_weaken_the_player_on_9x9x5(hip):
    """PUCT(256) that keeps its tree against PUCT(256) that does not, both on the heuristic evaluator of
    tests/test_gpu_puct.py, 256 games (half as black).  Measured on the MI355X: 0.5137 (128 W / 7 D / 121 L; standard error
    0.031), the threshold 5 standard errors below.  (At 64 iterations the same match measured 0.4512, not above one half:
    no test there.  DESIGN section 3.13)"""
    from test_gpu_puct import heuristic_evaluator

    pol = hip.policy
    keeps = pol.PUCTSearchPolicy(5, evaluator=heuristic_evaluator(5), iterations=256, seed=14, reuse=True)
    fresh = pol.PUCTSearchPolicy(5, evaluator=heuristic_evaluator(5), iterations=256, seed=15)
    score = _score(hip, keeps, fresh, (9, 9, 5), 256)
    print("PUCT(256, reuse)-PUCT(256) %.4f" % score)
    assert score > REUSE_MIN, score
