"""GPU: the built-in kernel variants on EVERY board that reaches them.

The host dispatch matches a row of MNK_BUILTIN_BOARDS by (n, k, words per plane), never by m, so <1,3,3> also runs
4..8 x 3 x 3, <3,9,5> 7x9x5 and 8x9x5, <6,13,5> 12x13x5, <8,15,5> 16x15x5 and <12,19,5> 18x19x5 (tests/line_rule.py).  Such
a sibling board has no run-time compiled twin (mnk_jit_prepare returns early for a built-in geometry): nothing disagrees
with a wrong result there but the oracle and the numpy rules, so this module takes every kernel family to them -- the
win scan line by line (every line and every would-be wrap of the board, through env.step, wrapper.step and the tactical
sampler), the API kernels at ragged batch sizes into aligned and misaligned outputs, self-play, the fused rollout in
every form the board has, the row players -- bit for bit.  The row players are the Monte Carlo and UCT players, plain
PUCT, search self-play and its gather on 8x3x3, 7x9x5 and 16x15x5, and the later forms of the PUCT player on those
three and on 12x13x5 and 18x19x5: a kept tree (``mnk_puct_rebase``: sequences one and two plies on, the smallest
workspace and ``SearchSelfPlay(reuse=True)`` on 7x9x5), several leaves (L = 4 everywhere, 16 on the two small boards,
a kept tree and narrow dtypes), proofs (``mnk_puct_step_solver`` on batches with a board that fills inside the search
and a win in row m - 1), root noise on 7x9x5, the Gumbel root (the prep kernel, an act, two shards,
``mnk_search_selfplay_step_moves`` over more than a lap of the ring) and ``mnk_search_selfplay_advance`` (mixed budgets
round by round: 8x3x3 and 7x9x5 from the empty board; 7x9x5, 12x13x5, 16x15x5 and 18x19x5 from stored states with rows
that fill the board and are drawn at m * n stones; the lockstep form on 7x9x5).  What the siblings add to the square
boards: a plane that fills its last 32-bit word exactly (16x15 = 256 bits, 8x3 = 32), a cell count that differs from
the row's own (240 vs 225, 342 vs 361, 63 vs 81), output rows of odd byte sizes (504 B, 168 B, masks of 63 / 21 / 18 B)
and valid cells that stop before the variant's last row.

Which (board, form) pairs exist, from the source (csrc/mnk_rollout.hip, mnk_rollout_ws.hip, mnk_rollout_pairw.hip,
mnk_host.h) -- a pair that does not exist is not parametrised, nothing here skips:
  lane    one lane per env                          every board
  pair    two lanes per env, scan directions split  every row of MNK_BUILTIN_BOARDS
  pairw   two lanes per env, board words split      the k = 5 rows (widths 9, 13, 15, 19)
  ws2/ws4 waves per env group                       widths 9 and 19 only
  action log: BITS7 C <= 128 (lane form only), U8 C <= 256, U8P1 256 < C <= 512, U16 always
"""
import os

import numpy as np
import pytest
import torch

import line_rule as lr
import test_gpu_draw_exact as de
import test_gpu_env as ge
import test_gpu_fused_draw as fd
import test_gpu_fuzz as fz
import test_gpu_playout as gpl
import test_gpu_puct as gpu
import test_gpu_puct_gumbel as ggu
import test_gpu_puct_leaves as gle
import test_gpu_puct_noise as gno
import test_gpu_puct_reuse as gre
import test_gpu_puct_solver as gso
import test_gpu_search_selfplay_async as gas
import test_gpu_search as gse
import test_gpu_search_selfplay as gss
import test_gpu_selfplay as gsp
import test_gpu_sink as gsk
import test_gpu_tactical as gta
from oracle import philox
from oracle.env_torch import OracleVectorEnv
from oracle.packing import pack_boards
from oracle.policies import LowestLegalPolicy
from oracle.rollout import decode_action_log, random_rollout
from replay import golden_files, replay_env_log, replay_selfplay_trace
from search_selfplay_rule import sym_ok
from tactical_rule import completions, tactical_sets

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OBS_DTYPES = (torch.float32, torch.bfloat16, torch.uint8)

SIBLINGS = lr.sibling_boards(square=False)     # 4..8 x 3 x 3, 7x9x5, 8x9x5, 12x13x5, 16x15x5, 18x19x5
SQUARES = lr.sibling_boards(non_square=False)  # the boards the rows are named after: controls
CONTROL = (7, 9, 7)                            # off the list: <3,9,5> for the kernels that never look at k, run-time compiled otherwise
PLAYER_BOARDS = [(8, 3, 3), (7, 9, 5), (16, 15, 5)]
WIDE = [(12, 13, 5), (18, 19, 5)]              # the <6,13,5> and <12,19,5> variants for the later forms of the PUCT player
FORMS = {"lane": "one lane per env", "pair": "two lanes per env", "pairw": "two lanes per env, words split",
         "ws2": "two waves per env group", "ws4": "four waves per env group"}


def forms_of(board):
    m, n, k = board
    return ["lane", "pair"] + (["pairw"] if k == 5 else []) + (["ws2", "ws4"] if n in (9, 19) else [])


BOARD_FORMS = [(b, f) for b in SIBLINGS for f in forms_of(b)]


def _id(v):
    return "x".join(str(x) for x in v) if isinstance(v, tuple) else None


@pytest.fixture(scope="module")
def hip():
    """the union of what the modules whose helpers run here take from their own ``hip`` fixtures"""
    import __graft_entry__ as entry

    entry.build_hip()
    entry._ensure_path()
    import mnk_hip
    from alg.packed_rollout_buffer import PackedRolloutBuffer
    from alg.rollout_buffer import RolloutBuffer
    from env.torch_vector_mnk_env import TorchVectorMnkEnv
    from selfplay import graphed, policy, random_rollout as rr, tournament, validation
    from selfplay.torch_self_play_wrapper import TorchSelfPlayWrapper

    mnk_hip.load()
    assert torch.cuda.is_available()

    class NS:
        pass

    ns = NS()
    ns.lib, ns.Env, ns.Wrapper, ns.policy, ns.graphed = mnk_hip, TorchVectorMnkEnv, TorchSelfPlayWrapper, policy, graphed
    ns.validation, ns.tournament, ns.Buffer, ns.PackedBuffer = validation, tournament, RolloutBuffer, PackedRolloutBuffer
    ns.rollout, ns.Rollout = rr, rr.RandomRollout
    return ns


@pytest.fixture(scope="module")
def builtin_only(hip):
    """Proof that the built-in variants run: with MNK_JIT_API=1 (compile a board's own kernel at its first launch) for
    the whole module, ``jit_prepare`` has nothing to prepare on any board of the matrix and compiles one for a board off
    the list; the number of programs compiled is then held after every test of the module."""
    lib = hip.lib
    saved = {key: os.environ.get(key) for key in ("MNK_JIT_API", "MNK_JIT")}
    os.environ.pop("MNK_JIT", None)
    os.environ["MNK_JIT_API"] = "1"
    lib.reload_config()
    for m, n, k in SIBLINGS + SQUARES:
        assert lib.jit_prepare(m, n, k, [lib.JIT_API_STEP]) == 0, (m, n, k)
        assert not lib.jit_api_ready(m, n, k, lib.JIT_API_STEP)
    assert lib.jit_prepare(*CONTROL, [lib.JIT_API_STEP]) >= 1, lib.load().mnk_jit_last_error()
    state = {"compiled": lib.jit_stats()["compiled"] + lib.jit_stats()["cache_hits"]}
    assert state["compiled"] >= 1
    yield state
    for key, val in saved.items():
        if val is None:
            os.environ.pop(key, None)
        else:
            os.environ[key] = val
    lib.reload_config()


@pytest.fixture(autouse=True)
def nothing_compiled(hip, builtin_only):
    yield
    stats = hip.lib.jit_stats()
    assert stats["compiled"] + stats["cache_hits"] == builtin_only["compiled"], "a sibling board ran a run-time compiled kernel"
    assert stats["failed"] == 0


def test_every_matrix_board_takes_a_built_in_variant(hip, builtin_only):
    """(the fixture has asserted it; this is the case that shows in the log) -- and the table of the boards itself"""
    assert {(7, 9, 5), (8, 9, 5), (4, 3, 3), (5, 3, 3), (6, 3, 3), (7, 3, 3), (8, 3, 3), (12, 13, 5), (16, 15, 5),
            (18, 19, 5)} <= set(SIBLINGS)
    assert {(9, 9, 5), (3, 3, 3), (13, 13, 5), (15, 15, 5), (19, 19, 5)} <= set(SQUARES)
    for m, n, k in SIBLINGS + SQUARES:
        for kind in range(hip.lib.JIT_API_COUNT):
            assert not hip.lib.jit_api_ready(m, n, k, kind), (m, n, k, kind)
    assert hip.lib.jit_api_ready(*CONTROL, hip.lib.JIT_API_STEP)


# ----------------------------------------------------------------------------- helpers
def poke(target, boards, side, counts):
    """the same hand-made state into a HIP env or the oracle"""
    if isinstance(target, OracleVectorEnv):
        target.boards.copy_(torch.from_numpy(boards))
        target.current_player.copy_(torch.from_numpy(side))
        target.move_counts.copy_(torch.from_numpy(counts))
    else:
        target.boards = torch.from_numpy(boards)
        target.current_player = torch.from_numpy(side)
        target.move_counts = torch.from_numpy(counts)


def same_step(hip_out, ora_out, env, ora, where):
    (o1, r1, d1), (o2, r2, d2) = hip_out, ora_out
    assert torch.equal(r1.cpu(), r2), f"{where}: rewards"
    assert torch.equal(d1.cpu(), d2), f"{where}: dones"
    assert torch.equal(o1["observation"].float().cpu(), o2["observation"]), f"{where}: observation"
    assert torch.equal(o1["action_mask"].cpu(), o2["action_mask"]), f"{where}: mask"
    same_state(env, ora, where)


def same_state(env, ora, where):
    assert torch.equal(env.boards[...].cpu(), ora.boards), f"{where}: boards"
    assert torch.equal(env.current_player.cpu(), ora.current_player), f"{where}: current_player"
    assert torch.equal(env.move_counts.cpu(), ora.move_counts), f"{where}: move_counts"


_BITS = {torch.float32: (torch.int32, {0, 0x3F800000}), torch.bfloat16: (torch.int16, {0, 0x3F80}), torch.uint8: (torch.uint8, {0, 1})}


def exactly_zero_or_one(obs):
    """every element is +0 or 1 of its dtype, as bit patterns (a -0.0 or a 1 with a stray mantissa bit compares equal
    to nothing here)"""
    view, allowed = _BITS[obs.dtype]
    seen = set(torch.unique(obs.contiguous().view(view)).cpu().tolist())
    assert seen <= allowed, (obs.dtype, sorted(seen)[:8])


def out_tensor(shape, dtype, offset):
    """a contiguous device tensor, base-aligned, or one element past the allocation's base (the non-vector store path)"""
    count = int(np.prod(shape))
    if not offset:
        t = torch.empty(shape, dtype=dtype, device=DEV)
    else:
        t = torch.empty(count + 1, dtype=dtype, device=DEV)[1:].view(shape)
        assert t.data_ptr() % 16 != 0 or count == 0
    if count:
        t.fill_(True if dtype == torch.bool else 77)  # (neither 0 nor 1: a cell the kernel leaves out shows)
    return t


def filler(m, n):
    """cells of two colours with no run longer than two of either in any of the four directions: (r + 2c) mod 4 < 2"""
    r, c = np.divmod(np.arange(m * n), n)
    return ((r + 2 * c) % 4 < 2).reshape(m, n)


def line_cases_for_step(m, n, k, side):
    """one env per line / wrap: the mover has all of its cells but the last, which is the move"""
    cs = lr.cases(m, n, k)
    boards = np.zeros((len(cs), 2, m, n), dtype=np.float32)
    acts = np.zeros(len(cs), dtype=np.int64)
    for i, (cells, _) in enumerate(cs):
        boards[i, side] = lr.plane_of(cells[:-1], m, n)
        acts[i] = cells[-1]
    want = np.array([w for _, w in cs])
    return boards, acts, want


def opponent_win_cases(m, n, k):
    """one env per line / wrap for ``wrapper.step`` with the agent black and a lowest-legal opponent: white holds every
    cell of the line but its lowest, x; every cell below x is taken (the two-colour filler: no run of three) but for the
    agent's own move when that lies there, so after the agent has moved the lowest legal cell IS the completing one.  The
    agent's move is the highest cell off the line that gives black no line.  Returns (boards, agent moves, opponent
    cells, wins)."""
    cs = lr.cases(m, n, k)
    fill = filler(m, n).reshape(-1)
    boards = np.zeros((len(cs), 2, m * n), dtype=np.float32)
    acts = np.zeros(len(cs), dtype=np.int64)
    reply = np.zeros(len(cs), dtype=np.int64)
    for i, (cells, _) in enumerate(cs):
        x = min(cells)
        below = np.arange(x)
        rest = [c for c in cells if c != x]
        for a in range(m * n - 1, -1, -1):
            if a in cells:
                continue
            boards[i] = 0.0
            boards[i, 0, below[fill[below]]] = 1.0
            boards[i, 1, below[~fill[below]]] = 1.0
            boards[i, :, a] = 0.0
            boards[i, 1, rest] = 1.0
            boards[i, 0, rest] = 0.0
            trial = boards[i, 0].copy()
            trial[a] = 1.0
            if not lr.has_line(trial.reshape(m, n), k):
                acts[i] = a
                break
        else:
            raise AssertionError(f"no quiet agent move for {cells} on {m}x{n}x{k}")
        reply[i] = x
    want = np.array([w for _, w in cs])
    return boards.reshape(len(cs), 2, m, n), acts, reply, want


# ----------------------------------------------------------------------------- 1. every line and every wrap
@pytest.mark.parametrize("board", SIBLINGS + SQUARES, ids=_id)
def test_every_line_wins_and_no_wrap_does_through_env_step(hip, board):
    """``env.step`` on poked states, black and white as the mover, one env per line / wrap of the board: the completing
    move wins on every line and on no wrap (the brute-force rule), and rewards, flags, observation, mask and state equal
    the oracle's"""
    m, n, k = board
    for side in (0, 1):
        boards, acts, want = line_cases_for_step(m, n, k, side)
        nenv = len(acts)
        env, ora = hip.Env(m, n, k, nenv, device=DEV), OracleVectorEnv(m, n, k, nenv)
        sides = np.full(nenv, side, dtype=np.int64)
        counts = np.full(nenv, k - 1, dtype=np.int64)
        poke(env, boards, sides, counts)
        poke(ora, boards, sides, counts)
        same_state(env, ora, f"{board} side {side} poke")
        out = env.step(torch.from_numpy(acts).to(DEV))
        exactly_zero_or_one(out[0]["observation"])
        same_step(out, ora.step(torch.from_numpy(acts)), env, ora, f"{board} side {side}")
        got = out[2].cpu().numpy()
        wrong = np.flatnonzero(got != want)
        assert wrong.size == 0, (board, side, [lr.cases(m, n, k)[i] for i in wrong[:4]])
        assert np.array_equal(out[1].cpu().numpy(), want.astype(np.float32))
        env.check_errors()


@pytest.mark.parametrize("board", SIBLINGS + SQUARES, ids=_id)
def test_every_line_through_the_wrapper_for_the_agent_and_for_the_opponent(hip, board):
    """``wrapper.step`` (pre + post kernels, a scripted lowest-legal opponent): the agent completes the line / wrap
    itself (+1, terminated on the lines), and the opponent completes it with its reply (-1, terminated) -- against the
    oracle wrapper on the same poked states"""
    m, n, k = board
    a_boards, a_acts, want = line_cases_for_step(m, n, k, 0)
    o_boards, o_acts, reply, want_o = opponent_win_cases(m, n, k)
    assert np.array_equal(want, want_o)
    for name, boards, acts in (("agent", a_boards, a_acts), ("opponent", o_boards, o_acts)):
        nenv = len(acts)
        wrap = hip.Wrapper(hip.Env(m, n, k, nenv, device=DEV), seed=3)
        ora = fz._ForcedSides(OracleVectorEnv(m, n, k, nenv))
        sides = torch.zeros(nenv, dtype=torch.long)
        wrap.force_sides(sides)
        ora.sides = sides
        wrap.set_opponent(LowestLegalPolicy())
        ora.set_opponent(LowestLegalPolicy())
        wrap.reset()
        ora.reset()
        stones = boards.reshape(nenv, -1).sum(axis=1).astype(np.int64)
        poke(wrap.env, boards, np.zeros(nenv, dtype=np.int64), stones)
        poke(ora.env, boards, np.zeros(nenv, dtype=np.int64), stones)
        o1, r1, t1, tr1, _ = wrap.step(torch.from_numpy(acts).to(DEV))
        o2, r2, t2, _, _ = ora.step(torch.from_numpy(acts))
        where = f"{board} {name} win"
        exactly_zero_or_one(o1["observation"])
        assert torch.equal(r1.cpu(), r2) and torch.equal(t1.cpu(), t2) and not bool(tr1.any()), where
        assert torch.equal(o1["observation"].cpu(), o2["observation"]) and torch.equal(o1["action_mask"].cpu(), o2["action_mask"]), where
        assert torch.equal(wrap.pending_resets.cpu(), ora.pending_resets), where
        same_state(wrap.env, ora.env, where)
        rew = r1.cpu().numpy()
        if name == "agent":
            assert np.array_equal(t1.cpu().numpy()[want], np.ones(int(want.sum()), bool)), where
            assert np.array_equal(rew[want], np.ones(int(want.sum()), np.float32)), where
            assert not (rew[~want] > 0).any(), where
        else:
            white = o1["observation"].cpu().numpy()[:, 1].reshape(nenv, -1)  # (the finished game stands until the next step)
            assert white[np.arange(nenv), reply].all(), where                 # the reply went to the lowest legal cell
            assert np.array_equal(rew[want], -np.ones(int(want.sum()), np.float32)) and t1.cpu().numpy()[want].all(), where
        wrap.env.check_errors()


@pytest.mark.parametrize("board", SIBLINGS + SQUARES, ids=_id)
def test_the_tactical_sampler_completes_every_line_from_every_gap(hip, board):
    """every line with each of its k cells left empty, the rest the mover's: ``mnk_sample_tactical`` offers exactly the
    completions of the numpy rule and takes the completing cell where it is the only one; the same stones given to the
    other side are blocked at the same cells"""
    m, n, k = board
    rows, gaps = [], []
    for cells in lr.lines(m, n, k):
        for gap in cells:
            rows.append(lr.plane_of([c for c in cells if c != gap], m, n))
            gaps.append(gap)
    planes = np.stack(rows)
    gaps = np.array(gaps)
    win = completions(planes != 0, planes == 0, k).reshape(len(gaps), -1)
    assert win[np.arange(len(gaps)), gaps].all()
    only = win.sum(axis=1) == 1
    assert only.any()
    for mine in (0, 1):  # the stones are the mover's (take the win) / the other side's (block it)
        obs = np.zeros((len(gaps), 2, m, n), dtype=np.float32)
        obs[:, mine] = planes
        s, w, b = tactical_sets(obs, k)
        assert np.array_equal(w if mine == 0 else b, win) and np.array_equal(s, win)
        for dtype in OBS_DTYPES:
            for det in (False, True):
                pol = hip.policy.TacticalPolicy(k, seed=11)
                cand = torch.full((len(gaps), m * n), 7, dtype=torch.uint8, device=DEV)
                acts = pol.act({"observation": torch.from_numpy(obs).to(DEV).to(dtype)}, deterministic=det, candidates=cand)
                acts = acts.cpu().numpy()
                assert np.array_equal(cand.cpu().numpy(), win.astype(np.uint8)), (board, mine, dtype, det)
                assert np.array_equal(acts[only], gaps[only]), (board, mine, dtype, det)
                assert win[np.arange(len(gaps)), acts].all()
                x = 0 if det else philox.rand_u32(11, np.arange(len(gaps), dtype=np.uint64), 0, philox.STREAM_SAMPLE)
                assert np.array_equal(acts, philox.pick_legal(win, np.broadcast_to(np.asarray(x, dtype=np.uint64), (len(gaps),))))


# ----------------------------------------------------------------------------- 2. the API kernels
def _random_state(m, n, k, nenv, rng):
    """positions of random density with both stones on some cells, a full and an empty board among them"""
    fill = rng.random((nenv, 1, 1, 1)) * 0.9
    dense = (rng.random((nenv, 2, m, n)) < fill * 0.5).astype(np.float32)
    dense[0] = 1.0
    if nenv > 1:
        dense[1] = 0.0
    return dense, rng.integers(0, 2, nenv), rng.integers(0, m * n, nenv)


@pytest.mark.parametrize("nenv", [1, 67, 129, 1000])
@pytest.mark.parametrize("board", SIBLINGS, ids=_id)
def test_api_kernels_at_ragged_batches_into_aligned_and_offset_outputs(hip, board, nenv):
    """step, step_subset over a random ascending subset, reset(idx), observe (f32 / bf16 / u8, absolute and flipped),
    sample_legal and the one-launch random step on poked mid-game states: == the oracle after every call, written into
    base-aligned tensors and into views one element past the base; observation elements are exactly 0 or 1"""
    m, n, k = board
    c = m * n
    rng = np.random.default_rng(1000 * m + 10 * n + nenv)
    env, ora = hip.Env(m, n, k, nenv, device=DEV), OracleVectorEnv(m, n, k, nenv)
    dense, side, counts = _random_state(m, n, k, nenv, rng)
    poke(env, dense, side, counts)
    poke(ora, dense, side, counts)
    for offset in (0, 1):
        where = f"{board} N={nenv} offset {offset}"
        # observe: every dtype, absolute and canonical
        want = ora.observe()
        flip = torch.from_numpy(rng.integers(0, 2, nenv)).to(DEV)
        for dtype in OBS_DTYPES:
            obs, mask = out_tensor((nenv, 2, m, n), dtype, offset), out_tensor((nenv, c), torch.bool, offset)
            env.observe_into(obs, mask)
            exactly_zero_or_one(obs)
            assert torch.equal(obs.float().cpu(), want["observation"]) and torch.equal(mask.cpu(), want["action_mask"]), (where, dtype)
            obs2, mask2 = out_tensor((nenv, 2, m, n), dtype, offset), out_tensor((nenv, c), torch.bool, offset)
            env.observe_into(obs2, mask2, flip_side=flip, fix_empty_mask=True)
            exactly_zero_or_one(obs2)
            canon = torch.where((flip.cpu() == 1).view(-1, 1, 1, 1), want["observation"].flip(1), want["observation"])
            fixed = want["action_mask"].clone()
            fixed[fixed.sum(dim=1) == 0, 0] = True
            assert torch.equal(obs2.float().cpu(), canon) and torch.equal(mask2.cpu(), fixed), (where, dtype, "canonical")
        # sample_legal: the oracle's Philox draw over the oracle's mask
        acts = out_tensor((nenv,), torch.int64, offset)
        env.sample_legal_into(acts, seed=5, step=7 + offset, env_id0=900)
        x = philox.rand_u32(5, np.arange(900, 900 + nenv, dtype=np.uint64), 7 + offset, philox.STREAM_MOVE)
        assert np.array_equal(acts.cpu().numpy(), philox.pick_legal(want["action_mask"].numpy(), x)), where
        # step into caller-owned outputs of every dtype (legal, occupied and negative actions)
        a = rng.integers(-c, c, nenv)
        legal = want["action_mask"].numpy()
        for i in range(nenv):
            if legal[i].any() and rng.random() < 0.7:
                a[i] = rng.choice(np.flatnonzero(legal[i]))
        dtype = OBS_DTYPES[(offset + nenv) % 3]
        obs, mask = out_tensor((nenv, 2, m, n), dtype, offset), out_tensor((nenv, c), torch.bool, offset)
        rew, done = out_tensor((nenv,), torch.float32, offset), out_tensor((nenv,), torch.bool, offset)
        env.step_into(torch.from_numpy(a).to(DEV), rew, done, mask, obs)
        exactly_zero_or_one(obs)
        same_step(({"observation": obs, "action_mask": mask}, rew, done), ora.step(torch.from_numpy(a)), env, ora, where + " step")
        # step_subset over a random ascending subset
        pick = rng.random(nenv) < 0.5
        pick[rng.integers(0, nenv)] = True
        idx = torch.from_numpy(np.flatnonzero(pick))
        sub = torch.from_numpy(rng.integers(0, c, int(pick.sum())))
        out = env.step_subset(sub.to(DEV), idx.to(DEV))
        exactly_zero_or_one(out[0]["observation"])
        same_step(out, ora.step_subset(sub, idx), env, ora, where + " step_subset")
        # reset(idx)
        ridx = torch.from_numpy(np.flatnonzero(rng.random(nenv) < 0.3))
        o1, o2 = env.reset(ridx.to(DEV)), ora.reset(ridx)
        assert torch.equal(o1["observation"].cpu(), o2["observation"]) and torch.equal(o1["action_mask"].cpu(), o2["action_mask"]), where
        same_state(env, ora, where + " reset(idx)")
        # mnk_step_random: draw, step, restart, observe in one launch
        for dtype in OBS_DTYPES:
            obs, mask = out_tensor((nenv, 2, m, n), dtype, offset), out_tensor((nenv, c), torch.bool, offset)
            rew, done = out_tensor((nenv,), torch.float32, offset), out_tensor((nenv,), torch.bool, offset)
            played = out_tensor((nenv,), torch.int64, offset)
            before = ora.observe()["action_mask"].numpy()
            env.step_random_into(rew, done, mask, obs, played, seed=41, step=3, env_id0=77)
            x = philox.rand_u32(41, np.arange(77, 77 + nenv, dtype=np.uint64), 3, philox.STREAM_MOVE)
            moves = philox.pick_legal(before, x)
            assert np.array_equal(played.cpu().numpy(), moves), (where, "step_random draw")
            _, r2, d2 = ora.step(torch.from_numpy(moves))
            if bool(d2.any()):
                ora.reset(torch.nonzero(d2).squeeze(1))
            exactly_zero_or_one(obs)
            same_step(({"observation": obs, "action_mask": mask}, rew, done), (ora.observe(), r2, d2), env, ora, where + " step_random")
    env.check_errors()


@pytest.mark.parametrize("board", [(7, 9, 5), (16, 15, 5)], ids=_id)
def test_api_kernels_at_forty_thousand_envs(hip, board):
    """the other ``mnk_block_envs`` setting (64 envs per workgroup above 32 768 items), once: observe, step, the random
    step"""
    m, n, k = board
    nenv, c = 40000, m * n
    rng = np.random.default_rng(m)
    env, ora = hip.Env(m, n, k, nenv, device=DEV), OracleVectorEnv(m, n, k, nenv)
    dense, side, counts = _random_state(m, n, k, nenv, rng)
    poke(env, dense, side, counts)
    poke(ora, dense, side, counts)
    for dtype in OBS_DTYPES:
        obs, mask = out_tensor((nenv, 2, m, n), dtype, 1), out_tensor((nenv, c), torch.bool, 1)
        env.observe_into(obs, mask)
        exactly_zero_or_one(obs)
        want = ora.observe()
        assert torch.equal(obs.float().cpu(), want["observation"]) and torch.equal(mask.cpu(), want["action_mask"]), dtype
    a = torch.from_numpy(rng.integers(-c, c, nenv))
    out = env.step(a.to(DEV))
    exactly_zero_or_one(out[0]["observation"])
    same_step(out, ora.step(a), env, ora, f"{board} step")
    rew, done = torch.empty(nenv, device=DEV), torch.empty(nenv, dtype=torch.bool, device=DEV)
    mask, played = torch.empty((nenv, c), dtype=torch.bool, device=DEV), torch.empty(nenv, dtype=torch.long, device=DEV)
    before = ora.observe()["action_mask"].numpy()
    env.step_random_into(rew, done, mask, actions=played, seed=2, step=5)
    moves = philox.pick_legal(before, philox.rand_u32(2, np.arange(nenv, dtype=np.uint64), 5, philox.STREAM_MOVE))
    assert np.array_equal(played.cpu().numpy(), moves)
    _, r2, d2 = ora.step(torch.from_numpy(moves))
    ora.reset(torch.nonzero(d2).squeeze(1))
    assert torch.equal(rew.cpu(), r2) and torch.equal(done.cpu(), d2) and torch.equal(mask.cpu(), ora.observe()["action_mask"])
    same_state(env, ora, f"{board} step_random")


@pytest.mark.parametrize("board", SIBLINGS, ids=_id)
def test_sample_legal_reaches_every_cell_every_rank_and_the_last_word(hip, board):
    """the construction of test_gpu_env.py (one env per cell with only that cell free; free cells round the word
    boundaries of the bit string) on the sibling, and the same with exactly the cells of the TOP word free -- on 16x15
    and 8x3 a word whose last bit is the last row's guard bit -- where every rank of the select must come out"""
    m, n, k = board
    ge.test_sample_legal_reaches_every_cell_and_every_rank(hip, m, n, k)
    cells = lr.last_word_cells(m, n)
    assert cells and cells[-1] == m * n - 1
    nenv = 4096
    taken = np.ones(m * n, dtype=np.float32)
    taken[cells] = 0.0
    dense = np.zeros((nenv, 2, m, n), dtype=np.float32)
    dense[:, 0] = taken.reshape(m, n)
    env = hip.Env(m, n, k, nenv, device=DEV)
    env.boards = torch.from_numpy(dense)
    acts = torch.empty(nenv, dtype=torch.int64, device=DEV)
    env.sample_legal_into(acts, seed=3, step=4, env_id0=50, stream_id=0)
    legal = ~(dense != 0).any(axis=1).reshape(nenv, m * n)
    got = acts.cpu().numpy()
    assert np.array_equal(got, philox.pick_legal(legal, philox.rand_u32(3, np.arange(50, 50 + nenv, dtype=np.uint64), 4, 0)))
    assert sorted(set(got.tolist())) == cells


@pytest.mark.parametrize("board", SIBLINGS, ids=_id)
def test_records_unpack_and_minibatches_gather(hip, board):
    """``mnk_unpack_records`` against numpy (test_gpu_selfplay.py's comparison) at a ragged batch, its narrow forms, and
    ``mnk_gather_obs`` of packed canonical planes against the dense observations they were packed from, every dtype,
    into aligned and offset outputs"""
    m, n, k = board
    c = m * n
    for nenv, steps in ((67, 9), (129, 4)):
        gsp.test_unpack_records_matches_numpy(hip, m, n, k, nenv, steps)
    nenv, t = 129, 3
    env = hip.Env(m, n, k, nenv, device=DEV)
    roll = hip.Rollout(env, seed=8)
    roll.run(max(4, c // 3), record=False)
    rec = roll.run(8)
    want = hip.rollout.unpack_records(rec, env)
    exactly_zero_or_one(want["observations"])
    for dtype in OBS_DTYPES[1:]:
        got = hip.rollout.unpack_records(rec, env, obs_dtype=dtype)
        exactly_zero_or_one(got["observations"])
        assert torch.equal(got["observations"].float(), want["observations"])
        assert all(torch.equal(got[key], want[key]) for key in ("action_masks", "actions", "rewards", "dones"))
    buf = hip.PackedBuffer(t, nenv, m, n, device=DEV)
    wrap = hip.Wrapper(env, seed=1)
    wrap.agent_side.copy_(torch.from_numpy(np.random.default_rng(c).integers(0, 2, nenv)).to(DEV))
    dense, masks = [], []
    ora = OracleVectorEnv(m, n, k, nenv)
    for j in range(t):
        buf.planes[j].copy_(wrap.packed_obs())
        ora.boards.copy_(env.boards[...].cpu())
        o = ora.observe()
        flip = (wrap.agent_side.cpu() == 1).view(-1, 1, 1, 1)
        dense.append(torch.where(flip, o["observation"].flip(1), o["observation"]))
        masks.append(o["action_mask"])
        roll.run(3, record=False)
    dense, masks = torch.cat(dense), torch.cat(masks)
    idx = torch.randperm(t * nenv, generator=torch.Generator().manual_seed(1))[:301]
    for dtype in OBS_DTYPES:
        for offset in (0, 1):
            obs, mask = out_tensor((len(idx), 2, m, n), dtype, offset), out_tensor((len(idx), c), torch.bool, offset)
            idx_t = idx.to(DEV)
            hip.lib.call("mnk_gather_obs", hip.lib.ptr(buf.planes), t, nenv, m, n, hip.lib.ptr(idx_t), len(idx), hip.lib.ptr(obs),
                         hip.lib.obs_code(obs), hip.lib.ptr(mask), 0, None, hip.lib.stream_ptr(DEV))
            exactly_zero_or_one(obs)
            assert torch.equal(obs.float().cpu(), dense[idx]) and torch.equal(mask.cpu(), masks[idx]), (board, dtype, offset)


# ----------------------------------------------------------------------------- 3. recorded from the reference
def test_reference_fixtures_of_the_sibling_boards(hip, golden_dir):
    """``make_golden.py --sibling-boards``: what the imported reference recorded on 8x3x3, 7x9x5, 16x15x5 and 18x19x5
    (env op-logs with subset steps and resets, wrapper traces with lowest / hash / highest opponents), replayed on the
    HIP env and wrapper with f32 and narrow observations"""
    envs, traces = golden_files(golden_dir, "siblings_env_"), golden_files(golden_dir, "siblings_selfplay_")
    assert len(envs) == 4 and len(traces) == 4
    for j, path in enumerate(envs):
        log = np.load(path)
        m, n, k, nenv, _ = (int(v) for v in log["geom"])
        assert (m, n, k) in SIBLINGS
        replay_env_log(hip.Env(m, n, k, nenv, device=DEV), log)
        replay_env_log(hip.Env(m, n, k, nenv, device=DEV, obs_dtype=OBS_DTYPES[1 + j % 2]), log)
    for j, path in enumerate(traces):
        log = np.load(path)
        m, n, k, nenv, _ = (int(v) for v in log["geom"])
        for dtype in (torch.float32, OBS_DTYPES[1 + j % 2]):
            wrap = hip.Wrapper(hip.Env(m, n, k, nenv, device=DEV, obs_dtype=dtype))
            wrap.set_opponent(gsp.OPP[path.split("_")[-2]]())
            replay_selfplay_trace(wrap, log, lambda w, sides: w.force_sides(torch.from_numpy(sides.astype(np.int64))))


# ----------------------------------------------------------------------------- 4. self-play
@pytest.mark.parametrize("board", SIBLINGS, ids=_id)
def test_wrapper_with_scripted_opponents_against_the_oracle(hip, board, monkeypatch):
    """the differential fuzzers of test_gpu_fuzz.py pinned to the sibling: every env operation; the wrapper with a
    lowest-legal / highest-legal / hash opponent handing out f32 / bf16 / u8 observations, forced sides, caller-owned
    outputs and a third of its steps through ``step_logits`` (two launches here: the folded draw declines a non-square
    board); the rollout with a random log format, replays and one-launch plies"""
    monkeypatch.setattr(fz, "_shape", lambda rng: board)
    fz._MAX_WRAPPER_STEPS[0] = 60
    try:
        base = 300 + 3 * SIBLINGS.index(board)
        for seed in (base, base + 1, base + 2):  # seed % 3: the opponent and the observation dtype
            fz.test_wrapper_fuzz(hip, seed)
        fz.test_env_fuzz(hip, base)
        fz.test_rollout_and_log_fuzz(hip, base)
    finally:
        fz._MAX_WRAPPER_STEPS[0] = 10 ** 9


@pytest.mark.parametrize("board", SIBLINGS, ids=_id)
def test_one_launch_self_play_steps_against_the_oracle(hip, board):
    """``mnk_selfplay_step_random`` (the Philox opponent inside the step) and ``mnk_selfplay_step_tactical`` with
    actions and with logits, against ``OracleSelfPlay`` with the same opponents, at a ragged batch"""
    m, n, k = board
    steps = min(2 * m * n, 70)
    gsp.test_fused_random_opponent_step_matches_oracle(hip, m, n, k, 67, steps)
    gta.run_against_oracle(hip, m, n, k, 67, min(steps, 40), False)
    gta.run_against_oracle(hip, m, n, k, 67, min(steps, 40), True)
    gta.test_actions_equal_the_numpy_rule_on_fuzzed_positions(hip, board)


@pytest.mark.parametrize("board", SIBLINGS, ids=_id)
def test_the_sink_and_the_packed_planes(hip, board):
    """``attach_sink`` with a buffer of each observation dtype (the step kernels write rows of the buffer: == the same
    run into fresh tensors), the narrow observations of every kernel against the f32 ones, and the packed canonical
    planes of the step kernels, one launch and two"""
    m, n, k = board
    c, nenv, steps = m * n, 129, 6
    gsk.test_narrow_observations_equal_the_f32_ones(hip, m, n, k, 67, torch.bfloat16)
    gsk.test_narrow_observations_equal_the_f32_ones(hip, m, n, k, 129, torch.uint8)
    for fused in (True, False):
        gsk.test_step_kernels_emit_the_packed_canonical_planes(hip, m, n, k, 67, fused)
    for dtype in OBS_DTYPES:
        for fused in (True, False):
            def build():
                w = hip.Wrapper(hip.Env(m, n, k, nenv, device=DEV, obs_dtype=dtype), seed=3)
                w.set_opponent(hip.policy.RandomPolicy(c, seed=2) if fused else LowestLegalPolicy())
                return w, hip.policy.RandomPolicy(c, seed=5)

            (plain, agent_a), (sunk, agent_b) = build(), build()
            buf = hip.Buffer(steps, nenv, (2, m, n), c, device=DEV, obs_dtype=dtype)
            sunk.attach_sink(buf)
            oa, _ = plain.reset()
            ob, _ = sunk.reset()
            assert ob["observation"].data_ptr() == buf.observations[0].data_ptr() and ob["observation"].dtype == dtype
            zeros = torch.zeros(nenv, device=DEV)
            for t in range(steps):
                exactly_zero_or_one(ob["observation"])
                assert torch.equal(oa["observation"], ob["observation"]) and torch.equal(oa["action_mask"], ob["action_mask"]), (dtype, fused, t)
                acts = agent_a.act(oa)
                assert torch.equal(acts, agent_b.act(ob))
                oa, ra, ta, _, _ = plain.step(acts)
                nxt, rb, tb, trb, _ = sunk.step(acts)
                assert rb.data_ptr() == buf.rewards[t].data_ptr() and tb.data_ptr() == buf.dones[t].data_ptr()
                assert torch.equal(ra, rb) and torch.equal(ta, tb), (dtype, fused, t)
                buf.add(ob["observation"], acts, rb, zeros.view(-1, 1), zeros, tb | trb, ob["action_mask"])
                ob = nxt
            assert torch.equal(oa["observation"], ob["observation"]) and torch.equal(plain.env._planes, sunk.env._planes)
            assert buf.copied_bytes == steps * nenv * (8 + 4 + 4 + 1)
            exactly_zero_or_one(buf.observations)


STEP_LOGITS = [(b, o) for b in SIBLINGS for o in ("random", "scripted")] + [(b, "net") for b in PLAYER_BOARDS]


@pytest.mark.parametrize("board,opponent", STEP_LOGITS, ids=[f"{_id(b)}-{o}" for b, o in STEP_LOGITS])
def test_step_logits_declines_the_fold_and_equals_draw_then_step(hip, board, opponent):
    """``wrapper.step_logits`` with f32, bf16 and absent logits on a non-square sibling: the row's compile-time draw
    shape is the SQUARE board's cell count (81 for a 63-cell board), so ``mnk_launch_sp_fused`` must decline and the call
    takes two launches (a network opponent's draw in ``post`` likewise: the three boards of the row players) -- the
    result equals ``HipSampler.draw`` followed by ``wrapper.step``, nothing was compiled for
    the draw kinds, and every draw is the float64 inverse CDF of its row (tests/draw_rule.py)"""
    m, n, k = board
    fd.test_step_logits_equals_sample_then_step(hip, m, n, k, 130, opponent)
    if opponent != "net":
        de._folded_steps(hip, m, n, k, 257, opponent)
    for which in (0, 1, 2):
        for dtype in (torch.float32, torch.bfloat16, None):
            assert not hip.lib.jit_api_ready(m, n, k, hip.lib.jit_api_draw_kind(which, dtype))


# ----------------------------------------------------------------------------- 5. the fused rollout
_ORACLE_ROLLOUTS = {}


def _chunks(c):
    """three launches that continue the Philox counter; all but the last a multiple of four plies (the action log)"""
    return (max(4, (c // 3) & ~3), 8, c + 5)


def oracle_rollout(m, n, k, nenv):
    """the oracle's raw loop over ``_chunks``, once per (board, batch): every kernel form is compared with the same run"""
    key = (m, n, k, nenv)
    if key not in _ORACLE_ROLLOUTS:
        ora = OracleVectorEnv(m, n, k, nenv)
        out, step0 = [], 0
        for t in _chunks(m * n):
            planes, meta, stats = random_rollout(ora, seed=5, step0=step0, steps=t, env_id0=12345)
            step0 += t
            out.append((planes, meta, stats, pack_boards(ora.boards.numpy(), m, n), ora.current_player.numpy().copy(),
                        ora.move_counts.numpy().copy()))
        _ORACLE_ROLLOUTS[key] = out
    return _ORACLE_ROLLOUTS[key]


def log_formats(hip, c, form):
    rr = hip.rollout
    fmts = [f for f in (rr.ACT_U8, rr.ACT_U16, rr.ACT_BITS7, rr.ACT_U8P1) if rr.action_log_fits(f, c)]
    if form in ("ws2", "ws4"):
        return []                                      # the waves-per-group forms write no log
    if form != "lane":
        fmts = [f for f in fmts if f != rr.ACT_BITS7]  # the 7-bit stream exists in the one-lane form only
    if form == "pair":
        fmts = [f for f in fmts if f != rr.ACT_U8P1]   # the direction-split pair writes byte / 16-bit logs only
    return fmts


@pytest.mark.parametrize("nenv", [64, 333])
@pytest.mark.parametrize("board,form", BOARD_FORMS, ids=[f"{_id(b)}-{f}" for b, f in BOARD_FORMS])
def test_rollout_in_every_form_the_board_has(hip, board, form, nenv):
    """test_gpu_env.py's comparison -- records, statistics and final state of ``mnk_rollout_random`` against the oracle
    over three launches that continue the Philox counter -- with the kernel form forced, then the same launches with
    every action-log format the board and the form admit: the records again, the log decoded by the oracle's
    ``decode_action_log`` == the recorded actions, and ``mnk_replay_actions`` on the log rebuilds the records"""
    m, n, k = board
    c = m * n
    want = oracle_rollout(m, n, k, nenv)
    saved = ge._force_form(FORMS[form])
    try:
        for fmt in [None] + log_formats(hip, c, form):
            env = hip.Env(m, n, k, nenv, device=DEV)
            roll = hip.Rollout(env, seed=5, env_id0=12345)
            total = np.zeros(5, dtype=np.int64)
            for j, (t, (planes, meta, stats, final, cp, mc)) in enumerate(zip(_chunks(c), want)):
                where = f"{board} {form} N={nenv} log {fmt} chunk {j}"
                ge.assert_rollout_reaches(hip.lib, FORMS[form], forms_of(board), m, n, k, nenv, t, fmt)
                if fmt is None:
                    rec = roll.run(t)
                else:
                    state = hip.rollout.gather_start_state(env)  # (a copy: what a receiver holds at the chunk's start)
                    rec = roll.alloc(t, log_actions=fmt, with_state=False)
                    roll.run(t, out=rec)
                total += stats
                assert np.array_equal(rec.planes.cpu().numpy().view(np.uint64), planes), where
                assert np.array_equal(rec.meta.cpu().numpy().view(np.uint32), meta), where
                assert np.array_equal(roll.stats.cpu().numpy(), total), where
                assert np.array_equal(pack_boards(env.boards.cpu().numpy(), m, n), final), where
                assert np.array_equal(env.current_player.cpu().numpy(), cp) and np.array_equal(env.move_counts.cpu().numpy(), mc), where
                if fmt is not None:
                    log = rec.act.cpu().numpy().view(np.uint64 if fmt == hip.rollout.ACT_U16 else np.uint32)
                    actions = (meta & 0xFFFF).astype(np.int64)
                    assert np.array_equal(decode_action_log(log, t, fmt), actions), where
                    logs = hip.rollout.GatheredLogs.empty(1, 0, nenv, t, c, DEV, fmt=fmt, with_state=False)
                    logs.msg.copy_(rec.msg.unsqueeze(0))
                    again = hip.rollout.replay_shard(logs, 0, m, n, k, state=state)
                    assert torch.equal(again.planes, rec.planes) and torch.equal(again.meta, rec.meta), where + " replay"
                    assert torch.equal(state.planes[0], env._planes) and torch.equal(state.meta[0], env._meta), where + " replay state"
    finally:
        ge._restore_form(saved)


@pytest.mark.parametrize("board", SIBLINGS, ids=_id)
def test_replayed_logs_equal_the_oracles_replay(hip, board):
    """test_gpu_env.py's log test on the sibling, in each form that writes a log: every format, with and without the
    chunk-start state in the message, the oracle's own replay of the recorded actions"""
    m, n, k = board
    for form in [f for f in forms_of(board) if not f.startswith("ws")]:
        saved = ge._force_form(FORMS[form])
        try:
            steps = min(m * n + 6, 150)
            for fmt in log_formats(hip, m * n, "lane"):  # every format of the board: the form, or its fallback for that log
                for chunk in (steps - steps % 4, steps):
                    ge.assert_rollout_reaches(hip.lib, FORMS[form], forms_of(board), m, n, k, 33, chunk, fmt)
            ge.test_action_log_replay_rebuilds_the_records(hip, m, n, k, 33, steps, FORMS[form])
        finally:
            ge._restore_form(saved)


@pytest.mark.parametrize("board", [(8, 3, 3), (7, 9, 5), (12, 13, 5)], ids=_id)
def test_poked_states_take_the_general_loop_on_the_fast_siblings(hip, board):
    """the boards whose one-lane kernel has the loop without a full-board branch (NW <= 3 and <6,13,5>), where the valid
    cells stop before the variant's last row: hand-made inconsistent states in half of the waves"""
    saved = ge._force_form(FORMS["lane"])
    try:
        ge.test_rollout_on_poked_states_takes_the_general_loop(hip, *board)
    finally:
        ge._restore_form(saved)


@pytest.mark.parametrize("board,nenv,warm,plies", [((7, 9, 5), 40000, 120, 8), ((16, 15, 5), 33000, 330, 4)], ids=_id)
def test_a_launch_above_32768_envs_takes_the_one_lane_default(hip, board, nenv, warm, plies):
    """nothing forced: above 32 768 envs the launcher picks one lane per env with 32-bit record offsets (SADDR);
    test_gpu_env.py's ply-for-ply comparison of a stationary mix of game phases with the oracle, and the same plies
    through ``mnk_step_random``"""
    for key in ("MNK_ROLLOUT_PAIR", "MNK_ROLLOUT_FORM", "MNK_ROLLOUT_SADDR"):
        assert os.environ.get(key) is None
    assert hip.lib.rollout_form(nenv, *board, plies, records=True) == hip.lib.ROLLOUT_LANE | hip.lib.ROLLOUT_SADDR
    assert hip.lib.rollout_form(nenv, *board, warm, records=False) == hip.lib.ROLLOUT_LANE
    ge.test_full_size_rollout_equals_the_oracle_ply_for_ply(hip, *board, nenv, warm, plies)


# ----------------------------------------------------------------------------- 6. the row players
@pytest.mark.parametrize("board", PLAYER_BOARDS, ids=_id)
def test_monte_carlo_and_tree_search_players_equal_their_rules(hip, board):
    """``mnk_sample_playouts`` and ``mnk_sample_search`` against playout_rule / search_rule on ``player_cases.positions``
    (finished games, an empty and a full board in the batch), every observation dtype"""
    rows = {(8, 3, 3): 24, (7, 9, 5): 12, (16, 15, 5): 4}[board]
    gpl.test_counts_and_actions_equal_the_rule(hip, board, rows, (3, 8) if board[1] == 3 else (3,))
    gse.test_actions_and_stats_equal_the_rule(hip, board, rows, {(8, 3, 3): ((40, 8, 1.0), (64, 3, 0.5)), (7, 9, 5): ((64, 8, 1.0),),
                                                                 (16, 15, 5): ((40, 8, 1.0),)}[board])


@pytest.mark.parametrize("board", PLAYER_BOARDS + WIDE, ids=_id)
def test_puct_player_equals_its_rule(hip, board):
    """``mnk_puct_begin`` / ``mnk_puct_step`` through ``PUCTSearchPolicy.act`` against puct_rule: actions, visits, root
    values and every leaf, every observation / leaf / prior dtype"""
    gpu.test_exact_evaluator_equals_the_rule(hip, board, {(8, 3, 3): 16, (7, 9, 5): 8, (16, 15, 5): 4}.get(board, 3),
                                             {(8, 3, 3): 40, (7, 9, 5): 64, (16, 15, 5): 40}.get(board, 16))


@pytest.mark.parametrize("board", PLAYER_BOARDS, ids=_id)
def test_search_self_play_and_its_gather_equal_the_rule(hip, board):
    """``mnk_search_selfplay_step`` over more than a lap of the ring and ``mnk_search_gather`` against
    search_selfplay_rule: a non-square board admits the four symmetries that keep its shape (``sym_ok``), ids 4..7 are
    refused there"""
    m, n, k = board
    assert [s for s in range(8) if sym_ok(s, m, n)] == [0, 1, 2, 3]
    gss.test_the_gather_equals_the_rule(hip, board)
    gss.run(hip, m, n, k, 4, m * n + 9, torch.uint8, 3, True)


# ----------------------------------------------------------------------------- 6b. the later forms of the PUCT player
#            board        rows  J   plies
SEQUENCES = [((8, 3, 3), 16, 10, 12), ((7, 9, 5), 8, 16, 40), ((16, 15, 5), 4, 16, 6), ((12, 13, 5), 3, 8, 6),
             ((18, 19, 5), 3, 8, 6)]


@pytest.mark.parametrize("distance", [1, 2])
@pytest.mark.parametrize("board,rows,J,plies", SEQUENCES, ids=_id)
def test_a_kept_tree_over_a_sequence_of_plies_equals_its_rule(hip, board, rows, J, plies, distance):
    """``mnk_puct_rebase`` through ``PUCTSearchPolicy(reuse=True)`` against puct_reuse_rule at every ply, the next root one
    and two plies on; on the two small boards games end and their rows start again inside the sequence"""
    resets, carried = gre.run_sequence(hip, board, rows, J, plies, distance)
    assert (carried[1:, :, 0] > 1).any() and not carried[0].any()
    if board in ((8, 3, 3), (7, 9, 5)):
        assert (resets >= 1).any(), resets
        assert (carried[1:, :, 0] == 0).any()


def test_the_smallest_workspace_and_self_play_with_a_kept_tree_on_7x9x5(hip):
    gre.test_the_smallest_workspace_truncates_at_every_ply(hip, (7, 9, 5), 6, 16)
    gre.test_search_selfplay_with_reuse_equals_the_rule(hip, (7, 9, 5), 5, 16, 6)


LEAVES = [(_id(b), L) for b in PLAYER_BOARDS + WIDE for L in ((4, 16) if b in ((8, 3, 3), (7, 9, 5)) else (4,))]


@pytest.mark.parametrize("name,L", LEAVES)
def test_several_leaves_per_evaluation_equal_their_rule(hip, name, L):
    """``mnk_puct_begin_leaves`` / ``mnk_puct_step_leaves`` against puct_leaves_rule on the cases of
    tests/puct_leaves_cases.py"""
    assert (name, L) in gle.PARAMS
    gle.test_an_act_equals_the_rule(hip, name, L)


def test_several_leaves_with_a_kept_tree_and_narrow_dtypes(hip):
    for distance in (1, 2):
        gle.test_a_sequence_of_plies_with_a_kept_tree_equals_the_rule(hip, (7, 9, 5), 6, 16, distance)
    gle.test_narrow_dtypes_on_one_board(hip, torch.float32, torch.uint8, torch.bfloat16, 4, name="16x15x5")
    gle.test_narrow_dtypes_on_one_board(hip, torch.uint8, torch.bfloat16, torch.bfloat16, 4, name="16x15x5")


@pytest.mark.parametrize("temperature", [0, 1])
@pytest.mark.parametrize("L", gso.LEAVES)
@pytest.mark.parametrize("board", PLAYER_BOARDS + WIDE, ids=_id)
def test_the_solver_equals_its_rule(hip, board, L, temperature):
    """``mnk_puct_step_solver`` against puct_solver_rule on ``puct_solver_cases.sibling_positions``: one, two and three
    free cells (the board fills inside the search and the draw is proven at m * n stones), a full board, a win at once in
    row m - 1, mid-game rows.  tests/test_puct_solver_cpu.py shows that the rule with the variant's own cell and row count
    answers otherwise on these batches."""
    assert _id(board) in gso.CASES
    gso.test_an_act_equals_the_rule(hip, _id(board), L, temperature)


@pytest.mark.parametrize("L", [1, 4])
@pytest.mark.parametrize("temperature", [0, 1])
def test_a_noisy_act_equals_its_rule_on_7x9x5(hip, temperature, L):
    gno.test_a_noisy_act_equals_the_rule_on_the_kernels_priors(hip, (7, 9, 5), 8, temperature, L)


@pytest.mark.parametrize("dtype", list(ggu.DTYPES))
@pytest.mark.parametrize("name", ggu.SIBLINGS)
def test_the_gumbel_root_equals_its_rule(hip, name, dtype):
    """``mnk_puct_gumbel_root`` and ``mnk_puct_step_gumbel``: C = 63, 156 and 342 are no multiple of 4"""
    ggu.test_the_prep_kernel_equals_the_rule(hip, name, dtype)
    ggu.test_an_act_equals_the_rule_fed_with_the_kernels_gscore(hip, name, dtype)


def test_two_gumbel_shards_equal_one_call_on_7x9x5(hip):
    ggu.test_two_shards_equal_one_call(hip, "7x9x5")


@pytest.mark.parametrize("board,N,I,cons", [((8, 3, 3), 7, 8, 4), ((7, 9, 5), 5, 8, 8)], ids=_id)
def test_self_play_from_the_gumbel_roots_moves_equals_its_rule(hip, board, N, I, cons):
    """``mnk_search_selfplay_step_moves`` against ``GumbelSelfPlayRule`` for more than a lap of the T = C ring"""
    m, n, k = board
    ggu.run_selfplay(hip, board, N, I, cons, m * n + 9)


def test_the_lockstep_form_of_per_row_budgets_on_7x9x5(hip):
    gas.test_with_every_ply_full_it_is_the_lockstep_player(hip, (7, 9, 5), 5, 63 + 5, 63)


@pytest.mark.parametrize("case", gas.SIBLING_CASES, ids=lambda c: _id(c[0]) + ("-stored" if c[7] else ""))
def test_per_row_budgets_equal_their_rule_round_by_round(hip, case):
    """``mnk_search_selfplay_advance`` against ``AsyncSelfPlayRule``: games end, fast and full plies are recorded, the rows
    are out of step and, from the empty board (the two small boards), the T = C ring goes round more than twice; 7x9x5
    and the three large boards start from stored states near the end of games, two rows of which fill the board and are
    drawn at m * n stones -- the runs that a rule with the variant's own cell count plays otherwise
    (tests/test_search_selfplay_async_cpu.py)"""
    gas.test_mixed_budgets_equal_the_rule_round_by_round(hip, *case)
