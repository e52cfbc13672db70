"""GPU: the K-in-a-row scan line by line in every ROLLOUT form, and on every path of the scan by k.

tests/test_gpu_variant_siblings.py takes every line and every would-be wrap of a board through ``env.step``,
``wrapper.step`` and the tactical sampler: all of them reach ``mnk_plane_wins`` (csrc/mnk_device.h), on boards with k = 3
and k = 5.  The rollout kernels carry copies of the scan of their own that met the oracle on random games only -- a few
hundred wins on boards with up to 1 020 lines and 192 wraps, and none at all with k >= 8:

  pair     ``bs_run_bits_pair`` / ``bs_shr_pair`` (mnk_pair_scan.h): per-lane shift amounts, a per-word select where the word
           parts of the two shifts differ
  pairw    ``RolloutPairW::shr`` / ``run_steps`` (mnk_rollout_pairw.hip): a shift that crosses a lane's last word takes
           the partner's words by DPP; an odd word count leaves a padding word
  ws2/ws4  one or two directions per wave, the verdicts meet in LDS (mnk_rollout_lane.h)
  lane     the FAST loop (``done`` from ``nlegal == 1``) and the general loop (``moves >= C``)
  generic  run-time shift amounts (CN = CK = 0) -- and the hiprtc-compiled kernels of every board off the list, the
           run-time compiled pair form among them

Here every line and every wrap goes through them, with the constructions of tests/line_cases.py (checked on the CPU
by tests/test_line_cases_cpu.py): a board with ONE FREE CELL, where the rollout's own draw must play the completing move
whatever its random word, and FORCED SEQUENCES from the empty board through ``mnk_replay_actions``.  The win flag is held
to the brute-force rule (``line_rule.cases``), everything else -- records, statistics, final state -- to the oracle, bit
for bit.  The boards: every built-in variant's board in every form it has, and thirteen boards off the list that
between them take each path of ``bs_has_run`` (k a power of two; len + 1 == k; the general tail; k = 1), on the generic
kernels (MNK_JIT = MNK_JIT_API = 0) and on their own (= 1; one lane and two lanes per env).
"""
import contextlib
import os

import numpy as np
import pytest
import torch

import line_cases as lc
import line_rule as lr
import test_gpu_env as ge
import test_gpu_variant_siblings as vs
from oracle.env_torch import OracleVectorEnv
from oracle.packing import pack_boards
from oracle.rollout import encode_action_log, random_rollout, replay_actions

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

hip = ge.hip  # the module-scoped fixture of test_gpu_env.py (binding, env, rollout)

BUILTIN = vs.SIBLINGS + vs.SQUARES
BOARD_FORMS = [(b, f) for b in BUILTIN for f in vs.forms_of(b)]
CHUNKS = (1, 5)  # the completing ply alone, then a few more: finished games restart, the others go on on a full board
COUNTERS = ("last cell", "k - 1")
KNOBS = ("MNK_JIT", "MNK_JIT_API", "MNK_ROLLOUT_PAIR", "MNK_ROLLOUT_FORM")
_id = vs._id


@contextlib.contextmanager
def knobs(lib, **values):
    """the library's environment knobs set to ``values`` (None: unset) for the block, then as they were"""
    saved = {key: os.environ.get(key) for key in KNOBS}
    for key in KNOBS:
        os.environ.pop(key, None)
    os.environ.update({key: val for key, val in values.items() if val is not None})
    lib.reload_config()
    try:
        yield
    finally:
        for key, val in saved.items():
            if val is None:
                os.environ.pop(key, None)
            else:
                os.environ[key] = val
        lib.reload_config()


def no_compilation_failed(lib):
    """a run-time kernel that does not compile or load hands its launch to the ahead-of-time kernel without a word; both
    failures leave a message"""
    assert lib.jit_stats()["failed"] == 0 and not lib.load().mnk_jit_last_error(), lib.load().mnk_jit_last_error()


def wrong_cases(where, wrong, cs):
    """the failure message: board, form / mode, side, and the cells of the first cases the kernel gets wrong (a string:
    pytest prints it whole)"""
    first = "; ".join(f"cells {list(cs[i][0])} {'win' if cs[i][1] else 'do not win'}" for i in wrong[:4])
    return f"{where}: {len(wrong)} of {len(cs)} cases wrong, the first: {first}"


# ----------------------------------------------------------------------------- one free cell
_ORACLE = {}


def oracle_one_free_cell(board, side, counters):
    """``random_rollout`` over CHUNKS on the poked oracle, once per (board, mover, counters): every form and mode is
    compared with the same run"""
    key = (board, side, counters)
    if key not in _ORACLE:
        m, n, k = board
        _, mine, theirs, _, _, _ = lc.one_free_cell(m, n, k)
        nenv = len(mine)
        ora = OracleVectorEnv(m, n, k, nenv)
        vs.poke(ora, lc.boards_of(mine, theirs, side, m, n), np.full(nenv, side, dtype=np.int64),
                np.full(nenv, m * n - 1 if counters == "last cell" else k - 1, dtype=np.int64))
        out, step0 = [], 0
        for t in CHUNKS:
            planes, meta, stats = random_rollout(ora, seed=5, step0=step0, steps=t, env_id0=777)
            step0 += t
            out.append((planes, meta, stats, pack_boards(ora.boards.numpy(), m, n), ora.current_player.numpy().copy(),
                        ora.move_counts.numpy().copy()))
        _ORACLE[key] = out
    return _ORACLE[key]


def one_free_cell_rollout(hip, board, tag, expect_form):
    """One env per line / wrap, full but for the completing cell, black and white as the mover, the counters at the
    stone count (a consistent game: the one-lane FAST loop, a win against a draw at the last cell) and at k - 1 (the
    general loop, done == win).  ``expect_form(nenv, plies)`` holds the launch to its kernel."""
    m, n, k = board
    c = m * n
    cs = lr.cases(m, n, k)
    keep, mine, theirs, free, wins, _ = lc.one_free_cell(m, n, k)
    nenv, nwin = len(keep), int(wins.sum())
    for side in (0, 1):
        for counters in COUNTERS:
            where = f"{_id(board)} {tag}, {'white' if side else 'black'} to move, counters {counters}"
            full = counters == "last cell"
            count = c - 1 if full else k - 1
            env = hip.Env(m, n, k, nenv, device=DEV)
            vs.poke(env, lc.boards_of(mine, theirs, side, m, n), np.full(nenv, side, dtype=np.int64), np.full(nenv, count, dtype=np.int64))
            roll = hip.Rollout(env, seed=5, env_id0=777)
            total = np.zeros(5, dtype=np.int64)
            for j, (t, (planes, meta, stats, final, cp, mc)) in enumerate(zip(CHUNKS, oracle_one_free_cell(board, side, counters))):
                expect_form(nenv, t)
                rec = roll.run(t)
                got = rec.meta.cpu().numpy().view(np.uint32)
                total += stats
                if j == 0:  # the rule: the draw found the free cell, and the move wins iff the case is a line
                    win, done = ((got[0] >> 16) & 0xFF) == 1, ((got[0] >> 24) & 1) == 1
                    assert np.array_equal((got[0] & 0xFFFF).astype(np.int64), free), where
                    wrong = np.flatnonzero(win != wins)
                    assert wrong.size == 0, wrong_cases(where, wrong, [cs[i] for i in keep])
                    assert np.array_equal(done, wins | full), where
                    assert roll.stats.cpu().tolist() == [nenv if full else nwin, nwin * (1 - side), nwin * side, (nenv - nwin) * full,
                                                         (nenv if full else nwin) * (count + 1)], where
                assert np.array_equal(got, meta), f"{where}: chunk {j} meta"
                assert np.array_equal(rec.planes.cpu().numpy().view(np.uint64), planes), f"{where}: chunk {j} planes"
                assert np.array_equal(roll.stats.cpu().numpy(), total), f"{where}: chunk {j} statistics"
                assert np.array_equal(pack_boards(env.boards.cpu().numpy(), m, n), final), f"{where}: chunk {j} final boards"
                assert np.array_equal(env.current_player.cpu().numpy(), cp) and np.array_equal(env.move_counts.cpu().numpy(), mc), where
            env.check_errors()
    print(f"line scan: {_id(board)} {tag}: {nwin} lines + {nenv - nwin} wraps x 2 movers x 2 counter settings")


@pytest.mark.parametrize("board,form", BOARD_FORMS, ids=[f"{_id(b)}-{f}" for b, f in BOARD_FORMS])
def test_every_line_and_wrap_through_every_rollout_form(hip, board, form):
    """the built-in variants: each board in each form it has, forced and held as test_gpu_env.py does"""
    m, n, k = board
    saved = ge._force_form(vs.FORMS[form])
    try:
        one_free_cell_rollout(hip, board, form, lambda nenv, t: ge.assert_rollout_reaches(hip.lib, vs.FORMS[form], vs.forms_of(board), m, n, k, nenv, t))
    finally:
        ge._restore_form(saved)


# ----------------------------------------------------------------------------- forced sequences
def replayed_sequences(hip, board, tag=""):
    """the action logs of ``line_cases.sequences`` through ``mnk_replay_actions`` in every log format the board admits:
    the completing ply wins iff the case is a line (the rule); records == the oracle's replay"""
    m, n, k = board
    c = m * n
    cs = lr.cases(m, n, k)
    wins = np.array([w for _, w in cs])
    nenv = len(cs)
    rr = hip.rollout
    for side in (0, 1) if k > 1 else (0,):  # (k = 1: black's first stone wins, white never completes anything)
        acts = lc.sequences(m, n, k, side).copy()
        steps, t_done = len(acts), lc.completing_ply(k, side)
        want_planes, want_meta = replay_actions(OracleVectorEnv(m, n, k, nenv), acts)
        for fmt in vs.log_formats(hip, c, "lane"):
            where = f"{_id(board)} {tag} replay, {'white' if side else 'black'} completes, log format {fmt}"
            env = hip.Env(m, n, k, nenv, device=DEV)
            logs = rr.GatheredLogs.empty(1, env.words, nenv, steps, c, DEV, fmt=fmt)
            logs.msg.zero_()
            log = encode_action_log(acts, fmt)
            logs.act[0].copy_(torch.from_numpy(log.view(np.int64 if fmt == rr.ACT_U16 else np.int32)))
            logs.planes0[0].copy_(env._planes)
            logs.meta0[0].copy_(env._meta)
            err = torch.zeros(2, dtype=torch.int32, device=DEV)
            rec = rr.replay_shard(logs, 0, m, n, k, err=err)
            got = rec.meta.cpu().numpy().view(np.uint32)
            assert err.cpu().tolist() == [0, 0], where
            assert np.array_equal((got & 0xFFFF).astype(np.int64), acts), where
            win = ((got[t_done] >> 16) & 0xFF) == 1
            wrong = np.flatnonzero(win != wins)
            assert wrong.size == 0, wrong_cases(where, wrong, cs)
            assert np.array_equal(((got[t_done] >> 24) & 1) == 1, wins) and not ((got[:t_done] >> 24) & 1).any(), where
            assert np.array_equal(got, want_meta), f"{where}: meta"
            assert np.array_equal(rec.planes.cpu().numpy().view(np.uint64), want_planes), f"{where}: planes"
    print(f"line scan: {_id(board)} {tag} replay: {int(wins.sum())} lines + {int((~wins).sum())} wraps x {2 if k > 1 else 1} completing sides "
          f"x {len(vs.log_formats(hip, c, 'lane'))} log formats")


@pytest.mark.parametrize("board", BUILTIN, ids=_id)
def test_every_line_and_wrap_through_the_replay_of_a_forced_log(hip, board):
    replayed_sequences(hip, board)


# ----------------------------------------------------------------------------- every path of the scan by k
MODES = {"generic": "0", "own": "1"}  # MNK_JIT = MNK_JIT_API: the generic kernels / the board's own, compiled by hiprtc
OFF_MODES = [(b, mode) for b in lc.OFF_LIST for mode in MODES]
_OFF_IDS = [f"{_id(b)}-{mode}" for b, mode in OFF_MODES]


def test_the_boards_off_the_list_have_no_built_in_variant(hip):
    lib = hip.lib
    with knobs(lib, MNK_JIT="0", MNK_JIT_API="0", MNK_ROLLOUT_PAIR="1"):
        for m, n, k in lc.OFF_LIST:  # two lanes asked for, no built-in variant: the generic one-lane kernel
            assert lib.rollout_form(64, m, n, k, 4, True) == lib.ROLLOUT_LANE, (m, n, k)
    assert not set(lc.OFF_LIST) & set(BUILTIN)


@pytest.mark.parametrize("board,mode", OFF_MODES, ids=_OFF_IDS)
def test_off_list_every_line_and_wrap_through_env_step(hip, board, mode):
    """the ``env.step`` test of the sibling module (its cases and helpers: sparse poked states, black and white; the rule
    first, so that a failure names the cells, then the oracle) on ``k_step_full`` with run-time shifts and as compiled
    for the board"""
    lib = hip.lib
    m, n, k = board
    with knobs(lib, MNK_JIT=MODES[mode], MNK_JIT_API=MODES[mode]):
        for side in (0, 1):
            where = f"{_id(board)} {mode} env.step, {'white' if side else 'black'} to move"
            boards, acts, want = vs.line_cases_for_step(m, n, k, side)
            nenv = len(acts)
            env, ora = hip.Env(m, n, k, nenv, device=DEV), OracleVectorEnv(m, n, k, nenv)
            for target in (env, ora):
                vs.poke(target, boards, np.full(nenv, side, dtype=np.int64), np.full(nenv, k - 1, dtype=np.int64))
            out = env.step(torch.from_numpy(acts).to(DEV))
            wrong = np.flatnonzero(out[2].cpu().numpy() != want)
            assert wrong.size == 0, wrong_cases(where, wrong, lr.cases(m, n, k))
            assert np.array_equal(out[1].cpu().numpy(), want.astype(np.float32)), where
            vs.exactly_zero_or_one(out[0]["observation"])
            vs.same_step(out, ora.step(torch.from_numpy(acts)), env, ora, where)
            env.check_errors()
        assert lib.jit_api_ready(m, n, k, lib.JIT_API_STEP) or mode == "generic", lib.load().mnk_jit_last_error()
        assert lib.jit_prepare(m, n, k, [lib.JIT_API_STEP]) == (1 if mode == "own" else 0)
    no_compilation_failed(lib)
    print(f"line scan: {_id(board)} {mode} env.step: {len(lr.lines(m, n, k))} lines + {len(lr.wraps(m, n, k))} wraps x 2 movers")


OFF_FILLED = [(b, mode) for b, mode in OFF_MODES if b[2] >= 3]  # (no full board is free of runs of two)


@pytest.mark.parametrize("board,mode", OFF_FILLED, ids=[f"{_id(b)}-{mode}" for b, mode in OFF_FILLED])
def test_off_list_every_line_and_wrap_through_the_rollout(hip, board, mode):
    """the one-free-cell rollout on ``k_rollout_random<NW, 0, 0>`` (generic) and on the board's own kernels with one
    lane and with two lanes per env (``k_rollout_random_pair``, compiled at run time); ``mnk_rollout_form`` names the
    kernel and nothing may have failed to compile"""
    lib = hip.lib
    m, n, k = board

    def held_to(code):
        def check(nenv, t):
            got = lib.rollout_form(nenv, m, n, k, t, True)
            assert got == code, f"{_id(board)} {mode}: expected form {code:#x}, runs {got:#x}"
        return check

    if mode == "generic":
        with knobs(lib, MNK_JIT="0", MNK_JIT_API="0", MNK_ROLLOUT_PAIR="0"):
            one_free_cell_rollout(hip, board, "generic lane", held_to(lib.ROLLOUT_LANE))
    else:
        with knobs(lib, MNK_JIT="1", MNK_JIT_API="1", MNK_ROLLOUT_PAIR="0"):
            one_free_cell_rollout(hip, board, "own lane", held_to(lib.ROLLOUT_LANE | lib.ROLLOUT_SADDR | lib.ROLLOUT_JIT))
            no_compilation_failed(lib)
        with knobs(lib, MNK_JIT="1", MNK_JIT_API="1", MNK_ROLLOUT_PAIR="1"):
            one_free_cell_rollout(hip, board, "own pair", held_to(lib.ROLLOUT_PAIR | lib.ROLLOUT_SADDR | lib.ROLLOUT_JIT))
            no_compilation_failed(lib)


@pytest.mark.parametrize("board,mode", OFF_MODES, ids=_OFF_IDS)
def test_off_list_every_line_and_wrap_through_the_replay_of_a_forced_log(hip, board, mode):
    """(``mnk_replay_actions`` has a kernel of the board's own only beyond 16 words per plane: up to there both modes
    replay on ``k_replay_actions<NW, 0, 0>``, whatever the knobs say)"""
    with knobs(hip.lib, MNK_JIT=MODES[mode], MNK_JIT_API=MODES[mode]):
        replayed_sequences(hip, board, mode)
    no_compilation_failed(hip.lib)
