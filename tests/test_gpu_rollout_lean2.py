"""The rollout ply's lean bookkeeping against the oracle rollout, record for record.

What the kernel no longer carries through its FAST loops -- the side to move (now the parity of the stone count), a
counter of white's wins of its own (now the high half of one register), round 1's lane-invariant Philox product (now
computed once per launch) -- is each pinned where a mistake in it would show:

* a hand-flipped side on a board whose stones still equal its ply count: only the parity term of the consistency test
  sends that wave to the general loop;
* 3x3x3, where games end every few plies, by a win of either colour or by a draw: the white-win count, the resets;
* env ids whose low word wraps inside the wave: a hoisted product built from the wrong half of the id;
* a board the library compiles at run time: the text hiprtc sees is the text hipcc saw.

Every case compares planes, meta words and all five statistics of every ply, and the final state, in both
``lanes_per_env`` forms."""
import numpy as np
import pytest
import torch

import test_gpu_env as ge
import test_gpu_line_scan as ls
from oracle.env_torch import OracleVectorEnv
from oracle.packing import pack_boards
from oracle.rollout import random_rollout

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FORMS = {"one lane per env": "0", "two lanes per env": "1"}  # MNK_ROLLOUT_PAIR

hip = ge.hip


def final_state(ora):
    return (pack_boards(ora.boards.numpy(), ora.m, ora.n), ora.current_player.numpy().copy(), ora.move_counts.numpy().copy())


def same_rollout(roll, env, rec, want, where):
    planes, meta, stats, (boards, side, counts) = want
    assert np.array_equal(rec.meta.cpu().numpy().view(np.uint32), meta), f"{where}: meta words"
    assert np.array_equal(rec.planes.cpu().numpy().view(np.uint64), planes), f"{where}: record planes"
    assert np.array_equal(roll.stats.cpu().numpy(), stats), f"{where}: statistics {roll.stats.cpu().tolist()} != {stats.tolist()}"
    assert np.array_equal(pack_boards(env.boards.cpu().numpy(), env.m, env.n), boards), f"{where}: final boards"
    assert np.array_equal(env.current_player.cpu().numpy(), side), f"{where}: final side to move"
    assert np.array_equal(env.move_counts.cpu().numpy(), counts), f"{where}: final ply counts"
    env.check_errors()


# ----------------------------------------------------------------------------- a poked side on 9x9x5
POKED = dict(board=(9, 9, 5), nenv=128, opening=5, steps=37, env=64 + 17, seed=23)
_POKED = {}


def oracle_poked_side():
    """five plies of the env's own play, then one env outside the first wave (env 81: the second wave with one lane per
    env, the third with two) gets its side flipped, then 37 plies from
    step 5: (the opening's records, the state the flip is made in, the 37 plies' records and final state)"""
    if not _POKED:
        m, n, k = POKED["board"]
        ora = OracleVectorEnv(m, n, k, POKED["nenv"])
        opening = random_rollout(ora, seed=POKED["seed"], step0=0, steps=POKED["opening"])
        side = ora.current_player.numpy().copy()
        assert (ora.move_counts.numpy() == POKED["opening"]).all() and (side == POKED["opening"] % 2).all()
        side[POKED["env"]] ^= 1
        ora.current_player.copy_(torch.from_numpy(side))
        planes, meta, stats = random_rollout(ora, seed=POKED["seed"], step0=POKED["opening"], steps=POKED["steps"])
        _POKED["run"] = (opening, side, (planes, meta, opening[2] + stats, final_state(ora)))
    return _POKED["run"]


@pytest.mark.parametrize("form", list(FORMS))
def test_a_flipped_side_on_a_board_whose_stones_match_its_count(hip, form):
    m, n, k = POKED["board"]
    opening, side, want = oracle_poked_side()
    with ls.knobs(hip.lib, MNK_ROLLOUT_PAIR=FORMS[form]):
        env = hip.Env(m, n, k, POKED["nenv"], device=DEV)
        roll = hip.Rollout(env, seed=POKED["seed"])
        rec = roll.run(POKED["opening"])
        assert np.array_equal(rec.meta.cpu().numpy().view(np.uint32), opening[1]), f"{form}: the opening's meta words"
        # stones == plies counted on every board, and on one of them the wrong colour to move
        stones = env.boards.cpu().numpy().reshape(POKED["nenv"], -1).sum(axis=1)
        assert np.array_equal(stones, env.move_counts.cpu().numpy()) and (stones == POKED["opening"]).all()
        env.current_player = torch.from_numpy(side)
        assert roll.step == POKED["opening"]
        rec = roll.run(POKED["steps"])
        same_rollout(roll, env, rec, want, f"9x9x5, {form}, side of env {POKED['env']} flipped")


# ----------------------------------------------------------------------------- dense resets, wins and draws on 3x3x3
_DENSE = {}


def oracle_dense(step0):
    if step0 not in _DENSE:
        ora = OracleVectorEnv(3, 3, 3, 64)
        planes, meta, stats = random_rollout(ora, seed=31, step0=step0, steps=41)
        _DENSE[step0] = (planes, meta, stats, final_state(ora))
    return _DENSE[step0]


@pytest.mark.parametrize("step0", (0, 2))
@pytest.mark.parametrize("form", list(FORMS))
def test_dense_resets_wins_of_both_colours_and_draws_on_3x3x3(hip, form, step0):
    want = oracle_dense(step0)
    stats = want[2]
    assert stats[2] > 0 and stats[3] > 0 and stats[1] > 0, f"the oracle's games must end all three ways: {stats.tolist()}"
    with ls.knobs(hip.lib, MNK_ROLLOUT_PAIR=FORMS[form]):
        env = hip.Env(3, 3, 3, 64, device=DEV)
        roll = hip.Rollout(env, seed=31)
        roll.step = step0
        rec = roll.run(41)
        same_rollout(roll, env, rec, want, f"3x3x3, {form}, step0 {step0}")


# ----------------------------------------------------------------------------- env ids whose low word wraps in the wave
ENV_ID0 = 2 ** 32 - 32
_WRAP = {}


def oracle_wrap():
    if not _WRAP:
        ora = OracleVectorEnv(9, 9, 5, 64)
        planes, meta, stats = random_rollout(ora, seed=47, step0=0, steps=8, env_id0=ENV_ID0)
        _WRAP["run"] = (planes, meta, stats, final_state(ora))
    return _WRAP["run"]


@pytest.mark.parametrize("form", list(FORMS))
def test_philox_where_the_env_ids_low_word_wraps_inside_the_wave(hip, form):
    with ls.knobs(hip.lib, MNK_ROLLOUT_PAIR=FORMS[form]):
        env = hip.Env(9, 9, 5, 64, device=DEV)
        roll = hip.Rollout(env, seed=47, env_id0=ENV_ID0)
        rec = roll.run(8)
        same_rollout(roll, env, rec, oracle_wrap(), f"9x9x5, {form}, env ids from 2^32 - 32")


# ----------------------------------------------------------------------------- a board compiled at run time
_JIT = {}


def oracle_jit():
    if not _JIT:
        ora = OracleVectorEnv(7, 9, 7, 64)
        planes, meta, stats = random_rollout(ora, seed=59, step0=0, steps=16)
        _JIT["run"] = (planes, meta, stats, final_state(ora))
    return _JIT["run"]


@pytest.mark.parametrize("form", list(FORMS))
def test_a_run_time_specialised_board_7x9x7(hip, form):
    with ls.knobs(hip.lib, MNK_JIT="1", MNK_JIT_API="1", MNK_ROLLOUT_PAIR=FORMS[form]):
        env = hip.Env(7, 9, 7, 64, device=DEV)
        roll = hip.Rollout(env, seed=59)
        rec = roll.run(16)
        torch.cuda.synchronize()
        ls.no_compilation_failed(hip.lib)
        same_rollout(roll, env, rec, oracle_jit(), f"7x9x7 compiled at run time, {form}")


# ----------------------------------------------------------------------------- a launch that crosses 2^32 Philox blocks
STEP_WRAP = 4 * 2 ** 32 - 8  # the block number's low word wraps after the launch's second block
_BLOCKS = {}


def oracle_block_wrap():
    if not _BLOCKS:
        ora = OracleVectorEnv(9, 9, 5, 64)
        planes, meta, stats = random_rollout(ora, seed=61, step0=STEP_WRAP, steps=18)
        _BLOCKS["run"] = (planes, meta, stats, final_state(ora))
    return _BLOCKS["run"]


@pytest.mark.parametrize("form", list(FORMS))
def test_a_launch_in_which_the_block_numbers_low_word_wraps(hip, form):
    """the FAST loops count Philox blocks with a block number of their own: the launch that crosses a multiple of 2^32
    blocks has to carry into the counter's fourth word between two blocks"""
    with ls.knobs(hip.lib, MNK_ROLLOUT_PAIR=FORMS[form]):
        env = hip.Env(9, 9, 5, 64, device=DEV)
        roll = hip.Rollout(env, seed=61)
        roll.step = STEP_WRAP
        rec = roll.run(18)
        same_rollout(roll, env, rec, oracle_block_wrap(), f"9x9x5, {form}, step0 = 2^34 - 8")
