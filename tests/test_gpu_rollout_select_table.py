"""The LDS byte table that ends the r-th-legal-cell select of the rollout kernels which have a FAST loop (DESIGN.md
section 5 row 36; ``MnkSelectTable`` / ``select_bit32_nr_tab`` in csrc/mnk_device.h).

On the CPU: the table as its ``constexpr`` generator makes it (``mnk_probe_select_table``), all 256 x 8 entries, against
the definition restated here.

On the GPU: the kernels that read it -- the one-lane form (``MNK_ROLLOUT_PAIR=0``; ``mnk_rollout_form`` confirms the
form) of the boards of at most three words -- against the oracle rollout, record for record: planes, meta words, all
five statistics, the final state.  Each case sits where the table could go wrong on its own:

* a last wave of one lane (N = 1, N = 65): all 64 threads fill the table before the ``i < N`` test, or a quarter of it
  is missing;
* games that end and restart (9x9x5, 512 plies): legal sets of every size, the pick in every word;
* 3x3x3: nine cells in two bytes, every bit of a byte legal at the start, ranks up to 7 within a byte;
* 13x13x5: the six-word kernel with a FAST loop, which measured slower with the table and keeps the arithmetic select
  -- the flag must leave it whole, its own Philox block (not made a trip ahead) included;
* 6x7x4, compiled at run time: hiprtc reads the same text, the ``constexpr`` generator included;
* a poked counter: that wave plays the general loop of the same kernel, which reads the table too.

The two-lane forms do not take the table (their code is the parent's), so there is no case for them here: the
existing suite holds them to the oracle."""
import ctypes

import numpy as np
import pytest
import torch

import __graft_entry__ as entry
import test_gpu_env as ge
import test_gpu_line_scan as ls
from oracle.env_torch import OracleVectorEnv
from oracle.rollout import random_rollout
from test_gpu_rollout_lean2 import final_state, same_rollout

DEV = "cuda:0"
LANE, FORM_MASK, JIT = 1, 0xF, 0x20


# ----------------------------------------------------------------------------- the table itself (CPU)
def table_by_definition():
    """t[b][r] = position of the r-th (0-based) set bit of byte b; 0 where r >= popcount(b)"""
    t = np.zeros((256, 8), dtype=np.uint8)
    for b in range(256):
        positions = [p for p in range(8) if (b >> p) & 1]
        for r, p in enumerate(positions):
            t[b, r] = p
    return t


def test_the_generators_table_is_the_definition_in_all_2048_entries():
    entry.build_hip()
    entry._ensure_path()
    import mnk_hip

    got = np.full((256, 8), 0xEE, dtype=np.uint8)
    assert mnk_hip.load().mnk_probe_select_table(got.ctypes.data_as(ctypes.c_void_p)) == 0
    want = table_by_definition()
    wrong = np.argwhere(got != want)
    assert len(wrong) == 0, f"{len(wrong)} entries differ, the first at byte {wrong[0][0]:#04x}, rank {wrong[0][1]}: " \
                            f"{got[tuple(wrong[0])]} != {want[tuple(wrong[0])]}"
    # the definition, said the other way round: every set bit of every byte is found at its rank, nothing else is
    for b in range(256):
        n = bin(b).count("1")
        assert sum(1 << int(p) for p in got[b, :n]) == b and not got[b, n:].any(), f"byte {b:#04x}: {got[b].tolist()}"


# ----------------------------------------------------------------------------- the kernels that read it (GPU)
hip = ge.hip

_ORACLE = {}


def oracle_run(board, nenv, steps, seed):
    key = (board, nenv, steps, seed)
    if key not in _ORACLE:
        ora = OracleVectorEnv(*board, nenv)
        planes, meta, stats = random_rollout(ora, seed=seed, step0=0, steps=steps)
        _ORACLE[key] = (planes, meta, stats, final_state(ora))
    return _ORACLE[key]


def one_lane_form(hip, board, nenv, steps, jit=False):
    """the launch takes the one-lane kernel (compiled at run time where asked): the form that reads the table"""
    form = hip.lib.load().mnk_rollout_form(nenv, *board, steps, 1, 0, 0)
    assert form & FORM_MASK == LANE and bool(form & JIT) == jit, f"{board} x {nenv}: form {form:#x}"


CASES = {
    "9x9x5, a wave of one lane": ((9, 9, 5), 1, 64),
    "9x9x5, a full wave and one lane": ((9, 9, 5), 65, 64),
    "9x9x5, games end and restart": ((9, 9, 5), 128, 512),
    "3x3x3, dense bytes": ((3, 3, 3), 64, 64),
    "13x13x5, six words": ((13, 13, 5), 64, 128),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_the_one_lane_kernels_equal_the_oracle(hip, case):
    board, nenv, steps = CASES[case]
    want = oracle_run(board, nenv, steps, seed=71)
    if steps >= 512:
        assert want[2][0] > nenv, f"the oracle's games must end and restart: {want[2].tolist()}"
    with ls.knobs(hip.lib, MNK_ROLLOUT_PAIR="0"):
        one_lane_form(hip, board, nenv, steps)
        env = hip.Env(*board, nenv, device=DEV)
        roll = hip.Rollout(env, seed=71)
        rec = roll.run(steps)
        same_rollout(roll, env, rec, want, case)


@pytest.mark.gpu
def test_a_board_compiled_at_run_time_6x7x4(hip):
    board, nenv, steps = (6, 7, 4), 64, 64
    want = oracle_run(board, nenv, steps, seed=73)
    with ls.knobs(hip.lib, MNK_JIT="1", MNK_ROLLOUT_PAIR="0"):
        one_lane_form(hip, board, nenv, steps, jit=True)
        env = hip.Env(*board, nenv, device=DEV)
        roll = hip.Rollout(env, seed=73)
        rec = roll.run(steps)
        torch.cuda.synchronize()
        ls.no_compilation_failed(hip.lib)
        same_rollout(roll, env, rec, want, "6x7x4 compiled at run time")


@pytest.mark.gpu
def test_a_poked_counter_sends_the_wave_through_the_general_loop(hip):
    """eight plies of the env's own play, then one env's ply counter is set behind its stones: the wave is no longer
    consistent and plays the launch on the general loop of the same kernel -- same table, same records"""
    board, nenv, opening, steps, poked = (9, 9, 5), 64, 8, 96, 21
    ora = OracleVectorEnv(*board, nenv)
    first = random_rollout(ora, seed=79, step0=0, steps=opening)
    ora.move_counts[poked] = 2
    planes, meta, stats = random_rollout(ora, seed=79, step0=opening, steps=steps)
    want = (planes, meta, first[2] + stats, final_state(ora))
    with ls.knobs(hip.lib, MNK_ROLLOUT_PAIR="0"):
        one_lane_form(hip, board, nenv, steps)
        env = hip.Env(*board, nenv, device=DEV)
        roll = hip.Rollout(env, seed=79)
        rec = roll.run(opening)
        assert np.array_equal(rec.meta.cpu().numpy().view(np.uint32), first[1]), "the opening's meta words"
        env.move_counts[poked] = 2
        rec = roll.run(steps)
        same_rollout(roll, env, rec, want, f"9x9x5, ply counter of env {poked} set to 2 after {opening} plies")
