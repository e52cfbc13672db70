"""GPU: the rollout kernels' statistics (csrc/mnk_device.h, mnk_stats_wave_totals) against the launch's own records.

Every rollout kernel sums four per-lane counts over its wave with a DPP add ladder and hands the wave's totals to one
replica row of ``stats``.  What can go wrong there shows in the sums and nowhere else -- a lane left out or counted twice
at a row or half-wave boundary, lanes without an env (a partly filled last wave, the second lane of a pair) adding
something, a total landing in the wrong counter or the wrong replica row -- so each case recomputes, from the done,
reward and side bits of the launch's own meta words and the envs' ply counters before the launch, what every replica
row must have gained, and compares the raw ``int64[REPLICAS][STRIDE]`` array word for word; the summed counters must
also equal the oracle's, as in the other rollout tests.  Shapes: a single lane, a partly filled only wave, a full wave,
a last wave of one lane, two full waves and two lanes; launches in which nothing finishes (every total zero: nothing
may be added); the largest legal launch, where a wave's sums are largest."""
import contextlib
import functools
import os

import numpy as np
import pytest
import torch

from oracle.env_torch import OracleVectorEnv
from oracle.rollout import random_rollout

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KNOBS = ("MNK_ROLLOUT_PAIR", "MNK_ROLLOUT_FORM", "MNK_JIT")
SEED, ENV_ID0 = 5, 12345  # env_id0 != 0: the statistics do not depend on it, the games do


@pytest.fixture(scope="module")
def hip():
    import __graft_entry__ as entry

    entry.build_hip()
    entry._ensure_path()
    import mnk_hip
    from env.torch_vector_mnk_env import TorchVectorMnkEnv
    from selfplay.random_rollout import RandomRollout

    mnk_hip.load()
    assert torch.cuda.is_available()

    class NS:
        pass

    ns = NS()
    ns.lib, ns.Env, ns.Rollout = mnk_hip, TorchVectorMnkEnv, RandomRollout
    return ns


@contextlib.contextmanager
def knobs(lib, **values):
    """the library's developer knobs for the duration of a case (it reads them once: reload_config)"""
    saved = {key: os.environ.get(key) for key in KNOBS}
    try:
        for key in KNOBS:
            os.environ.pop(key, None)
        for key, val in values.items():
            os.environ[key] = val
        lib.reload_config()
        yield
    finally:
        for key, val in saved.items():
            if val is None:
                os.environ.pop(key, None)
            else:
                os.environ[key] = val
        lib.reload_config()


# form -> (knobs, the form code mnk_rollout_form must report, envs per workgroup = per replica row)
FORMS = {
    "lane": ({"MNK_ROLLOUT_PAIR": "0"}, "ROLLOUT_LANE", 64),
    "pair": ({"MNK_ROLLOUT_PAIR": "1", "MNK_ROLLOUT_FORM": "pair"}, "ROLLOUT_PAIR", 32),
    "pairw": ({"MNK_ROLLOUT_PAIR": "1", "MNK_ROLLOUT_FORM": "pairw"}, "ROLLOUT_PAIRW", 32),
    "ws2": ({"MNK_ROLLOUT_PAIR": "0", "MNK_ROLLOUT_FORM": "ws2"}, "ROLLOUT_WS2", 64),
    "ws4": ({"MNK_ROLLOUT_PAIR": "0", "MNK_ROLLOUT_FORM": "ws4"}, "ROLLOUT_WS4", 64),
    "lane, compiled at run time": ({"MNK_ROLLOUT_PAIR": "0", "MNK_JIT": "1"}, "ROLLOUT_LANE", 64),
    "lane, the generic kernel": ({"MNK_ROLLOUT_PAIR": "0", "MNK_JIT": "0"}, "ROLLOUT_LANE", 64),
}


def gained_from_records(lib, meta, moves_before, group):
    """What one launch adds to the raw statistics, from its meta words u32[T][N] and the envs' ply counters before it:
    int64[REPLICAS][STRIDE].  A finished game is a done bit; it was won iff the reward field is 1, by the side in the
    side bit; its length is the ply counter before the launch (first game of the launch) or 0 (every later one) plus
    the plies since -- so an env's lengths sum to counter + index of its last done ply, counted from 1.  Workgroup b
    holds envs [b * group, (b + 1) * group) and adds to replica row b % REPLICAS."""
    meta = meta.astype(np.int64)
    done = ((meta >> lib.REC_DONE_BIT) & 1).astype(bool)
    won = done & (((meta >> lib.REC_REWARD_SHIFT) & 0xFF) == 1)
    white = ((meta >> lib.REC_SIDE_BIT) & 1).astype(bool)
    steps, nenv = meta.shape
    per_env = np.zeros((nenv, lib.STATS_COUNTERS), dtype=np.int64)
    per_env[:, 0] = done.sum(axis=0)
    per_env[:, 1] = (won & ~white).sum(axis=0)
    per_env[:, 2] = (won & white).sum(axis=0)
    per_env[:, 3] = (done & ~won).sum(axis=0)
    last = steps - np.argmax(done[::-1], axis=0)
    per_env[:, 4] = np.where(done.any(axis=0), moves_before.astype(np.int64) + last, 0)
    raw = np.zeros((lib.STATS_REPLICAS, lib.STATS_STRIDE), dtype=np.int64)
    np.add.at(raw, ((np.arange(nenv) // group) % lib.STATS_REPLICAS, slice(0, lib.STATS_COUNTERS)), per_env)
    return raw


def poke(target, pokes):
    for i, count in pokes:
        target.move_counts[i] = count


@functools.lru_cache(maxsize=None)
def oracle_launches(m, n, k, nenv, chunks, pokes):
    """the oracle's meta words and cumulative statistics of every launch: computed once per shape, shared by the forms"""
    ora = OracleVectorEnv(m, n, k, nenv)
    poke(ora, pokes)
    out, total, step0 = [], np.zeros(5, dtype=np.int64), 0
    for t in chunks:
        _, meta, stats = random_rollout(ora, seed=SEED, step0=step0, steps=t, env_id0=ENV_ID0)
        total = total + stats
        step0 += t
        out.append((meta, total))
    return out


def run_case(hip, form, m, n, k, nenv, chunks, pokes=(), jit=False):
    lib = hip.lib
    env_knobs, code, group = FORMS[form]
    want = oracle_launches(m, n, k, nenv, tuple(chunks), tuple(pokes))
    with knobs(lib, **env_knobs):
        env = hip.Env(m, n, k, nenv, device=DEV)
        poke(env, pokes)
        roll = hip.Rollout(env, seed=SEED, env_id0=ENV_ID0)
        for t, (meta, total) in zip(chunks, want):
            got_form = lib.rollout_form(nenv, m, n, k, t, True, 0)
            assert got_form & 0xF == getattr(lib, code), f"labelled {form}, runs {got_form:#x}"
            assert bool(got_form & lib.ROLLOUT_JIT) == jit, f"labelled {form}, runs {got_form:#x}"
            moves_before = env.move_counts.cpu().numpy()
            raw_before = roll._stats.cpu().numpy().copy()
            rec = roll.run(t)
            torch.cuda.synchronize()
            got_meta = rec.meta.cpu().numpy().view(np.uint32)
            gained = roll._stats.cpu().numpy() - raw_before
            assert np.array_equal(gained, gained_from_records(lib, got_meta, moves_before, group)), (form, nenv, t)
            assert np.array_equal(got_meta, meta), (form, nenv, t)
            assert np.array_equal(roll.stats.cpu().numpy(), total), (form, nenv, t)
            if t == 1 and not pokes:  # a game of one ply does not exist: no total may have been added
                assert not gained.any()


@pytest.mark.parametrize("form", ["lane", "pair"])
@pytest.mark.parametrize("plies", [1, 5, 64])
@pytest.mark.parametrize("nenv", [1, 37, 64, 65, 130])
def test_stats_equal_the_records_3x3x3(hip, nenv, plies, form):
    """3x3x3: games end every few plies and draws are frequent, so every counter moves in nearly every lane; two
    launches in a row add into the same ``stats``."""
    run_case(hip, form, 3, 3, 3, nenv, (plies, plies))


@pytest.mark.parametrize("form", ["lane", "pair", "pairw"])
@pytest.mark.parametrize("nenv", [37, 130])
def test_stats_equal_the_records_9x9x5(hip, nenv, form):
    run_case(hip, form, 9, 9, 5, nenv, (64,))


def test_stats_of_a_wave_on_the_general_loop(hip):
    """9x9x5, 130 envs on one lane each: env 70's ply counter is set ahead of its stones, so the second wave plays the
    general loop (its game "ends in a draw" by the counter); the other two waves play the FAST loop."""
    run_case(hip, "lane", 9, 9, 5, 130, (64,), pokes=((70, 30),))


@pytest.mark.parametrize("form,nenv", [("ws2", 1), ("ws4", 130)])
def test_stats_of_the_waves_per_group_forms(hip, form, nenv):
    """several waves carry the same 64 envs: one of them counts"""
    run_case(hip, form, 9, 9, 5, nenv, (64,))


@pytest.mark.parametrize("form", ["lane, compiled at run time", "lane, the generic kernel"])
def test_stats_on_a_board_of_two_words(hip, form):
    """6x7x4 has no ahead-of-time variant: the kernel hiprtc makes for it, and the generic one"""
    run_case(hip, form, 6, 7, 4, 70, (32,), jit="run time" in form)


def test_stats_of_the_largest_legal_launch(hip):
    """3x3x3, a full wave, 65 535 plies in one launch: the wave's 32-bit sums at their largest (some 6e5 games, 4e6
    plies).  Against the records, and the summed lengths also against the closed form the kernel uses per lane:
    counters before + plies played - counters after."""
    lib, nenv, plies = hip.lib, 64, 65535
    with knobs(lib, MNK_ROLLOUT_PAIR="0"):
        assert lib.rollout_form(nenv, 3, 3, 3, plies, True, 0) & 0xF == lib.ROLLOUT_LANE
        env = hip.Env(3, 3, 3, nenv, device=DEV)
        roll = hip.Rollout(env, seed=SEED, env_id0=ENV_ID0)
        roll.run(5, record=False)  # mid-game counters at the start
        moves_before = env.move_counts.cpu().numpy()
        raw_before = roll._stats.cpu().numpy().copy()
        rec = roll.run(plies)
        torch.cuda.synchronize()
        gained = roll._stats.cpu().numpy() - raw_before
        assert np.array_equal(gained, gained_from_records(lib, rec.meta.cpu().numpy().view(np.uint32), moves_before, 64))
        moves_after = env.move_counts.cpu().numpy()
        assert int(gained[:, 4].sum()) == int(moves_before.sum()) + nenv * plies - int(moves_after.sum())
        assert int(gained[:, 0].sum()) > nenv * plies // 9
