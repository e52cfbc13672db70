"""GPU: every masked draw, one by one, against the float64 inverse CDF of tests/draw_rule.py.

The draw (``draw_row`` in csrc/mnk_draw.h) is a deterministic function of the row's logits, its mask and its uniform,
and the uniform is ``oracle.philox.uniform_open01`` of the row's Philox word -- so each draw of ``mnk_sample_logits`` and
of the step kernels that fold it in must be THE cell the float64 inverse CDF (lane-major walk) gives for that uniform,
unless the uniform lies within the derived f32 tolerance of a boundary (an "ambiguous" draw, which may take either
neighbour); its log-probability must be within the derived bound of the float64 one.  Deterministic draws are the argmax
over the legal cells, ties to the lowest cell, exactly.

Covered: every lanes-per-row shape and both sides of every bucket edge (row widths 1 ... 1024), f32 / bf16 / absent
logits, logits of any finite size (offsets up to 0.9 f32-max), peaked, flat, wide and tied rows, single-cell, one-residue
and all-masked rows, ragged last workgroups, the unaligned scalar staging path, uniforms within 2^-18 of 0 and of 1, and
the folded draw of ``wrapper.step_logits`` on the built-in boards and two run-time compiled ones."""
import os

import numpy as np
import pytest
import torch

import draw_rule as dr
import test_gpu_fused_draw as fd
from oracle.policies import LowestLegalPolicy

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

hip = fd.hip  # the module-scoped fixture of the fused-draw tests (library, env, wrapper, policies)

WIDTHS = [1, 2, 9, 24, 32, 33, 81, 96, 97, 144, 169, 225, 256, 257, 361, 484, 512, 513, 625, 961, 1024]
F32_MAX = float(np.finfo(np.float32).max)
AMBIGUOUS = []  # (case, ambiguous draws, draws): reported at the end of the module


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if AMBIGUOUS:
        worst = max(AMBIGUOUS, key=lambda r: r[1] / r[2])
        total = sum(r[1] for r in AMBIGUOUS), sum(r[2] for r in AMBIGUOUS)
        print(f"\nambiguous draws: {total[0]} of {total[1]} over {len(AMBIGUOUS)} cases; worst case {worst[0]}: "
              f"{worst[1]} of {worst[2]}")
        for case, a, n in AMBIGUOUS:
            print(f"  {case}: {a} / {n}")


def _masks(n, C, rng):
    """random density per row; every 16th row from 0 on has one legal cell at the first cell, from 1 on at the last,
    from 2 on at the last slot of lane 0, from 3 on legal cells in one residue class mod LPR only, from 4 on none"""
    lpr, _ = dr.shape(C)
    mask = rng.random((n, C)) < rng.uniform(0.05, 1.0, size=(n, 1))
    kind = np.arange(n) % 16
    cells = np.arange(C)
    mask[kind == 0] = cells == 0
    mask[kind == 1] = cells == C - 1
    mask[kind == 2] = cells == lpr * ((C - 1) // lpr)
    r3 = np.flatnonzero(kind == 3)
    res = rng.integers(0, lpr, size=len(r3)) % max(1, min(lpr, C))
    mask[r3] = (cells[None, :] % lpr == res[:, None]) & (rng.random((len(r3), C)) < 0.7)
    mask[r3, res] = True
    mask[kind == 4] = False
    return mask


def _logits(regime, n, C, rng):
    """f32 [n, C] logits of a regime (the caller rounds to bf16 where it tests bf16)"""
    if regime == "randn3":
        return rng.standard_normal((n, C)) * 3
    if regime == "peaked":
        x = rng.standard_normal((n, C))
        x[np.arange(n), rng.integers(0, C, n)] += 20.0
        return x
    if regime == "flat":
        return np.full((n, C), 1.25)
    if regime == "wide":
        return rng.standard_normal((n, C)) * 200
    if regime.startswith("offset"):
        return rng.standard_normal((n, C)) * 3 + float(regime[len("offset"):])
    if regime == "ties_int":
        return rng.integers(0, 4, (n, C)).astype(np.float64)
    if regime == "ties_bf16":
        return torch.from_numpy(rng.standard_normal((n, C)).astype(np.float32)).to(torch.bfloat16).float().numpy()
    if regime == "signed_zero":
        x = np.where(rng.random((n, C)) < 0.5, 0.0, -0.0)
        return np.where(rng.random((n, C)) < 0.2, -1.0, x)
    raise ValueError(regime)


# (regime, cells per case): the bulk of the draws on randn * 3; fewer for the extreme-offset and tie regimes
REGIMES = [("randn3", 1 << 22), ("peaked", 1 << 20), ("flat", 1 << 20), ("wide", 1 << 20),
           ("offset1e3", 1 << 17), ("offset-1e3", 1 << 17), ("offset1e6", 1 << 17), ("offset-1e6", 1 << 17),
           ("offset-1e9", 1 << 17), ("offset1e10", 1 << 17), ("offset-1e10", 1 << 17),
           (f"offset{0.9 * F32_MAX!r}", 1 << 17), (f"offset{-0.9 * F32_MAX!r}", 1 << 17),
           ("ties_int", 1 << 17), ("ties_bf16", 1 << 17), ("signed_zero", 1 << 17)]


def _device(x, dtype, unaligned=False):
    """numpy -> a contiguous cuda tensor of ``dtype``; ``unaligned``: one element past a 16-byte boundary"""
    t = torch.from_numpy(np.ascontiguousarray(x)).to(DEV).to(dtype)
    if not unaligned:
        return t
    flat = torch.empty(t.numel() + 1, dtype=dtype, device=DEV)
    view = flat[1:].view(t.shape)
    view.copy_(t)
    return view


def _draw_and_check(sampler, logits_t, mask_t, ref, case, few=False):
    """both draws of ``sampler`` on (logits_t, mask_t), each checked draw by draw against ``ref``; ``few``: a launch of a
    row or two, whose ambiguous share says nothing (the caller bounds the total)"""
    n = mask_t.shape[0]
    u = dr.row_uniforms(sampler.seed, sampler.env_id0, n, sampler.calls)
    act, logp = sampler.draw(logits_t, mask_t, False, want_logp=True)
    act, logp = act.cpu().numpy(), logp.cpu().numpy()
    bad, amb = dr.check(ref, act, logp, u)
    if bad.any():
        r = int(np.flatnonzero(bad)[0])
        a = int(np.clip(act[r], 0, ref.C - 1))
        exact, _ = ref.inverse_cdf(u)
        pytest.fail(f"{case}: {int(bad.sum())} of {n} draws wrong; row {r}: drew {act[r]} (logp {logp[r]!r}, p64 "
                    f"{ref.p[r, a]!r}, log p64 {ref.logp[r, a]!r}), float64 answer {exact[r]}, u {u[r]!r}, rowmax "
                    f"{ref.rowmax[r]!r}, legal {int(ref.legal[r].sum())}")
    assert few or amb.mean() < 0.02, (case, amb.mean())
    AMBIGUOUS.append((case, int(amb.sum()), n))
    act, logp = sampler.draw(logits_t, mask_t, True, want_logp=True)
    act, logp = act.cpu().numpy(), logp.cpu().numpy()
    bad, _ = dr.check(ref, act, logp)
    if bad.any():
        r = int(np.flatnonzero(bad)[0])
        pytest.fail(f"{case} (deterministic): {int(bad.sum())} of {n} draws wrong; row {r}: drew {act[r]} (logp "
                    f"{logp[r]!r}), argmax {ref.argmax()[r]}, rowmax {ref.rowmax[r]!r}")


@pytest.mark.parametrize("dtype", ["f32", "bf16", "none"])
@pytest.mark.parametrize("C", WIDTHS)
def test_sampler_draws_are_the_float64_inverse_cdf(hip, C, dtype):
    """``_HipSampler.draw``, stochastic and deterministic with log-probabilities, every regime: each draw against the
    float64 answer; the row count is odd, so the last workgroup is ragged"""
    rng = np.random.default_rng(1000 * C + {"f32": 0, "bf16": 1, "none": 2}[dtype])
    sampler = hip.policy._HipSampler(seed=C * 7 + 1)
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float32
    regimes = REGIMES if dtype != "none" else [("none", 1 << 22)]
    for regime, cells in regimes:
        n = max(cells // C, 512) | 1
        mask = _masks(n, C, rng)
        if dtype == "none":
            logits_t, lg = None, None
        else:
            logits_t = _device(_logits(regime, n, C, rng).astype(np.float32), tdt)
            lg = logits_t.float().cpu().numpy()  # what the kernel reads: f32, or bf16 widened exactly
        ref = dr.Reference(lg, mask)
        _draw_and_check(sampler, logits_t, torch.from_numpy(mask).to(DEV), ref, f"C={C} {dtype} {regime}")
    # the scalar staging path: logits and mask one element past a 16-byte boundary
    n = 257
    mask = _masks(n, C, rng)
    lg = None if dtype == "none" else _logits("randn3", n, C, rng).astype(np.float32)
    logits_t = None if lg is None else _device(lg, tdt, unaligned=True)
    mask_t = _device(mask, torch.bool, unaligned=True)
    assert logits_t is None or logits_t.data_ptr() % 16 != 0
    assert mask_t.data_ptr() % 16 != 0
    ref = dr.Reference(None if logits_t is None else logits_t.float().cpu().numpy(), mask)
    _draw_and_check(sampler, logits_t, mask_t, ref, f"C={C} {dtype} unaligned")


@pytest.mark.parametrize("dtype", ["f32", "none"])
@pytest.mark.parametrize("C", WIDTHS)
def test_draws_at_both_ends_of_the_uniform(hip, C, dtype):
    """rows keyed (``env_id0``) at Philox ids whose uniform lies within 2^-18 of 1 and of 0, found on the CPU from a
    fixed seed: the point u * total lands next to the total, where rounding can leave it beyond the last cell's
    cumulative weight (the kernel's fallback), and next to 0.  (The top Philox word gives u = 1.0 exactly:
    (2^24 - 1) + 0.5 rounds up in f32; the fallback takes the last cell with weight, the float64 answer for u = 1.)
    Draws near 1 are often ambiguous -- the last boundary lies within the tolerance of 1 whenever the last cell of the walk
    is improbable -- and are then held to legality, positive probability, the tolerance and the log-prob bound."""
    seed, step = 4321 + C, 6
    ids = np.concatenate([dr.find_row_ids(seed, step, 8, near_one=True), dr.find_row_ids(seed, step, 8, near_one=False)])
    rng = np.random.default_rng(C)
    sampler = hip.policy._HipSampler(seed=seed)
    regimes = ["randn3", "peaked", "flat", "wide"]
    for j, rid in enumerate(ids.tolist()):
        mask = _masks(16, C, rng)[[5 + j % 11]] if j % 4 else np.ones((1, C), bool)
        lg = None if dtype == "none" else _logits(regimes[j % 4], 1, C, rng).astype(np.float32)
        sampler.calls, sampler.env_id0 = step, rid
        ref = dr.Reference(lg, mask)
        _draw_and_check(sampler, None if lg is None else _device(lg, torch.float32), torch.from_numpy(mask).to(DEV), ref,
                        f"C={C} {dtype} row id {rid}", few=True)


# ----------------------------------------------------------------------------- the folded draw
@pytest.fixture()
def jit_api(hip):
    """every API kernel of a board without a built-in variant is compiled at its first launch (as in test_gpu_jit_api.py)"""
    saved = {k: os.environ.get(k) for k in ("MNK_JIT_API", "MNK_JIT")}
    os.environ["MNK_JIT_API"] = "1"
    hip.lib.reload_config()
    yield hip.lib
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    hip.lib.reload_config()


def _folded_steps(hip, m, n, k, nenv, opponent):
    """``wrapper.step_logits`` for a dozen steps: every agent draw against the float64 answer for the mask it was given,
    including one step whose legal logits are all -1e10 and one at -1e9 (the log-prob must be -log(n_legal) within the
    bound); moves legal, the env's error word clean"""
    c = m * n
    w = hip.Wrapper(hip.Env(m, n, k, nenv, device=DEV), seed=31)
    w.set_opponent(hip.policy.RandomPolicy(c, seed=5) if opponent == "random" else LowestLegalPolicy())
    sampler = hip.policy.HipSampler(seed=97 + c)
    obs, _ = w.reset()
    rng = np.random.default_rng(c + nenv)
    kinds = ["f32", "bf16", "none", "wide", "f32", "det", "-1e10", "-1e9", "bf16", "f32", "none", "det"]
    for t, kind in enumerate(kinds):
        mask = obs["action_mask"]
        mask_np = mask.cpu().numpy()
        if kind == "none":
            logits = None
        elif kind in ("-1e10", "-1e9"):
            logits = torch.full((nenv, c), float(kind), device=DEV)
        else:
            logits = _device(_logits("wide" if kind == "wide" else "randn3", nenv, c, rng).astype(np.float32),
                             torch.bfloat16 if kind == "bf16" else torch.float32)
        ref = dr.Reference(None if logits is None else logits.float().cpu().numpy(), mask_np)
        det = kind == "det"
        u = dr.row_uniforms(sampler.seed, sampler.env_id0, nenv, sampler.calls)
        obs, _, _, _, info = w.step_logits(logits, mask, sampler, deterministic=det)
        act, logp = info["actions"].cpu().numpy(), info["log_probs"].cpu().numpy()
        bad, amb = dr.check(ref, act, logp, None if det else u)
        case = f"{m}x{n}x{k} {opponent} step {t} {kind}"
        assert not bad.any(), (case, int(bad.sum()), np.flatnonzero(bad)[:5], act[bad][:5], logp[bad][:5])
        assert amb.mean() < 0.02, case
        if not det:
            AMBIGUOUS.append((case, int(amb.sum()), nenv))
        if kind in ("-1e10", "-1e9"):
            live = mask_np.any(axis=1)
            assert mask_np[live, act[live]].all(), case
            nl = mask_np.sum(axis=1)[live]
            assert np.all(np.isfinite(logp)), case
            assert np.all(np.abs(logp[live] + np.log(nl)) <= ref.logp_bound(act)[live]), case
    w.env.check_errors()


@pytest.mark.parametrize("opponent", ["random", "scripted"])
@pytest.mark.parametrize("m,n,k,nenv", [(3, 3, 3, 3001), (9, 9, 5, 4097), (13, 13, 5, 1001), (15, 15, 5, 1001),
                                        (19, 19, 5, 777)])
def test_folded_draws_are_the_float64_inverse_cdf(hip, m, n, k, nenv, opponent):
    """the agent's draw inside ``mnk_selfplay_step_random_logits`` (random opponent) / ``mnk_selfplay_pre_logits``
    (scripted opponent) on the boards with a built-in draw shape"""
    _folded_steps(hip, m, n, k, nenv, opponent)


@pytest.mark.parametrize("opponent", ["random", "scripted"])
@pytest.mark.parametrize("m,n,k,nenv", [(12, 12, 5, 1001), (22, 22, 5, 333)])
def test_folded_draws_of_run_time_compiled_boards(hip, jit_api, m, n, k, nenv, opponent):
    """the same on boards whose step kernels hiprtc specialises (``MNK_JIT_API=1``): 12x12 draws inside the specialised
    step kernel; 22x22 is checked on whichever path ``step_logits`` takes there"""
    lib = jit_api
    _folded_steps(hip, m, n, k, nenv, opponent)
    which = 2 if opponent == "random" else 0
    folded = [lib.jit_api_ready(m, n, k, lib.jit_api_draw_kind(which, dt)) for dt in (torch.float32, torch.bfloat16, None)]
    print(f"{m}x{n}x{k} {opponent}: draw folded into the step kernel: {folded}")
    if (m, n) == (12, 12):
        assert all(folded)
