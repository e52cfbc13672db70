"""Record the reference's traces of ``oracle/pin_against_reference.py`` as digests: ``pin_traces.npz``.

Run where the reference tree is present (see ``oracle/pin_against_reference.py``):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_pin.py

Every trace (state and outputs after every operation of the env, or after every step of the self-play wrapper) is stored
as one 64-bit digest per entry, so ``tests/test_oracle_golden.py`` pins the oracle to the reference without it:
  env_<i>, selfplay_<i>          ENV_CASES[:5] / SELFPLAY_CASES[:6]
  random_cases                   int64 [R, 5]: m, n, k, N, seed -- random geometries, drawn once here
  random_env_<j>, random_selfplay_<j>   their env trace (3 max(m, n) steps) and self-play trace (2 max(m, n) steps,
                                 opponent "random" for odd seeds, "hash" for even ones)
No reference source and no reference output other than these digests is stored.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle.pin_against_reference import (ENV_CASES, SELFPLAY_CASES, reference_available, reference_env_trace,  # noqa: E402
                                          reference_selfplay_trace, trace_digests)

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pin_traces.npz")
N_ENV, N_SELFPLAY, N_RANDOM = 5, 6, 12


def random_cases(count, seed=2024):
    """random board shapes, batch sizes and seeds: m, n in [2, 12], k in [1, 6] clipped to the board, N in [1, 24]"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        m, n = (int(v) for v in rng.integers(2, 13, 2))
        k = min(int(rng.integers(1, 7)), m, n)
        out.append((m, n, k, int(rng.integers(1, 25)), int(rng.integers(0, 10 ** 6))))
    return np.array(out, dtype=np.int64)


def random_selfplay_opponent(seed: int) -> str:
    return "random" if seed % 2 else "hash"


def main():
    if not reference_available():
        print("reference tree not present")
        return 1
    data = {}
    for i, case in enumerate(ENV_CASES[:N_ENV]):
        data[f"env_{i}"] = trace_digests(reference_env_trace(*case))
    for i, case in enumerate(SELFPLAY_CASES[:N_SELFPLAY]):
        data[f"selfplay_{i}"] = trace_digests(reference_selfplay_trace(*case))
    cases = random_cases(N_RANDOM)
    data["random_cases"] = cases
    for j, (m, n, k, nenv, seed) in enumerate(cases.tolist()):
        data[f"random_env_{j}"] = trace_digests(reference_env_trace(m, n, k, nenv, 3 * max(m, n), seed))
        data[f"random_selfplay_{j}"] = trace_digests(reference_selfplay_trace(m, n, k, nenv, 2 * max(m, n), seed,
                                                                              random_selfplay_opponent(seed)))
    np.savez_compressed(OUT, **data)
    print("wrote", OUT, sum(v.nbytes for v in data.values()), "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
