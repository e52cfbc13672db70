"""What the tests of the players on a canonical observation share (tactical, Monte Carlo, tree search): the ``hip``
fixture of the GPU modules and the ``lib`` fixture of the CPU ones, the positions they play on, the header / binding check
of an entry point and the match score of the strength ladders.  A plain module: the tests import from it."""
import os
import re
from typing import Callable, NamedTuple

import numpy as np
import pytest
import torch

import __graft_entry__ as entry
from playout_rule import playout_moves
from search_rule import search
from tactical_rule import random_positions

DEV = "cuda:0"
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mnk_hip.h")


@pytest.fixture(scope="module")
def lib():
    entry.build_hip()
    entry._ensure_path()
    import mnk_hip

    return mnk_hip


@pytest.fixture(scope="module")
def hip():
    entry.build_hip()
    entry._ensure_path()
    import mnk_hip
    from alg.rollout_buffer import RolloutBuffer
    from env.torch_vector_mnk_env import TorchVectorMnkEnv
    from selfplay import graphed, policy, tournament, validation
    from selfplay.torch_self_play_wrapper import TorchSelfPlayWrapper

    mnk_hip.load()
    assert torch.cuda.is_available()

    class NS:
        pass

    ns = NS()
    ns.lib, ns.Env, ns.Wrapper, ns.policy, ns.graphed, ns.validation, ns.tournament = (
        mnk_hip, TorchVectorMnkEnv, TorchSelfPlayWrapper, policy, graphed, validation, tournament)
    ns.Buffer = RolloutBuffer
    return ns


def board(rows):
    """canonical observation [1, 2, m, n] from strings: 'x' = side to move, 'o' = the other side, '.' = empty"""
    a = np.array([list(r) for r in rows])
    return np.stack([(a == "x"), (a == "o")]).astype(np.float32)[None]


def positions(m, n, k, count, seed, max_fill=1.0):
    """random positions, a quarter of them finished games (a run already on the board), an empty and a full board"""
    rng = np.random.default_rng(seed)
    live = random_positions(m, n, k, count - count // 4, rng, max_fill=max_fill)
    done = random_positions(m, n, k, count // 4, rng, max_fill=max_fill, stop_at_win=False)
    obs = np.concatenate([live, done])
    obs[0] = 0
    obs[1] = 0
    obs[1, 0].reshape(-1)[::2] = 1
    obs[1, 1].reshape(-1)[1::2] = 1
    return obs


def mostly_full(m, n, k, count, seed, fill=0.75):
    """positions filled to about ``fill``: a drawn board less stones taken off at random, either side to move (no run
    on the board); the last row a finished game, a run of the opponent along row 0.  For the boards on which the numpy
    rules take too long from positions with many free cells"""
    from puct_solver_cases import drawn_board  # (that module imports this one)

    rng, full = np.random.default_rng(seed), drawn_board(m, n, k)
    obs = np.zeros((count, 2, m, n), np.float32)
    for i in range(count):
        obs[i] = full[:: 1 if i % 2 else -1] & (rng.random((m, n)) < fill)
    obs[-1, 1, 0, :k], obs[-1, 0, 0, :k] = 1, 0
    return obs


def header_constants():
    return dict(re.findall(r"#define (MNK_\w+) (\d+)", open(HEADER).read()))


def check_header_and_binding(lib, name):
    """include/mnk_hip.h declares ``name`` with as many parameters as the binding's signature; the library exports it;
    ABI 6"""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert decl, name
    assert len([a for a in decl.group(1).split(",") if a.strip()]) == len(lib.SIGNATURES[name]), name
    assert hasattr(lib.load(), name)
    assert lib.load().mnk_abi_version() == 6 and lib.ABI_VERSION == 6


def _score(hip, p1, p2, board, games=1024):
    res = hip.tournament.play_match(p1, p2, board, games, device=DEV)
    assert res["wins"] + res["losses"] + res["draws"] == games
    return res["score"]


class Player(NamedTuple):
    """a player that runs one workgroup per row, as the shared GPU tests (test_gpu_players.py) see it: its policy class,
    the keyword and plane count of its int32 output tensor, its numpy rule, and the budget -- the arguments after k --
    each test plays it with"""
    policy: str
    out: str
    planes: int
    rule: Callable          # rule(obs, k, *budget, seed=, step=, deterministic=) -> (actions, ...)
    layout: tuple           # launch-layout independence
    keys: tuple             # device key words, on key_rows rows
    key_rows: int
    empty: tuple            # the policy of the empty-batch test; `full` for its full boards and the rule
    full: tuple
    bad_budgets: tuple      # budgets the constructor refuses
    opponent: tuple         # the wrapper's opponent; `validate` for validate_gpu
    validate: tuple
    captured: tuple         # the opponent switched in on a captured rollout

    def make(self, hip, k, budget, seed=None):
        return getattr(hip.policy, self.policy)(k, *budget, seed=seed)

    def act(self, hip, obs_np, k, budget, seed, step=0, env_id0=0, dtype=torch.float32, deterministic=False):
        """(actions, output tensor) of a fresh policy on call ``step``, as numpy"""
        b, _, m, n = obs_np.shape
        pol = self.make(hip, k, budget, seed)
        pol._sampler.calls, pol._sampler.env_id0 = step, env_id0
        out = torch.full((b, self.planes, m * n), -7, dtype=torch.int32, device=DEV)
        acts = pol.act({"observation": torch.from_numpy(obs_np).to(DEV).to(dtype)}, deterministic=deterministic,
                       **{self.out: out})
        return acts.cpu().numpy(), out.cpu().numpy()


MC = Player("MonteCarloPolicy", "counts", 2, playout_moves, layout=(24,), keys=(8,), key_rows=32, empty=(4,), full=(4,),
            bad_budgets=((0,), (4097,)), opponent=(8,), validate=(16,), captured=(6,))
SEARCH = Player("SearchPolicy", "stats", 3, search, layout=(48, 16, 1.0), keys=(32, 8, 1.0), key_rows=16, empty=(8, 4),
                full=(8, 4, 1.0), bad_budgets=((0,), (2049,)), opponent=(32, 8), validate=(64, 8), captured=(24, 8))
