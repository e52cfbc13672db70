"""Policies with the reference's ``act(obs, deterministic=False) -> (B,) int64`` contract
(``/root/reference/src/selfplay/policy.py:7-54``), drawing through the HIP sampler.

``RandomPolicy``   uniform over the legal cells (policy.py:13-29) -- the masked draw over a zero
                   logit row in ``mnk_sample_logits``; as a wrapper opponent it is recognised
                   (``fused_uniform_random``) and the whole self-play step becomes one launch.
``NNPolicy``       the reference's network policy, unchanged in behaviour: the net applies
                   its own mask and ``Categorical`` (policy.py:32-54).
``TacticalPolicy`` the one-ply tactical player, an opponent of fixed, known strength: take a win, else block one, else
                   play at random (``mnk_sample_tactical``); as a wrapper opponent it is folded into the one-launch step
                   (``mnk_selfplay_step_tactical``) like ``RandomPolicy``.
``MonteCarloPolicy`` the flat Monte Carlo player: for every legal cell P uniformly random playouts to the end of the game,
                   then a cell of best wins-minus-losses (``mnk_sample_playouts``); strength set by P, no training.  As a
                   wrapper opponent it goes through pre -> act -> post like any policy.
``PUCTSearchPolicy`` AlphaZero-style search on a policy/value evaluator (a trained net): one launch per evaluation
                   backs up the last one and selects the next leaves (``mnk_puct_step``); root visit counts as policy
                   targets; capturable in a graph.  As a wrapper opponent it goes through pre -> act -> post.
``SearchPolicy``   the tree-search player (UCT): I iterations of selection, expansion, B random playouts from the leaf
                   and backup, then a root child of most visits (``mnk_sample_search``); strength set by I, no training;
                   hands out the root visit counts per cell.  As a wrapper opponent it goes through pre -> act -> post.
``FusedNNPolicy``  same distribution, but mask + softmax + draw run in ``mnk_sample_logits``
                   on the raw logits (the epilogue of cnn.py:69-79 fused with the sample).  As a wrapper opponent it is
                   recognised (``fused_logits``): the wrapper asks it for its logits only and the draw happens INSIDE
                   ``mnk_selfplay_post_logits`` -- same stream of random numbers, one launch fewer per step.
"""
import ctypes
import math
from abc import ABC, abstractmethod
from typing import Dict

import torch
import torch.nn as nn

import mnk_hip


class Policy(ABC):
    @abstractmethod
    def act(self, obs: Dict[str, torch.Tensor], deterministic: bool = False) -> torch.Tensor:
        pass


_GOLDEN = 0x9E3779B97F4A7C15
_instances = [0]  # samplers created so far in this process


def _mix64(x: int) -> int:
    """splitmix64 finaliser: a bijection on 64-bit integers with good avalanche"""
    x &= 0xFFFFFFFFFFFFFFFF
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    return x ^ (x >> 31)


def default_key(seed=None) -> int:
    """Philox key of a sampler.  With an explicit ``seed`` the key IS the seed (reproducible, what the tests use).
    Without one -- the reference's constructors take no seed (policy.py:14, :33) -- every sampler created in the
    process gets its own key, derived from ``torch.initial_seed()`` and a per-process instance counter: two
    unseeded policies (agent and opponent of the same net, two RandomPolicy instances) must not draw the same
    uniform for row i on call c.  ``torch.manual_seed`` before constructing the policies makes a run repeatable."""
    if seed is not None:
        return int(seed) & 0xFFFFFFFFFFFFFFFF
    _instances[0] += 1
    return _mix64(int(torch.initial_seed()) + _instances[0] * _GOLDEN)


class _HipSampler:
    """Philox-keyed draws from masked logits on the mask's device."""

    def __init__(self, seed=None):
        self.seed = default_key(seed)
        self.calls = 0
        self.step_dev = None  # optional device int64[1] added to the step counter (graph replays)
        self.seed_dev = None  # optional device int64[1] that REPLACES the key (a captured sampler that can be re-keyed)
        self.env_id0 = 0      # Philox row id of row 0

    def block(self, deterministic=False):
        """the sampler's part of the argument list of mnk_sample_logits / mnk_selfplay_*_logits (after logits, dtype,
        mask): seed, seed_dev, step, step_dev, env_id0, deterministic"""
        return (self.seed, mnk_hip.ptr(self.seed_dev), self.calls, mnk_hip.ptr(self.step_dev), self.env_id0,
                1 if deterministic else 0)

    def advance(self):
        """one draw has been made with ``block()``"""
        if self.step_dev is None:
            self.calls += 1

    @staticmethod
    def prepare(logits, mask):
        """(logits contiguous f32 / bf16 [B, C] or None, MNK_LOGITS_* code, mask contiguous bool / u8 [B, C])"""
        mask = mask.contiguous()
        if mask.device.type != "cuda":
            raise RuntimeError("mnk policies sample on the GPU; got a mask on " + str(mask.device))
        if mask.dim() == 1:
            mask = mask.unsqueeze(0)
        if mask.dtype != torch.bool and mask.dtype != torch.uint8:
            mask = mask != 0
        b, c = mask.shape
        dtype = mnk_hip.LOGITS_F32
        if logits is not None:
            if logits.dtype == torch.bfloat16:
                dtype = mnk_hip.LOGITS_BF16
            elif logits.dtype != torch.float32:
                logits = logits.to(torch.float32)
            logits = logits.reshape(b, c).contiguous()
        return logits, dtype, mask

    def draw(self, logits, mask, deterministic, want_logp=False):
        """logits: f32 / bf16 [B, C] (bf16 is read as is -- what a network emits under autocast, alg/ppo.py:194),
        or None for all-zero logits (a uniform draw over the legal cells that reads only the mask)."""
        logits, dtype, mask = self.prepare(logits, mask)
        b, c = mask.shape
        actions = torch.empty(b, dtype=torch.long, device=mask.device)
        logp = torch.empty(b, dtype=torch.float32, device=mask.device) if want_logp else None
        if b:
            mnk_hip.call("mnk_sample_logits", mnk_hip.ptr(logits), dtype, mnk_hip.ptr(mask), b, c, *self.block(deterministic),
                         mnk_hip.ptr(actions), mnk_hip.ptr(logp), mnk_hip.stream_ptr(mask.device))
        self.advance()
        return (actions, logp) if want_logp else actions


HipSampler = _HipSampler


class RandomPolicy(Policy):
    fused_uniform_random = True  # lets TorchSelfPlayWrapper fold the opponent into its step kernel

    def __init__(self, action_dim: int, seed=None):
        self.action_dim = action_dim
        self._sampler = _HipSampler(seed)

    def act(self, obs: Dict[str, torch.Tensor], deterministic: bool = False) -> torch.Tensor:
        # all logits zero: uniform over the legal cells; deterministic: argmax of the 0/1 weights = first legal
        # cell (policy.py:26-27).  No logits tensor is materialised -- the kernel reads the mask only.
        return self._sampler.draw(None, obs["action_mask"], deterministic)


class TacticalPolicy(Policy):
    """The one-ply tactical player for k-in-a-row (the rule: include/mnk_hip.h, mnk_sample_tactical): a cell that
    completes its own run of ``k`` if there is one, else a cell where the other side would complete one, else a uniformly
    random legal cell -- the draw is over the set that applies, in action order, from one Philox u32 per row
    (``deterministic``: its first cell).  Reads only the observation (channel 0 = the side to move, any of float32 /
    bfloat16 / uint8; the board size comes from its shape); the mask is not looked at.

    As the opponent of ``TorchSelfPlayWrapper`` the whole step is one launch (``fused_tactical``): the reply is drawn
    inside the step kernel from the wrapper's own key and stream OPP, like ``RandomPolicy``'s.  A subclass that
    overrides ``act`` is called as a policy instead."""

    fused_tactical = True  # lets TorchSelfPlayWrapper fold the opponent into its step kernel (only when act is this one)

    def __init__(self, k: int, seed=None):
        self.k = int(k)
        self._sampler = _HipSampler(seed)

    def act(self, obs: Dict[str, torch.Tensor], deterministic: bool = False, candidates=None) -> torch.Tensor:
        """``candidates``: optional uint8 / bool ``[B, m*n]`` tensor that receives the set each row drew from"""
        return _play(self._sampler, "mnk_sample_tactical", obs, (self.k,), deterministic,
                     "candidates", candidates, 1, (torch.uint8, torch.bool))


def folds_tactical(policy) -> bool:
    """does ``policy`` play as the built-in tactical opponent of the one-launch step?  Only a ``TacticalPolicy`` whose
    ``act`` is not overridden: a subclass that changes the moves goes through pre -> act -> post."""
    return getattr(policy, "fused_tactical", False) and type(policy).act is TacticalPolicy.act


def _canonical_observation(obs):
    """the observation of ``obs`` as a contiguous cuda [B, 2, m, n] tensor of float32 / bfloat16 / uint8"""
    observation = obs["observation"]
    if observation.dim() == 3:
        observation = observation.unsqueeze(0)
    if observation.device.type != "cuda":
        raise RuntimeError("mnk policies sample on the GPU; got an observation on " + str(observation.device))
    if observation.dtype not in (torch.float32, torch.bfloat16, torch.uint8):
        observation = observation.to(torch.float32)
    observation = observation.contiguous()
    if observation.dim() != 4 or observation.shape[1] != 2:
        raise ValueError(f"expected an observation [B, 2, m, n], got {tuple(observation.shape)}")
    return observation


def _play(sampler, entry, obs, args, deterministic, out_name, out, planes, out_dtypes):
    """one call of the player ``entry`` on the canonical observation of ``obs``: ``args`` are its arguments after m, n
    and before the sampler's; ``out`` (``out_name``), optional, is a contiguous ``[B, m*n]`` (``planes`` = 1) or
    ``[B, planes, m*n]`` tensor of one of ``out_dtypes`` on the observation's device.  Returns the actions."""
    observation = _canonical_observation(obs)
    b, _, m, n = observation.shape
    shape = (b, m * n) if planes == 1 else (b, planes, m * n)
    if out is not None and (out.shape != shape or out.dtype not in out_dtypes or not out.is_contiguous()
                            or out.device != observation.device):
        kinds = " / ".join(str(d).replace("torch.", "") for d in out_dtypes)
        raise ValueError(f"{out_name} must be a contiguous {kinds} {shape} tensor on {observation.device}")
    actions = torch.empty(b, dtype=torch.long, device=observation.device)
    if b:
        mnk_hip.call(entry, mnk_hip.ptr(observation), mnk_hip.obs_code(observation), b, m, n, *args,
                     *sampler.block(deterministic), mnk_hip.ptr(actions), mnk_hip.ptr(out),
                     mnk_hip.stream_ptr(observation.device))
    sampler.advance()
    return actions


class MonteCarloPolicy(Policy):
    """The flat Monte Carlo player for k-in-a-row (the rule: include/mnk_hip.h, mnk_sample_playouts): for every legal cell
    ``playouts`` games are played to the end from that move on, both sides drawing uniformly random legal cells; the move
    is drawn among the cells of maximal wins-minus-losses, in action order, from one Philox u32 per row (the u32
    ``TacticalPolicy`` draws; ``deterministic``: the first such cell).  A cell that wins at once scores ``playouts`` and is
    never missed.  Strength rises with ``playouts`` and needs no training: Random < Tactical < MC(16) < MC(64) < MC(256).
    Reads only the observation (channel 0 = the side to move, any of float32 / bfloat16 / uint8; the board size comes
    from its shape).  One launch per call, one workgroup per row.

    As the opponent of ``TorchSelfPlayWrapper`` it is called through pre -> act -> post like any policy; it is not folded
    into the one-launch step."""

    def __init__(self, k: int, playouts: int = 64, seed=None):
        self.k = int(k)
        self.playouts = int(playouts)
        if not 1 <= self.playouts <= mnk_hip.PLAYOUTS_MAX:
            raise ValueError(f"playouts must lie in [1, {mnk_hip.PLAYOUTS_MAX}], got {playouts}")
        self._sampler = _HipSampler(seed)

    def act(self, obs: Dict[str, torch.Tensor], deterministic: bool = False, counts=None) -> torch.Tensor:
        """``counts``: optional int32 ``[B, 2, m*n]`` tensor that receives each row's wins (``[:, 0]``) and losses
        (``[:, 1]``) per cell over its ``playouts`` games (draws = playouts - wins - losses; 0 on occupied cells)"""
        return _play(self._sampler, "mnk_sample_playouts", obs, (self.k, self.playouts), deterministic,
                     "counts", counts, 2, (torch.int32,))


class SearchPolicy(Policy):
    """The tree-search player for k-in-a-row (the rule: include/mnk_hip.h, mnk_sample_search): UCT with ``iterations``
    iterations per move, each of which expands one node (the first untried cell, in action order) or descends to the
    child of maximal ``q + c * sqrt(n_parent / n_child)``, plays ``playouts`` uniformly random games from the leaf and
    backs their outcomes up the path.  The move is drawn among the root children of most visits, in action order, from
    one Philox u32 per row (the u32 ``TacticalPolicy`` draws; ``deterministic``: the first such cell).  Strength rises with
    ``iterations`` and needs no training.  Reads only the observation (channel 0 = the side to move, any of float32 /
    bfloat16 / uint8; the board size comes from its shape).  One launch per call, one workgroup per row, the tree in LDS.

    As the opponent of ``TorchSelfPlayWrapper`` it is called through pre -> act -> post like any policy; it is not folded
    into the one-launch step."""

    def __init__(self, k: int, iterations: int = 256, playouts: int = 32, c: float = 0.05, seed=None):
        self.k = int(k)
        self.iterations = int(iterations)
        self.playouts = int(playouts)
        self.c = float(c)
        if not 1 <= self.iterations <= mnk_hip.SEARCH_ITERS_MAX:
            raise ValueError(f"iterations must lie in [1, {mnk_hip.SEARCH_ITERS_MAX}], got {iterations}")
        if not 1 <= self.playouts <= mnk_hip.SEARCH_PLAYOUTS_MAX:
            raise ValueError(f"playouts must lie in [1, {mnk_hip.SEARCH_PLAYOUTS_MAX}], got {playouts}")
        if not (math.isfinite(self.c) and 0.0 <= self.c <= 3.0e38):
            raise ValueError(f"c must be finite and >= 0, got {c}")
        self._sampler = _HipSampler(seed)

    def act(self, obs: Dict[str, torch.Tensor], deterministic: bool = False, stats=None) -> torch.Tensor:
        """``stats``: optional int32 ``[B, 3, m*n]`` tensor that receives each row's root visit counts (``[:, 0]``), and
        the wins (``[:, 1]``) and losses (``[:, 2]``) of the side to move through each cell; 0 on occupied cells and on
        cells the search never expanded"""
        return _play(self._sampler, "mnk_sample_search", obs, (self.k, self.iterations, self.playouts, self.c),
                     deterministic, "stats", stats, 3, (torch.int32,))


def model_evaluator(model: nn.Module):
    """the evaluator of a reference-style ``model(obs, mask) -> (dist, value)``: ``dist.probs`` and ``value.reshape(-1)``,
    under ``torch.no_grad()``.  (Under graph capture the model must build its distribution without argument validation,
    ``torch.distributions.Distribution.set_default_validate_args(False)``: the check is a host synchronisation.)"""

    def evaluate(leaf_obs, leaf_mask):
        with torch.no_grad():
            dist, value = model(leaf_obs, leaf_mask)
        return dist.probs, value.reshape(-1)

    return evaluate


class PUCTSearchPolicy(Policy):
    """The PUCT search player (the rule: include/mnk_hip.h, mnk_puct_step): AlphaZero-style search on top of a
    policy/value evaluator, ``iterations`` evaluations per move after the roots', batched over the rows.  Each iteration is
    one launch that backs up the previous evaluation and selects every row's next leaf (child of maximal
    ``q + c * P * sqrt(n_parent) / (1 + n_child)``), then one call of the evaluator on the whole batch of leaves.  The move
    is drawn among the root children of most visits (``temperature=0``; ``deterministic``: the first of them), or in
    proportion to the root visits (``temperature=1``), from one Philox u32 per row (the u32 ``TacticalPolicy`` draws).

    ``evaluator(leaf_obs, leaf_mask) -> (priors [N, m*n], values [N])``: ``leaf_obs`` is a canonical view ``[N, 2, m, n]``
    of ``leaf_dtype`` (channel 0 = the leaf's side to move), ``leaf_mask`` a bool ``[N, m*n]`` of its legal cells; priors
    and values in float32 or bfloat16, the value from the view of the leaf's side to move.  Priors are used as returned
    (not renormalised).  With ``model`` instead, ``model_evaluator(model)``.  The first evaluator call of every ``act`` is
    always on the roots (the rows of ``obs`` themselves): an evaluator that perturbs the priors of that call only has to
    count its calls modulo ``evaluations_per_act``.  The rows of terminal leaves are evaluated too (a fixed batch shape)
    and their outputs ignored.

    ``root_noise=(alpha, eps)`` mixes Dirichlet noise into every root's priors (the rule: include/mnk_hip.h,
    mnk_puct_root_noise): ``(1 - eps) * P + eps * eta`` on the root's free cells, ``eta ~ Dirichlet(alpha)`` over them,
    drawn from Philox keyed by (seed, row id, call) like the move -- the same noise however the rows are sharded, after a
    restored ``state_dict`` and in every replay of a captured ``act``.  One more launch per ``act``, after the roots'
    evaluation, into a float32 buffer of the policy's own: the evaluator's tensor is never written.  With ``reuse`` a
    carried root takes fresh priors every ``act`` and so fresh noise.  ``None`` (the default): no noise, no launch, no
    buffer.

    The tree and the leaf buffers are allocated on the first ``act`` and reused while (N, m, n, iterations) stay; after
    that an ``act`` allocates nothing of its own but its result and never synchronises with the host, so
    ``torch.cuda.graph`` can capture it (with a capturable evaluator).  As the opponent of ``TorchSelfPlayWrapper`` it is
    called through pre -> act -> post like any policy.

    ``reuse=True`` keeps each row's tree between calls (``mnk_puct_rebase`` in the place of ``mnk_puct_begin``): a row whose
    position is the stored root, or one or two plies on from it through children that exist, starts its search from the
    subtree of that position -- its visits are then the carried ones plus ``iterations`` -- and every other row (a reset
    game, an unrelated position, the first call) starts fresh.  The rule is by position, so self-play (the next root is
    one ply on) and a wrapper's opponent (two plies on) are the same call, and every ``act`` is the same launches.  The
    workspace holds ``tree_nodes`` nodes per row (default ``2 * iterations + 1``, at most ``PUCT_ITERS_MAX + 1``) of which
    an ``act`` carries at most ``tree_nodes - iterations`` over, the oldest first.  The first evaluator call of an
    ``act`` is still on the roots; on a carried root it only renews the root's priors.  The kept statistics come from the
    evaluator as it was: after its weights change, ``reset_tree()`` drops them -- whether stale visits matter is the
    caller's decision.

    ``leaves=L`` (1 .. ``PUCT_LEAVES_MAX``, a divisor of ``iterations``; default 1, the search above) selects L leaves per
    row before every evaluator call, each under a virtual loss for the ones selected before it in the round
    (``mnk_puct_step_leaves``): the evaluator is called ``evaluations_per_act = iterations / L + 1`` times on batches of
    ``N * L`` rows, rows ``i * L .. i * L + L - 1`` being row i's.  The first call is still the roots (row ``i * L``; the
    other rows of that call, like every slot a round could not fill, repeat the root and are ignored).  With ``reuse`` the
    workspace's ``tree_nodes - 1`` must be a multiple of L as well (the default is).

    ``solver=True`` proves wins, draws and losses in the tree ("MCTS-Solver"; the rule: include/mnk_hip.h,
    mnk_puct_step_solver): every node carries a proof, a move that ends the game is proven when its node is created, and
    the backup of a proven leaf proves what follows from it along the path -- a node with a winning move is lost for the
    player who moved into it, a node all of whose moves are proven is a win or a draw.  The selection leaves out moves
    proven to lose, a proven child costs no evaluation, a proven root stops searching, the visit counts handed out drop
    the proven losses (or everything but the proven wins), and the root value of a proven root is exactly +1, 0 or -1.
    Every step is then ``mnk_puct_step_solver``, at any ``leaves``, with or without ``reuse`` (a kept subtree keeps its
    proofs) and ``root_noise``; the evaluator sees the same batches.  With the solver the visits no longer sum to the
    number of iterations.  ``False`` (the default): the search above, launch for launch.

    ``gumbel=m`` (1 .. ``PUCT_CONSIDERED_MAX``) makes the root a Gumbel root ("Policy improvement by planning with
    Gumbel", Danihelka et al. 2022; the rule: include/mnk_hip.h, mnk_puct_step_gumbel): one Philox-keyed Gumbel variable
    per root move, the budget spent on the m best moves by Sequential Halving, the survivor played, and the improved
    policy ``softmax(ln P + sigma(completed q))`` handed out through ``act(policy=...)`` as the training target -- a
    search meant for small ``iterations``, where visit counts say little.  ``gumbel_c=(c_visit, c_scale)`` are sigma's
    constants (q lies in [-1, 1] here, hence 0.5 where the paper has 1) and ``gumbel_scale`` scales the Gumbel variables
    (0, which ``act(deterministic=True)`` passes: no randomness at all).  Below the root the search is the one above.  One
    more launch per ``act`` (the draw, after the roots' evaluation) and three buffers of the policy's own.  It does not
    combine with ``reuse``, ``leaves > 1``, ``solver``, ``root_noise`` or ``temperature=1`` yet (``ValueError``).
    ``None`` (the default): the search above, launch for launch, and nothing is allocated.

    ``fpu=r`` or ``fpu=(r, r_root)`` turns on first-play urgency (the rule: include/mnk_hip.h, mnk_puct_step_fpu).  The
    score above values a move without a visit at ``q = 0``, "an untried move is a draw": where every visited move looks
    lost the search then tries each remaining cell once before it returns to any, and where the first move looks won it
    never tries a second.  With ``fpu`` an untried move is valued at its parent's own mean value less ``r * sqrt(prior
    mass of the parent's visited moves)`` (``r_root`` at the root, ``r`` below it; not below -1) -- KataGo's and Leela's
    reduction; 0.2 is their usual value, and ``fpu=0`` still differs from ``None`` (the parent's value, not 0).  Every
    step is then ``mnk_puct_step_fpu``, at any ``leaves``, with or without ``reuse``, ``solver`` and ``root_noise``; the
    evaluator sees the same batch shapes.  It does not combine with ``gumbel`` yet (``ValueError``).  ``None`` (the
    default): the search above, launch for launch, and nothing is allocated.

    ``forced=k`` (a number, finite and > 0; KataGo's 2) turns on forced playouts and policy target pruning (Wu 2019,
    section 3.2; the rule: include/mnk_hip.h, mnk_puct_step_forced) -- what makes ``root_noise`` useful as a policy target
    at small ``iterations``.  At the root a visited child is selected before any other while its visits n satisfy ``n * n
    < k * P * (root visits - 1)``, so a move the noise promotes is tried more than once; where the move is made those
    visits are taken out again wherever PUCT alone would not have spent them (and a lone remaining visit is dropped), so
    ``visits`` -- the counts the move is drawn from -- no longer sum to ``iterations``.  ``act(raw_visits=...)`` hands out
    the counts before the pruning.  Every step is then ``mnk_puct_step_forced``, at any ``leaves``, with or without
    ``reuse``, ``solver``, ``root_noise`` and ``fpu``; no launch and no buffer is added.  It does not combine with
    ``gumbel`` (``ValueError``): Sequential Halving has its own allocation of the budget.  ``None`` (the default): the
    search above, launch for launch."""

    def __init__(self, k: int, model=None, evaluator=None, iterations: int = 256, c: float = 1.25, temperature: int = 0,
                 leaf_dtype=torch.float32, seed=None, reuse: bool = False, tree_nodes: int = None, leaves: int = 1,
                 root_noise=None, solver: bool = False, gumbel: int = None, gumbel_c=(50.0, 0.5),
                 gumbel_scale: float = 1.0, fpu=None, forced=None):
        if (model is None) == (evaluator is None):
            raise ValueError("PUCTSearchPolicy needs exactly one of model and evaluator")
        self.k = int(k)
        self.model = model
        if model is not None:
            model.eval()
        self.evaluator = evaluator if evaluator is not None else model_evaluator(model)
        self.iterations = int(iterations)
        self.c = float(c)
        self.temperature = temperature
        if not 1 <= self.iterations <= mnk_hip.PUCT_ITERS_MAX:
            raise ValueError(f"iterations must lie in [1, {mnk_hip.PUCT_ITERS_MAX}], got {iterations}")
        if not (math.isfinite(self.c) and 0.0 <= self.c <= 3.0e38):
            raise ValueError(f"c must be finite and >= 0, got {c}")
        if temperature not in (0, 1):
            raise ValueError(f"temperature must be 0 or 1, got {temperature}")
        self.leaves = int(leaves)
        if not 1 <= self.leaves <= mnk_hip.PUCT_LEAVES_MAX or self.leaves != leaves:
            raise ValueError(f"leaves must lie in [1, {mnk_hip.PUCT_LEAVES_MAX}], got {leaves}")
        if self.iterations % self.leaves:
            raise ValueError(f"iterations must be a multiple of leaves, got {iterations} and {leaves}")
        self.leaf_dtype = leaf_dtype
        self._leaf_code = mnk_hip.obs_dtype_code(leaf_dtype)  # (TypeError for anything but float32 / bfloat16 / uint8)
        self._sampler = _HipSampler(seed)
        self.reuse = bool(reuse)
        if self.reuse:
            self.tree_nodes = 2 * self.iterations + 1 if tree_nodes is None else int(tree_nodes)
            if not self.iterations + 1 <= self.tree_nodes <= mnk_hip.PUCT_ITERS_MAX + 1:
                raise ValueError(f"tree_nodes must lie in [iterations + 1, {mnk_hip.PUCT_ITERS_MAX + 1}] = "
                                 f"[{self.iterations + 1}, {mnk_hip.PUCT_ITERS_MAX + 1}], got {tree_nodes}"
                                 + (" (the default, 2 * iterations + 1)" if tree_nodes is None else ""))
            if (self.tree_nodes - 1) % self.leaves:
                raise ValueError(f"tree_nodes - 1 must be a multiple of leaves, got {self.tree_nodes} and {leaves}")
        else:
            if tree_nodes is not None:
                raise ValueError("tree_nodes is the workspace of a search that keeps its tree: it needs reuse=True")
            self.tree_nodes = self.iterations + 1
        self.root_noise = self._checked_root_noise(root_noise)
        self.solver = bool(solver)
        self.gumbel, self.gumbel_c, self.gumbel_scale = self._checked_gumbel(gumbel, gumbel_c, gumbel_scale)
        if self.gumbel is not None:
            for name, on in (("reuse=True", self.reuse), ("leaves > 1", self.leaves > 1), ("solver=True", self.solver),
                             ("root_noise", self.root_noise is not None), ("temperature=1", temperature == 1)):
                if on:
                    raise ValueError(f"gumbel does not combine with {name} yet")
        self.fpu = self._checked_fpu(fpu)
        if self.fpu is not None and self.gumbel is not None:
            raise ValueError("fpu does not combine with gumbel yet")
        self.forced = self._checked_forced(forced)
        if self.forced is not None and self.gumbel is not None:
            raise ValueError("forced does not combine with gumbel: Sequential Halving has its own allocation")
        self._bufs = None  # (key, workspace, leaf_obs, leaf_mask, noised priors or None)
        self._gumbel_bufs = None  # gumbel: (key, table, gscore, vroot)

    @staticmethod
    def _checked_root_noise(root_noise):
        """None, or (alpha, eps) as floats: alpha finite and > 0 (as a float32 too), eps in [0, 1]"""
        if root_noise is None:
            return None
        try:
            alpha, eps = (float(x) for x in root_noise)
        except (TypeError, ValueError):
            raise ValueError(f"root_noise must be None or (alpha, eps), got {root_noise!r}") from None
        if not (math.isfinite(alpha) and alpha <= 3.0e38 and ctypes.c_float(alpha).value > 0.0):
            raise ValueError(f"root_noise: alpha must be finite and > 0 as a float32, got {alpha}")
        if not 0.0 <= eps <= 1.0:
            raise ValueError(f"root_noise: eps must lie in [0, 1], got {eps}")
        return alpha, eps

    @staticmethod
    def _checked_fpu(fpu):
        """None, or (fpu, fpu_root) as floats, each finite and >= 0 (as a float32 too); a number r stands for (r, r)"""
        if fpu is None:
            return None
        try:
            pair = tuple(float(x) for x in fpu) if hasattr(fpu, "__iter__") else (float(fpu),) * 2
            if len(pair) != 2 or isinstance(fpu, (bool, str)):
                raise ValueError
        except (TypeError, ValueError):
            raise ValueError(f"fpu must be None, a number or (fpu, fpu_root), got {fpu!r}") from None
        for x in pair:
            if not (math.isfinite(x) and 0.0 <= x <= 3.0e38):
                raise ValueError(f"fpu: the reductions must be finite and >= 0, got {fpu!r}")
        return pair

    @staticmethod
    def _checked_forced(forced):
        """None, or k as a float: finite and > 0 (as a float32 too)"""
        if forced is None:
            return None
        try:
            if isinstance(forced, (bool, str)):
                raise ValueError
            k = float(forced)
        except (TypeError, ValueError):
            raise ValueError(f"forced must be None or a number k > 0, got {forced!r}") from None
        if not (math.isfinite(k) and k <= 3.0e38 and ctypes.c_float(k).value > 0.0):
            raise ValueError(f"forced: k must be finite and > 0 as a float32, got {forced!r}")
        return k

    @staticmethod
    def _checked_gumbel(gumbel, gumbel_c, gumbel_scale):
        """(None or m, (c_visit, c_scale), gumbel_scale): m an int in [1, PUCT_CONSIDERED_MAX], the floats finite, >= 0"""
        try:
            c_visit, c_scale = (float(x) for x in gumbel_c)
            scale = float(gumbel_scale)
        except (TypeError, ValueError):
            raise ValueError(f"gumbel_c must be (c_visit, c_scale) and gumbel_scale a number, got {gumbel_c!r} and "
                             f"{gumbel_scale!r}") from None
        for name, x in (("gumbel_c: c_visit", c_visit), ("gumbel_c: c_scale", c_scale), ("gumbel_scale", scale)):
            if not (math.isfinite(x) and 0.0 <= x <= 3.0e38):
                raise ValueError(f"{name} must be finite and >= 0, got {x}")
        if gumbel is None:
            return None, (c_visit, c_scale), scale
        if isinstance(gumbel, bool) or gumbel != int(gumbel) or not 1 <= int(gumbel) <= mnk_hip.PUCT_CONSIDERED_MAX:
            raise ValueError(f"gumbel must be None or a number of moves in [1, {mnk_hip.PUCT_CONSIDERED_MAX}], got {gumbel!r}")
        return int(gumbel), (c_visit, c_scale), scale

    def _gumbel_buffers(self, b, c, device):
        key = (b, c, self.iterations, self.gumbel, device)
        if self._gumbel_bufs is None or self._gumbel_bufs[0] != key:
            table = mnk_hip.puct_gumbel_schedule(self.gumbel, self.iterations)
            self._gumbel_bufs = (key, torch.from_numpy(table.view("int16")).to(device),
                                 torch.empty((b, c), dtype=torch.float32, device=device),
                                 torch.empty(b, dtype=torch.float32, device=device))
        return self._gumbel_bufs[1:]

    @property
    def evaluations_per_act(self) -> int:
        """evaluator calls per ``act``: the roots', then one per round of ``leaves`` simulations"""
        return self.iterations // self.leaves + 1

    def _buffers(self, b, m, n, device):
        key = (b, m, n, self.iterations, self.tree_nodes, device)
        if self._bufs is None or self._bufs[0] != key:
            size = mnk_hip.puct_workspace_bytes(b, m, n, self.tree_nodes - 1, self.leaves)
            # (a tree that is kept starts as zeros: no row continues a workspace of zeros)
            self._bufs = (key, (torch.zeros if self.reuse else torch.empty)(size, dtype=torch.uint8, device=device),
                          torch.empty((b * self.leaves, 2, m, n), dtype=self.leaf_dtype, device=device),
                          torch.empty((b * self.leaves, m * n), dtype=torch.bool, device=device),
                          # (zeros: only the roots' rows are ever written, the step reads no other row of evaluation 0)
                          torch.zeros((b * self.leaves, m * n), dtype=torch.float32, device=device)
                          if self.root_noise is not None else None)
        return self._bufs[1:]

    def _evaluate(self, leaf_obs, leaf_mask, b, c):
        priors, values = self.evaluator(leaf_obs, leaf_mask)
        if priors.dtype not in (torch.float32, torch.bfloat16):
            priors = priors.to(torch.float32)
        if values.dtype not in (torch.float32, torch.bfloat16):
            values = values.to(torch.float32)
        priors, values = priors.reshape(b, c).contiguous(), values.reshape(b).contiguous()
        if priors.device != leaf_obs.device or values.device != leaf_obs.device:
            raise ValueError("the evaluator must return priors and values on the leaves' device")
        code = {torch.float32: mnk_hip.LOGITS_F32, torch.bfloat16: mnk_hip.LOGITS_BF16}
        return priors, code[priors.dtype], values, code[values.dtype]

    def reset_tree(self) -> None:
        """forget every row's tree (``reuse=True``): the next ``act`` starts every row fresh.  For after the evaluator's
        weights changed, when the caller wants no statistics of the old ones in the next searches"""
        if self._bufs is not None and self.reuse:
            self._bufs[1].zero_()

    def act(self, obs: Dict[str, torch.Tensor], deterministic: bool = False, visits=None, root_value=None,
            carried=None, proof=None, policy=None, raw_visits=None) -> torch.Tensor:
        """``visits``: optional int32 ``[B, m*n]`` tensor that receives each row's root visit counts (an AlphaZero policy
        target; they sum to ``iterations`` on a row with a legal cell, to the carried visits plus ``iterations`` on a row
        that kept its tree); ``root_value``: optional float32 ``[B]`` tensor that receives the root's mean value for the
        side to move; ``carried`` (``reuse=True``): optional int32 ``[B, 2]`` tensor that receives {nodes kept, the visit
        count of the root that was kept} of each row, {0, 0} where the row started fresh; ``proof`` (``solver=True``):
        optional int8 ``[B]`` tensor that receives +1, 0 or -1 where the root is a proven win, draw or loss for the side to
        move and ``mnk_hip.PROOF_UNKNOWN`` elsewhere.  With ``solver=True`` ``visits`` are the adjusted counts (the proven
        wins alone when there is one, else all but the proven losses) and do not sum to ``iterations``, and
        ``root_value`` is exactly +1, 0 or -1 on a proven root; ``policy`` (``gumbel=m``): optional float32 ``[B, m*n]``
        tensor that receives the improved policy (it sums to 1 over the free cells; 0 on occupied cells and on a row
        without a free cell).  With ``forced=k`` ``visits`` are the pruned counts, and ``raw_visits``: optional int32 ``[B,
        m*n]`` tensor that receives the counts before the pruning (what ``visits`` would be without it)"""
        if policy is not None and self.gumbel is None:
            raise ValueError("policy is an output of a search with a Gumbel root: it needs gumbel=m")
        if raw_visits is not None and self.forced is None:
            raise ValueError("raw_visits is an output of a search with forced playouts: it needs forced=k")
        observation = _canonical_observation(obs)
        b, _, m, n = observation.shape
        dev = observation.device
        if carried is not None and not self.reuse:
            raise ValueError("carried is an output of a search that keeps its tree: it needs reuse=True")
        if proof is not None and not self.solver:
            raise ValueError("proof is an output of a search that proves its tree: it needs solver=True")
        for name, t, shape, dtype in (("visits", visits, (b, m * n), torch.int32),
                                      ("root_value", root_value, (b,), torch.float32),
                                      ("carried", carried, (b, 2), torch.int32), ("proof", proof, (b,), torch.int8),
                                      ("policy", policy, (b, m * n), torch.float32),
                                      ("raw_visits", raw_visits, (b, m * n), torch.int32)):
            if t is not None and (t.shape != shape or t.dtype != dtype or not t.is_contiguous() or t.device != dev):
                raise ValueError(f"{name} must be a contiguous {str(dtype).replace('torch.', '')} {shape} tensor on {dev}")
        actions = torch.empty(b, dtype=torch.long, device=dev)
        if b and self.gumbel is not None:
            self._act_gumbel(observation, deterministic, actions, visits, root_value, policy)
        elif b:
            ws, leaf_obs, leaf_mask, noised = self._buffers(b, m, n, dev)
            stream = mnk_hip.stream_ptr(dev)
            I, k, code = self.iterations, self.k, self._leaf_code
            cap = self.tree_nodes - 1  # the workspace's layout parameter: node capacity - 1 (= I without reuse)
            # leaves = 1 stays on the entry points without the argument (the same results either way: include/mnk_hip.h)
            # (the solver's step takes `leaves` always, and the workspace the *_leaves entry points set up)
            # (so does the step with first-play urgency, which takes the solver as an argument)
            # (and the step with forced playouts, which takes both)
            sfx, lv = (("_leaves", (self.leaves,))
                       if self.leaves > 1 or self.solver or self.fpu is not None or self.forced is not None else ("", ()))
            step, out = ("mnk_puct_step_solver", (mnk_hip.ptr(proof),)) if self.solver else ("mnk_puct_step" + sfx, ())
            if self.fpu is not None:
                step, out = "mnk_puct_step_fpu", (mnk_hip.ptr(proof), int(self.solver), *self.fpu)
            if self.forced is not None:
                step, out = "mnk_puct_step_forced", (mnk_hip.ptr(proof), int(self.solver), *(self.fpu or (0.0, 0.0)),
                                                     int(self.fpu is not None), self.forced, mnk_hip.ptr(raw_visits))
            if self.reuse:
                mnk_hip.call("mnk_puct_rebase" + sfx, mnk_hip.ptr(observation), mnk_hip.obs_code(observation), b, m, n, k,
                             cap, self.tree_nodes - I, *lv, mnk_hip.ptr(ws), mnk_hip.ptr(leaf_obs), code,
                             mnk_hip.ptr(leaf_mask), mnk_hip.ptr(carried), stream)
            else:
                mnk_hip.call("mnk_puct_begin" + sfx, mnk_hip.ptr(observation), mnk_hip.obs_code(observation), b, m, n, k,
                             I, *lv, mnk_hip.ptr(ws), mnk_hip.ptr(leaf_obs), code, mnk_hip.ptr(leaf_mask), stream)
            rounds = I // self.leaves
            for it in range(rounds + 1):
                priors, pcode, values, vcode = self._evaluate(leaf_obs, leaf_mask, b * self.leaves, m * n)
                last = it == rounds
                if it == 0 and noised is not None:  # the roots' priors, noise mixed in, as f32 in the policy's buffer
                    mnk_hip.call("mnk_puct_root_noise", mnk_hip.ptr(priors), pcode, mnk_hip.ptr(leaf_mask), b, m * n,
                                 self.leaves, *self.root_noise, *self._sampler.block()[:5], mnk_hip.ptr(noised), stream)
                    priors, pcode = noised, mnk_hip.LOGITS_F32
                mnk_hip.call(step, mnk_hip.ptr(ws), b, m, n, k, cap, *lv, mnk_hip.ptr(priors), pcode,
                             mnk_hip.ptr(values), vcode, self.c, 1 if last else 0, self.temperature,
                             *self._sampler.block(deterministic), mnk_hip.ptr(leaf_obs), code, mnk_hip.ptr(leaf_mask),
                             mnk_hip.ptr(actions) if last else None, mnk_hip.ptr(visits) if last else None,
                             mnk_hip.ptr(root_value) if last else None, *out, stream)
        self._sampler.advance()
        return actions

    def _act_gumbel(self, observation, deterministic, actions, visits, root_value, policy):
        """the launches of an ``act`` with a Gumbel root: mnk_puct_begin_leaves, the roots' evaluation,
        mnk_puct_gumbel_root, then ``iterations + 1`` times mnk_puct_step_gumbel with an evaluation between them"""
        b, _, m, n = observation.shape
        dev = observation.device
        ws, leaf_obs, leaf_mask, _ = self._buffers(b, m, n, dev)
        table, gscore, vroot = self._gumbel_buffers(b, m * n, dev)
        stream = mnk_hip.stream_ptr(dev)
        I, k, code = self.iterations, self.k, self._leaf_code
        mnk_hip.call("mnk_puct_begin_leaves", mnk_hip.ptr(observation), mnk_hip.obs_code(observation), b, m, n, k, I, 1,
                     mnk_hip.ptr(ws), mnk_hip.ptr(leaf_obs), code, mnk_hip.ptr(leaf_mask), stream)
        for it in range(I + 1):
            priors, pcode, values, vcode = self._evaluate(leaf_obs, leaf_mask, b, m * n)
            last = it == I
            if it == 0:
                mnk_hip.call("mnk_puct_gumbel_root", mnk_hip.ptr(priors), pcode, mnk_hip.ptr(leaf_mask), mnk_hip.ptr(values),
                             vcode, b, m * n, 0.0 if deterministic else self.gumbel_scale, *self._sampler.block()[:5],
                             mnk_hip.ptr(gscore), mnk_hip.ptr(vroot), stream)
            mnk_hip.call("mnk_puct_step_gumbel", mnk_hip.ptr(ws), b, m, n, k, I, 1, mnk_hip.ptr(priors), pcode,
                         mnk_hip.ptr(values), vcode, self.c, 1 if last else 0, self.gumbel, *self.gumbel_c,
                         mnk_hip.ptr(table), mnk_hip.ptr(gscore), mnk_hip.ptr(vroot), *self._sampler.block(deterministic),
                         mnk_hip.ptr(leaf_obs), code, mnk_hip.ptr(leaf_mask), mnk_hip.ptr(actions) if last else None,
                         mnk_hip.ptr(visits) if last else None, mnk_hip.ptr(root_value) if last else None,
                         mnk_hip.ptr(policy) if last else None, stream)


class NNPolicy(Policy):
    def __init__(self, model: nn.Module):
        self.model = model
        self.model.eval()  # policy.py:35

    def act(self, obs: Dict[str, torch.Tensor], deterministic: bool = False) -> torch.Tensor:
        observation, action_mask = obs["observation"], obs["action_mask"]
        if observation.dim() == 3:  # policy.py:41-44
            observation = observation.unsqueeze(0)
        if action_mask.dim() == 1:
            action_mask = action_mask.unsqueeze(0)
        with torch.no_grad():
            dist, _ = self.model(observation, action_mask)
            return torch.argmax(dist.logits, dim=1) if deterministic else dist.sample()


class FusedNNPolicy(Policy):
    """``model(obs, None)`` must return ``(dist, value)`` with ``dist.logits`` the unmasked
    (possibly normalised) logits -- true for every reference architecture."""

    fused_logits = True  # lets TorchSelfPlayWrapper fold this opponent's draw into its post kernel

    def __init__(self, model: nn.Module, seed=None):
        self.model = model
        self.model.eval()
        self._sampler = _HipSampler(seed)

    def logits(self, obs: Dict[str, torch.Tensor]) -> torch.Tensor:
        """the raw logits of the policy head on ``obs`` (no mask, no draw): what the step kernels with a folded-in
        draw take (``mnk_selfplay_*_logits``)"""
        observation = obs["observation"]
        if observation.dim() == 3:
            observation = observation.unsqueeze(0)
        with torch.no_grad():
            dist, _ = self.model(observation, None)
            return dist.logits

    def act(self, obs: Dict[str, torch.Tensor], deterministic: bool = False) -> torch.Tensor:
        action_mask = obs["action_mask"]
        if action_mask.dim() == 1:
            action_mask = action_mask.unsqueeze(0)
        return self._sampler.draw(self.logits(obs), action_mask, deterministic)
