"""Search self-play: PUCT plays itself on N boards in lockstep and fills a ``SearchReplayBuffer`` with outcome-labelled
records (AlphaZero / expert iteration; the rule: include/mnk_hip.h, mnk_search_selfplay_step).

A ply is ``PUCTSearchPolicy.act(visits=...)`` on the current roots, then one ``mnk_search_selfplay_step`` launch that
plays every row's move from its root visits (temperature 1 for the first ``temp_plies`` plies of a game, then 0), records
the position and the visits in the ring, labels the records of every game that ends, resets it and writes the next roots.
Nothing waits on the host: the ply counter is a device word (the buffer's ``plies``) that the search's sampler and the
step kernel both read, and one more tiny kernel advances it, so ``torch.cuda.graph`` can capture ``play(1)`` once the
buffers exist (after one eager ply) and the evaluator is capturable.

``root_noise=(alpha, eps)`` mixes Dirichlet noise into every root's priors (``PUCTSearchPolicy(root_noise=...)``, the rule:
include/mnk_hip.h, mnk_puct_root_noise).  The sampler's step is the ring's ply counter, so the noise of ply p is a function
of (seed, row id, p) alone: a restored ``state_dict`` and every replay of a captured ``play(1)`` draw what an eager run
draws.  (An evaluator wrapper can still perturb the roots' call -- the first of every ``evaluations_per_act`` -- from a
generator of its own, without any of that: examples/alphazero_selfplay.py keeps one.)

``leaves=L`` searches with L leaves per row and evaluator call (``PUCTSearchPolicy(leaves=L)``): ``iterations / L + 1``
calls per ply on batches of ``num_envs * L`` rows.

``reuse=True`` keeps every row's search tree from ply to ply (``PUCTSearchPolicy(reuse=True)``): the next root that the step
kernel writes is what the next search matches its stored tree against, so the subtree of the move that was played -- drawn
by temperature or not -- is carried over and a game that was reset starts fresh, with no word from the host.

``solver=True`` searches with exact proofs of wins, draws and losses (``PUCTSearchPolicy(solver=True)``, the rule:
include/mnk_hip.h, mnk_puct_step_solver).  The step kernel is the same: it plays from, and records, the visits it is
given, which are then the adjusted ones -- the ring's policy targets carry no count of a move proven to lose, and only the
proven wins where there is one.

``gumbel=m`` searches with a Gumbel root (``PUCTSearchPolicy(gumbel=m)``, the rule: include/mnk_hip.h,
mnk_puct_step_gumbel) and plays through ``mnk_search_selfplay_step_moves``: the move is the search's own -- a sample from
the improved policy, drawn at the ring's ply counter like the noise -- and the ring's u16 visits are that policy scaled to
65 535, which ``mnk_search_gather`` turns back into the target.  ``temp_plies`` is then not read.

``fpu=r`` or ``fpu=(r, r_root)`` searches with first-play urgency (``PUCTSearchPolicy(fpu=...)``, the rule:
include/mnk_hip.h, mnk_puct_step_fpu): a move without a visit is valued at its parent's mean value less a reduction, not
at 0, so a root that looks lost still concentrates its visits -- and its policy target -- on few moves.

``forced=k`` searches with forced playouts and policy target pruning (``PUCTSearchPolicy(forced=k)``, the rule:
include/mnk_hip.h, mnk_puct_step_forced): with ``root_noise`` a move the noise promotes is tried more than once, and the
visits that PUCT alone would not have spent are taken out of the counts the step kernel plays from and records.

``AsyncSearchSelfPlay`` (below) is the same loop without the lockstep: one launch per evaluator call, a search budget per
row and ply, rows that play on as soon as their search is done.  It takes ``root_noise`` and ``solver`` too, built into
its one launch (``mnk_search_selfplay_advance_opts``): the noise of a row's ply is a function of (seed, row id, the row's
ply count), and a row whose root is proven plays at once instead of idling until the slowest row is done.  ``keep_tree=True`` is its
``reuse`` (``mnk_search_selfplay_advance_keep``): the launch that plays a row's ply carries the played move's subtree into
the row's next search.  ``leaves=L`` is its ``leaves`` (``mnk_search_selfplay_advance_leaves``): L positions per row and
evaluator call, a ply's budget counted in the simulations it has been offered, with ``root_noise`` and ``solver``.
``gumbel=m`` is its ``gumbel`` (``mnk_search_selfplay_advance_gumbel``): the Gumbel draw of a row's ply is made inside the
launch that backs its root up, and a fast ply plays a sample of the improved policy of its small search.
"""
from typing import Dict

import torch

import mnk_hip
from alg.search_replay_buffer import SearchReplayBuffer
from env.torch_vector_mnk_env import TorchVectorMnkEnv
from selfplay.policy import PUCTSearchPolicy


class SearchSelfPlay:
    def __init__(self, m: int, n: int, k: int, num_envs: int, model=None, evaluator=None, iterations: int = 64,
                 c: float = 1.25, temp_plies: int = None, capacity: int = None, seed=None, leaf_dtype=torch.float32,
                 device="cuda", reuse: bool = False, tree_nodes: int = None, leaves: int = 1, root_noise=None,
                 solver: bool = False, gumbel: int = None, gumbel_c=(50.0, 0.5), gumbel_scale: float = 1.0,
                 fpu=None, forced=None):
        self.m, self.n, self.k, self.num_envs = int(m), int(n), int(k), int(num_envs)
        C = self.m * self.n
        self.temp_plies = C // 4 if temp_plies is None else int(temp_plies)
        if self.temp_plies < 0:
            raise ValueError(f"temp_plies must be >= 0, got {temp_plies}")
        if self.num_envs < 1:
            raise ValueError(f"num_envs must be >= 1, got {num_envs}")
        if not mnk_hip.geometry_supported(self.m, self.n, self.k) or self.n < 2:
            raise ValueError(f"unsupported board {self.m}x{self.n} (k={self.k})")
        capacity = 2 * C if capacity is None else int(capacity)
        if capacity < C:
            raise ValueError(f"capacity must be at least m*n = {C} plies, got {capacity}")
        # (the policy checks model / evaluator, iterations, c, leaves, root_noise, fpu, forced and leaf_dtype before anything
        # touches the GPU)
        self.policy = PUCTSearchPolicy(self.k, model=model, evaluator=evaluator, iterations=iterations, c=c,
                                       temperature=0, leaf_dtype=leaf_dtype, seed=seed, reuse=reuse, tree_nodes=tree_nodes,
                                       leaves=leaves, root_noise=root_noise, solver=solver, gumbel=gumbel,
                                       gumbel_c=gumbel_c, gumbel_scale=gumbel_scale, fpu=fpu, forced=forced)
        self.env = TorchVectorMnkEnv(self.m, self.n, self.k, self.num_envs, device=device)
        dev = self.env._dev
        self.buffer = SearchReplayBuffer(capacity, self.num_envs, self.m, self.n, dev)
        self.sampler = self.policy._sampler
        self.sampler.step_dev = self.buffer.plies  # the search and the step both draw at the ply counter
        self.env.reset()
        self.obs = torch.empty((self.num_envs, 2, self.m, self.n), dtype=torch.float32, device=dev)
        self.mask = torch.empty((self.num_envs, C), dtype=torch.bool, device=dev)
        self.env.observe_into(obs=self.obs, mask=self.mask)  # a fresh board: black to move, absolute = canonical
        self.visits = torch.zeros((self.num_envs, C), dtype=torch.int32, device=dev)
        # reuse: {nodes kept, the kept root's visit count} of every row in the last ply's search ({0, 0}: it began afresh)
        self.carried = torch.zeros((self.num_envs, 2), dtype=torch.int32, device=dev) if reuse else None
        # gumbel: the search's improved policy, what mnk_search_selfplay_step_moves records
        self.target = (torch.zeros((self.num_envs, C), dtype=torch.float32, device=dev)
                       if self.policy.gumbel is not None else None)
        self.stats = torch.zeros((mnk_hip.STATS_REPLICAS, mnk_hip.STATS_STRIDE), dtype=torch.int64, device=dev)
        self._ones = torch.ones(1, dtype=torch.int64, device=dev)

    def play(self, plies: int = 1) -> None:
        """``plies`` self-play plies on every board; enqueues work only"""
        env, buf = self.env, self.buffer
        stream = mnk_hip.stream_ptr(env._dev)
        for _ in range(int(plies)):
            if self.target is not None:
                self._ply_gumbel(stream)
                continue
            self.policy.act({"observation": self.obs, "action_mask": self.mask}, visits=self.visits, carried=self.carried)
            seed, seed_dev, step, step_dev, env_id0, _ = self.sampler.block()
            mnk_hip.call("mnk_search_selfplay_step", mnk_hip.ptr(env._planes), mnk_hip.ptr(env._meta), self.num_envs,
                         self.m, self.n, self.k, mnk_hip.ptr(self.visits), self.temp_plies, seed, seed_dev, step, step_dev,
                         env_id0, buf.capacity, mnk_hip.ptr(buf.planes), mnk_hip.ptr(buf.visits), mnk_hip.ptr(buf.z),
                         mnk_hip.ptr(self.obs), mnk_hip.OBS_F32, mnk_hip.ptr(self.mask), mnk_hip.ptr(self.stats),
                         mnk_hip.ptr(env._err), stream)
            buf.plies.add_(self._ones)
            buf.plies_host += 1

    def _ply_gumbel(self, stream) -> None:
        """one ply of a search with a Gumbel root: the search's own move and its improved policy go to the step"""
        env, buf = self.env, self.buffer
        actions = self.policy.act({"observation": self.obs, "action_mask": self.mask}, visits=self.visits,
                                  policy=self.target)
        _, _, step, step_dev, _, _ = self.sampler.block()
        mnk_hip.call("mnk_search_selfplay_step_moves", mnk_hip.ptr(env._planes), mnk_hip.ptr(env._meta), self.num_envs,
                     self.m, self.n, self.k, mnk_hip.ptr(self.target), mnk_hip.ptr(actions), step, step_dev, buf.capacity,
                     mnk_hip.ptr(buf.planes), mnk_hip.ptr(buf.visits), mnk_hip.ptr(buf.z), mnk_hip.ptr(self.obs),
                     mnk_hip.OBS_F32, mnk_hip.ptr(self.mask), mnk_hip.ptr(self.stats), mnk_hip.ptr(env._err), stream)
        buf.plies.add_(self._ones)
        buf.plies_host += 1

    def reset_trees(self) -> None:
        """``reuse=True``: forget the kept trees, so that the next ply searches every row afresh -- for after the
        evaluator's weights changed (``PUCTSearchPolicy.reset_tree``)"""
        self.policy.reset_tree()

    def note_replayed(self, plies: int) -> None:
        """a captured graph of ``play`` has been replayed for ``plies`` plies in all: the host's count of written plies
        (what ``buffer.sample`` checks for emptiness) follows; the device counter advanced by itself"""
        self.buffer.plies_host += int(plies)

    def pop_game_stats(self) -> Dict[str, float]:
        """games finished since the last call: games, black wins, white wins, draws and mean length (one sync)"""
        tot = self.stats.sum(dim=0).tolist()
        self.stats.zero_()
        self.env.check_errors()
        games = int(tot[0])
        return {"games": games, "black_wins": int(tot[1]), "white_wins": int(tot[2]), "draws": int(tot[3]),
                "mean_length": tot[4] / games if games else 0.0}

    def state_dict(self) -> Dict[str, object]:
        """env, ring, ply counter and Philox key: a restored run continues bit-exactly with ``reuse=False``.  The kept
        trees of ``reuse=True`` are not part of the state: ``load_state_dict`` drops them, and the plies after it search
        afresh where the run that was saved had carried visits"""
        return {"env": self.env.state_dict(), "buffer": self.buffer.state_dict(), "seed": self.sampler.seed,
                "temp_plies": self.temp_plies, "stats": self.stats.cpu()}

    def load_state_dict(self, state: Dict[str, object]) -> None:
        self.env.load_state_dict(state["env"])
        self.buffer.load_state_dict(state["buffer"])
        self.sampler.seed = int(state["seed"])
        self.temp_plies = int(state["temp_plies"])
        self.stats.copy_(state["stats"])
        self.reset_trees()
        self.env.observe_into(obs=self.obs, mask=self.mask, flip_side=(self.env._meta & 1).to(torch.int64))


class AsyncSearchSelfPlay:
    """Search self-play with a search budget per row and ply (the rule: include/mnk_hip.h, mnk_search_selfplay_advance).

    ``SearchSelfPlay`` moves every row in lockstep: ``iterations + 1`` evaluator calls, then one ply of every row.  Here
    a round is one evaluator call on every row's leaf and ONE launch that backs the evaluation up and, row by row,
    either selects the next leaf or -- when the row's budget for its ply is spent -- plays the ply, records it, labels and
    resets a finished game and starts the search of the position reached, whose root is the row's leaf of the next round.
    Rows finish their searches at different times and go on at once, so plies can have different budgets ("playout cap
    randomisation"): a ply is searched with ``iterations`` with probability ``full_prob`` and becomes a policy and value
    target, and with ``fast_iterations`` otherwise, when its ring record carries zero visits -- ``SearchReplayBuffer``'s
    gather then hands out an all-zero policy for it -- and is a value target only.  Which plies are full is a function of
    (seed, row id, the row's ply count) alone (``mnk_hip.STREAM_BUDGET``).  With ``full_prob=1`` (the default) and
    ``fast_iterations=None`` (= ``iterations``), ``P * (iterations + 1)`` rounds leave exactly what
    ``SearchSelfPlay(same seed).play(P)`` leaves, with two launches fewer per ply.

    ``row_plies`` (int64 ``[N]``) holds the plies every row has played since construction; row i's next record goes to
    ring slot ``row_plies[i] % capacity``.  ``fresh`` (uint8 ``[N]``) tells which rows of ``leaf_obs`` / ``leaf_mask`` --
    the batch the next evaluator call sees -- are roots: an evaluator that perturbs root priors reads it, there is no
    "first call of an act" any more.  ``buffer.plies`` is the ply count of the most advanced row (a device word the
    kernel keeps), which is what ``buffer.sample`` draws below: a slot a slower row has not written yet holds an unknown
    outcome, weight 0.  ``buffer.plies_host`` advances by one per round: an upper bound of that count, exact only in
    what ``sample`` uses it for -- whether anything was launched at all.  During the first ``fast_iterations + 1`` rounds
    no row has played a ply yet and ``buffer.plies`` is still 0 while ``plies_host`` is not: a ``sample()`` in that window
    is not refused as empty, every id it draws wraps to the ring's last slot, and that slot holds an unknown outcome, so
    the whole batch has weight 0 -- harmless to a weighted loss, and over once the first ply is played.

    ``root_noise=(alpha, eps)`` mixes Dirichlet noise into the priors a fresh tree's root stores -- the draw and the mix
    of ``PUCTSearchPolicy(root_noise=...)`` (the rule: include/mnk_hip.h, mnk_puct_root_noise), made inside the launch
    that backs the root's evaluation up, keyed by (seed, row id, the row's ply count).  The evaluator's tensor is not
    written and no torch op is added to a round.  By default only the roots of full plies are noised (the fast searches
    only move the game on and play at full strength, as KataGo's do); ``noise_on_fast=True`` noises every root.
    ``root_priors`` (float32 ``[N, C]``) then shows, for every row, the priors its current root holds: a row is written
    by the launch that backs up its root's evaluation, noised or not.  With every ply full the games are those of
    ``SearchSelfPlay(root_noise=...)`` of the same seed, bit for bit.

    ``solver=True`` searches with exact proofs (``PUCTSearchPolicy(solver=True)``, the rule: include/mnk_hip.h,
    mnk_puct_step_solver) and ends a row's ply as soon as its root is proven: the row plays from the adjusted counts --
    which are also what a full ply records -- and starts its next search in the same launch, where the lockstep player
    would idle until the ply of the slowest row ends.

    ``keep_tree=True`` is ``SearchSelfPlay``'s ``reuse``: a row keeps the subtree of the move it played (the rule:
    include/mnk_hip.h, mnk_search_selfplay_advance_keep), carried over inside the launch that plays the ply, so a fast ply
    searches ``fast_iterations`` on top of what the searches before it left there.  The budget of a ply counts the
    iterations of that ply, not the root's total visits, and with every ply full the games are those of
    ``SearchSelfPlay(reuse=True, tree_nodes=...)`` of the same seed, bit for bit.  ``tree_nodes`` is the workspace's node
    capacity per row (default ``2 * iterations + 1``, ``PUCTSearchPolicy``'s range); a ply carries at most ``tree_nodes -
    iterations`` nodes over, the oldest first.  ``carried`` (int32 ``[N, 2]``) holds {nodes kept, the kept root's visit
    count} of every row's current search, {0, 0} for one that began afresh.  ``reset_trees()`` drops the kept trees --
    for after the evaluator's weights changed.  With the solver a carried root keeps the proof it had as a child and
    plays in the launch that renews it.

    ``leaves=L`` is ``SearchSelfPlay``'s ``leaves``: every row shows the evaluator L positions per call (the rule:
    include/mnk_hip.h, mnk_search_selfplay_advance_leaves), so a round is one evaluator call on ``num_envs * L`` rows --
    slot j of row i is row ``i * L + j`` of ``leaf_obs`` / ``leaf_mask`` -- and one launch that backs a row's pending slots
    up and selects up to L new leaves under virtual visits.  ``iterations`` must be a multiple of L; ``fast_iterations``
    need not be: a ply of budget B is offered exactly B simulations in ``ceil(B / L) + 1`` rounds, the slots beyond the
    budget staying void (they show the root and nothing is read for them).  ``row_sims`` (int32 ``[N]``) counts the
    simulations every row's current ply has been offered -- the budget is held against it, not against the root's visits,
    so that a slot the search itself leaves void counts as it does for the lockstep player.  ``fresh[i]`` then says that
    slot 0 of row i -- batch row ``i * L`` -- is a root, and ``root_priors`` stays ``[N, C]``.  With every ply full the games
    are those of ``SearchSelfPlay(leaves=L, ...)`` of the same seed, bit for bit, with ``root_noise`` too.  It takes
    ``root_noise`` and ``solver``; with ``keep_tree`` it raises ``ValueError``.

    ``gumbel=m`` is ``SearchSelfPlay``'s ``gumbel``: every root is a Gumbel root (the rule: include/mnk_hip.h,
    mnk_search_selfplay_advance_gumbel).  The launch that backs a fresh tree's root up draws the root's Gumbel variables
    -- ``PUCTSearchPolicy(gumbel=m)``'s draw, keyed by (seed, row id, the row's ply count) -- into ``gscore`` (float32
    ``[N, C]``) and keeps the root's value in ``vroot`` (float32 ``[N]``); the selections follow Sequential Halving with
    the schedule of the ply's own budget (two tables, one for ``iterations`` and one for ``fast_iterations``, uploaded
    once), and the launch that ends the ply plays the search's own move.  A full ply records the improved policy scaled
    to 65 535, a fast ply zero visits as before -- but its move is still a sample of the improved policy of a
    ``fast_iterations`` search, which a visit-count search of that size cannot give.  ``gumbel_c=(c_visit, c_scale)`` and
    ``gumbel_scale`` are ``PUCTSearchPolicy``'s.  ``temp_plies`` is accepted and not read: the Gumbel draw is the
    exploration at every ply, as in the lockstep player.  With every ply full the games are those of
    ``SearchSelfPlay(gumbel=m)`` of the same seed, bit for bit.  With ``root_noise``, ``solver``, ``keep_tree`` or
    ``leaves > 1`` it raises ``ValueError``, the lockstep player's rule.  ``state_dict`` needs nothing new for it: the
    trees are not state, and the ``gscore`` that the search restarted by ``load_state_dict`` redraws is a function of
    (seed, row id, ply count), so it is the one the interrupted search had.

    ``fpu=r`` or ``fpu=(r, r_root)`` is ``SearchSelfPlay``'s ``fpu``: first-play urgency in every selection (the rule:
    include/mnk_hip.h, mnk_puct_step_fpu), with ``root_noise``, ``solver`` and ``keep_tree``.  ``advance`` then calls
    ``mnk_search_selfplay_advance_opts_fpu``, under ``keep_tree`` ``mnk_search_selfplay_advance_keep_fpu``; with every ply
    full the games are those of ``SearchSelfPlay(fpu=..., same options)`` of the same seed, bit for bit (the solver
    excepted, as above).  With ``leaves > 1`` or ``gumbel`` it raises ``ValueError``.

    ``forced=k`` is ``SearchSelfPlay``'s ``forced``: forced playouts at the root and policy target pruning where the ply is
    played (the rule: include/mnk_hip.h, mnk_puct_step_forced and mnk_search_selfplay_advance_opts_forced), on exactly the
    plies the built-in noise applies to -- the full plies, and the fast ones too under ``noise_on_fast=True`` -- with or
    without ``root_noise``, ``solver`` and ``fpu``.  A ply that does not force is searched, played and recorded as without
    the option; a full ply records the pruned counts.  ``advance`` then calls ``mnk_search_selfplay_advance_opts_forced``;
    with every ply full the games are those of ``SearchSelfPlay(forced=k, same options)`` of the same seed, bit for bit
    (the solver excepted, as above).  With ``keep_tree``, ``leaves > 1`` or ``gumbel`` it raises ``ValueError`` (DESIGN
    section 10).

    With no option ``advance`` calls ``mnk_search_selfplay_advance``, as before; with ``root_noise`` or ``solver`` it
    calls ``mnk_search_selfplay_advance_opts``; with ``keep_tree`` it calls ``mnk_search_selfplay_advance_keep``, which
    takes the other two; with ``leaves > 1`` it calls ``mnk_search_selfplay_advance_leaves``, which takes ``root_noise``
    and ``solver``; with ``gumbel`` it calls ``mnk_search_selfplay_advance_gumbel``."""

    def __init__(self, m: int, n: int, k: int, num_envs: int, model=None, evaluator=None, iterations: int = 64,
                 fast_iterations: int = None, full_prob: float = 1.0, c: float = 1.25, temp_plies: int = None,
                 capacity: int = None, seed=None, leaf_dtype=torch.float32, device="cuda", root_noise=None,
                 noise_on_fast: bool = False, solver: bool = False, keep_tree: bool = False, tree_nodes: int = None,
                 leaves: int = 1, gumbel: int = None, gumbel_c=(50.0, 0.5), gumbel_scale: float = 1.0, fpu=None,
                 forced=None):
        self.m, self.n, self.k, self.num_envs = int(m), int(n), int(k), int(num_envs)
        C = self.m * self.n
        self.temp_plies = C // 4 if temp_plies is None else int(temp_plies)
        if self.temp_plies < 0:
            raise ValueError(f"temp_plies must be >= 0, got {temp_plies}")
        if self.num_envs < 1:
            raise ValueError(f"num_envs must be >= 1, got {num_envs}")
        if not mnk_hip.geometry_supported(self.m, self.n, self.k) or self.n < 2:
            raise ValueError(f"unsupported board {self.m}x{self.n} (k={self.k})")
        capacity = 2 * C if capacity is None else int(capacity)
        if capacity < C:
            raise ValueError(f"capacity must be at least m*n = {C} plies, got {capacity}")
        self.keep_tree = bool(keep_tree)
        # (the policy checks model / evaluator, iterations, c, leaf_dtype, leaves -- its range, and that iterations is a
        # multiple of it -- and tree_nodes -- its range, and that it comes with keep_tree; it lends its evaluator call, its
        # key, its workspace and its leaf tensors, both sized for `leaves`, and is never asked to act)
        self.policy = PUCTSearchPolicy(self.k, model=model, evaluator=evaluator, iterations=iterations, c=c,
                                       temperature=0, leaf_dtype=leaf_dtype, seed=seed, reuse=self.keep_tree,
                                       tree_nodes=tree_nodes, leaves=leaves)
        self.leaves = self.policy.leaves
        if self.leaves > 1 and self.keep_tree:
            raise ValueError("keep_tree does not combine with leaves > 1 yet")
        self.iterations = self.policy.iterations
        self.tree_nodes = self.policy.tree_nodes  # (iterations + 1 without keep_tree)
        self.fast_iterations = self.iterations if fast_iterations is None else int(fast_iterations)
        if not 1 <= self.fast_iterations <= self.iterations:
            raise ValueError(f"fast_iterations must lie in [1, iterations] = [1, {self.iterations}], got {fast_iterations}")
        self.full_prob = float(full_prob)
        if not 0.0 <= self.full_prob <= 1.0:
            raise ValueError(f"full_prob must lie in [0, 1], got {full_prob}")
        self.full_threshold = int(round(self.full_prob * 2.0 ** 32))  # a ply is full iff its u32 lies below
        self.root_noise = PUCTSearchPolicy._checked_root_noise(root_noise)
        self.noise_on_fast = bool(noise_on_fast)
        if self.noise_on_fast and self.root_noise is None:
            raise ValueError("noise_on_fast=True needs root_noise=(alpha, eps)")
        self.solver = bool(solver)
        self.gumbel, self.gumbel_c, self.gumbel_scale = PUCTSearchPolicy._checked_gumbel(gumbel, gumbel_c, gumbel_scale)
        if self.gumbel is not None:
            for name, on in (("keep_tree=True", self.keep_tree), ("leaves > 1", self.leaves > 1),
                             ("solver=True", self.solver), ("root_noise", self.root_noise is not None)):
                if on:
                    raise ValueError(f"gumbel does not combine with {name} yet")
        self.fpu = PUCTSearchPolicy._checked_fpu(fpu)
        if self.fpu is not None:
            if self.gumbel is not None:
                raise ValueError("fpu does not combine with gumbel yet")
            if self.leaves > 1:
                raise ValueError("fpu does not combine with leaves > 1 in the per-row loop yet")
        self.forced = PUCTSearchPolicy._checked_forced(forced)
        if self.forced is not None:
            for name, on in (("gumbel", self.gumbel is not None), ("keep_tree=True", self.keep_tree),
                             ("leaves > 1", self.leaves > 1)):
                if on:
                    raise ValueError(f"forced does not combine with {name} in the per-row loop yet")
        self.env = TorchVectorMnkEnv(self.m, self.n, self.k, self.num_envs, device=device)
        dev = self.env._dev
        self.buffer = SearchReplayBuffer(capacity, self.num_envs, self.m, self.n, dev)
        self.sampler = self.policy._sampler
        self.env.reset()
        # gumbel: every row's root scores and root value (written by the launch that backs its root's evaluation up), and
        # the schedules of considered visits of the two budgets, uploaded once
        self.gscore = self.vroot = self._table_full = self._table_fast = None
        if self.gumbel is not None:
            self.gscore = torch.zeros((self.num_envs, C), dtype=torch.float32, device=dev)
            self.vroot = torch.zeros(self.num_envs, dtype=torch.float32, device=dev)
            table = mnk_hip.puct_gumbel_schedule(self.gumbel, self.iterations)
            self._table_full = torch.from_numpy(table.view("int16")).to(dev)
            self._table_fast = self._table_full
            if self.fast_iterations != self.iterations:
                table = mnk_hip.puct_gumbel_schedule(self.gumbel, self.fast_iterations)
                self._table_fast = torch.from_numpy(table.view("int16")).to(dev)
        self.row_plies = torch.zeros(self.num_envs, dtype=torch.int64, device=dev)
        self.fresh = torch.zeros(self.num_envs, dtype=torch.uint8, device=dev)
        self.stats = torch.zeros((mnk_hip.STATS_REPLICAS, mnk_hip.STATS_STRIDE), dtype=torch.int64, device=dev)
        self._roots = torch.empty((self.num_envs, 2, self.m, self.n), dtype=torch.float32, device=dev)
        self.workspace, self.leaf_obs, self.leaf_mask, _ = self.policy._buffers(self.num_envs, self.m, self.n, dev)
        # root_noise: the priors every row's current root holds (written by the launch that backs its evaluation up)
        self.root_priors = (torch.zeros((self.num_envs, C), dtype=torch.float32, device=dev)
                            if self.root_noise is not None else None)
        # keep_tree: {nodes kept, the kept root's visit count} of every row's current search ({0, 0}: it began afresh)
        self.carried = torch.zeros((self.num_envs, 2), dtype=torch.int32, device=dev) if self.keep_tree else None
        # leaves > 1: the simulations every row's current ply has been offered (the kernel's u32 words)
        self.row_sims = torch.zeros(self.num_envs, dtype=torch.int32, device=dev) if self.leaves > 1 else None
        self._begin()

    def _begin(self) -> None:
        """every row's search starts afresh on its current position (mnk_puct_begin; with ``leaves > 1``,
        mnk_puct_begin_leaves): the roots are the next leaves, in slot 0 of every row"""
        env = self.env
        env.observe_into(obs=self._roots, flip_side=(env._meta & 1).to(torch.int64))
        if self.leaves > 1:
            mnk_hip.call("mnk_puct_begin_leaves", mnk_hip.ptr(self._roots), mnk_hip.OBS_F32, self.num_envs, self.m, self.n,
                         self.k, self.iterations, self.leaves, mnk_hip.ptr(self.workspace), mnk_hip.ptr(self.leaf_obs),
                         self.policy._leaf_code, mnk_hip.ptr(self.leaf_mask), mnk_hip.stream_ptr(env._dev))
            self.row_sims.zero_()
        else:
            mnk_hip.call("mnk_puct_begin", mnk_hip.ptr(self._roots), mnk_hip.OBS_F32, self.num_envs, self.m, self.n,
                         self.k, self.tree_nodes - 1, mnk_hip.ptr(self.workspace), mnk_hip.ptr(self.leaf_obs),
                         self.policy._leaf_code, mnk_hip.ptr(self.leaf_mask), mnk_hip.stream_ptr(env._dev))
        self.fresh.fill_(1)
        if self.carried is not None:
            self.carried.zero_()

    def reset_trees(self) -> None:
        """``keep_tree=True``: forget the kept trees, so that every row's current search starts afresh on its position --
        for after the evaluator's weights changed"""
        self._begin()

    def advance(self, rounds: int = 1) -> None:
        """``rounds`` times: the evaluator on ``leaf_obs`` / ``leaf_mask``, then the kernel.  Enqueues work only;
        ``torch.cuda.graph`` can capture it after one eager round when the evaluator is capturable"""
        env, buf, N, C = self.env, self.buffer, self.num_envs, self.m * self.n
        stream = mnk_hip.stream_ptr(env._dev)
        for _ in range(int(rounds)):
            priors, pcode, values, vcode = self.policy._evaluate(self.leaf_obs, self.leaf_mask, N * self.leaves, C)
            seed, seed_dev, _, _, env_id0, _ = self.sampler.block()
            head = (mnk_hip.ptr(self.workspace), mnk_hip.ptr(env._planes), mnk_hip.ptr(env._meta), N, self.m, self.n,
                    self.k, self.iterations, self.fast_iterations)
            tail = (self.full_threshold, mnk_hip.ptr(priors), pcode,
                    mnk_hip.ptr(values), vcode, self.policy.c, self.temp_plies, seed, seed_dev, env_id0,
                    mnk_hip.ptr(self.row_plies), buf.capacity, mnk_hip.ptr(buf.planes), mnk_hip.ptr(buf.visits),
                    mnk_hip.ptr(buf.z), mnk_hip.ptr(self.leaf_obs), self.policy._leaf_code, mnk_hip.ptr(self.leaf_mask),
                    mnk_hip.ptr(self.fresh), mnk_hip.ptr(buf.plies), mnk_hip.ptr(self.stats), mnk_hip.ptr(env._err))
            args = head + tail
            if self.gumbel is not None:  # (no temp_plies: argument 15 of the plain entry point)
                mnk_hip.call("mnk_search_selfplay_advance_gumbel", *args[:15], *args[16:], self.gumbel, *self.gumbel_c,
                             self.gumbel_scale, mnk_hip.ptr(self._table_full), mnk_hip.ptr(self._table_fast),
                             mnk_hip.ptr(self.gscore), mnk_hip.ptr(self.vroot), stream)
            elif self.leaves > 1:
                alpha, eps = self.root_noise or (0.0, 0.0)
                mnk_hip.call("mnk_search_selfplay_advance_leaves", *head, self.leaves, *tail, int(self.solver), alpha, eps,
                             int(self.noise_on_fast), mnk_hip.ptr(self.root_priors), mnk_hip.ptr(self.row_sims), stream)
            elif self.forced is not None:
                alpha, eps = self.root_noise or (0.0, 0.0)
                mnk_hip.call("mnk_search_selfplay_advance_opts_forced", *args, int(self.solver), alpha, eps,
                             int(self.noise_on_fast), mnk_hip.ptr(self.root_priors), *(self.fpu or (0.0, 0.0)),
                             int(self.fpu is not None), self.forced, stream)
            elif self.fpu is not None:
                alpha, eps = self.root_noise or (0.0, 0.0)
                opts = (*args, int(self.solver), alpha, eps, int(self.noise_on_fast), mnk_hip.ptr(self.root_priors))
                if self.keep_tree:
                    mnk_hip.call("mnk_search_selfplay_advance_keep_fpu", *opts, self.tree_nodes - 1,
                                 self.tree_nodes - self.iterations, mnk_hip.ptr(self.carried), *self.fpu, stream)
                else:
                    mnk_hip.call("mnk_search_selfplay_advance_opts_fpu", *opts, *self.fpu, stream)
            elif self.keep_tree:
                alpha, eps = self.root_noise or (0.0, 0.0)
                mnk_hip.call("mnk_search_selfplay_advance_keep", *args, int(self.solver), alpha, eps,
                             int(self.noise_on_fast), mnk_hip.ptr(self.root_priors), self.tree_nodes - 1,
                             self.tree_nodes - self.iterations, mnk_hip.ptr(self.carried), stream)
            elif self.root_noise is None and not self.solver:
                mnk_hip.call("mnk_search_selfplay_advance", *args, stream)
            else:
                alpha, eps = self.root_noise or (0.0, 0.0)
                mnk_hip.call("mnk_search_selfplay_advance_opts", *args, int(self.solver), alpha, eps,
                             int(self.noise_on_fast), mnk_hip.ptr(self.root_priors), stream)
            buf.plies_host += 1

    def note_replayed(self, rounds: int) -> None:
        """a captured graph of ``advance`` has been replayed for ``rounds`` rounds in all: the host's count follows"""
        self.buffer.plies_host += int(rounds)

    def pop_game_stats(self) -> Dict[str, float]:
        """games finished since the last call: games, black wins, white wins, draws and mean length (one sync)"""
        tot = self.stats.sum(dim=0).tolist()
        self.stats.zero_()
        self.env.check_errors()
        games = int(tot[0])
        return {"games": games, "black_wins": int(tot[1]), "white_wins": int(tot[2]), "draws": int(tot[3]),
                "mean_length": tot[4] / games if games else 0.0}

    def state_dict(self) -> Dict[str, object]:
        """env, ring, every row's ply count, the Philox key, ``temp_plies`` and the statistics.  The trees are not state:
        ``load_state_dict`` starts every row's current search afresh, and since the budget of a ply is a function of (key,
        row id, ply count) the search that starts again gets the budget the interrupted one had -- and, with
        ``root_noise``, which is a function of the same three, redraws the noise the interrupted one had.  With
        ``keep_tree`` that search starts without the subtree the interrupted one was carried with (``carried`` is zero
        after ``load_state_dict``)"""
        return {"env": self.env.state_dict(), "buffer": self.buffer.state_dict(), "row_plies": self.row_plies.cpu(),
                "seed": self.sampler.seed, "temp_plies": self.temp_plies, "stats": self.stats.cpu()}

    def load_state_dict(self, state: Dict[str, object]) -> None:
        self.env.load_state_dict(state["env"])
        self.buffer.load_state_dict(state["buffer"])
        self.row_plies.copy_(state["row_plies"])
        self.sampler.seed = int(state["seed"])
        self.temp_plies = int(state["temp_plies"])
        self.stats.copy_(state["stats"])
        self._begin()
