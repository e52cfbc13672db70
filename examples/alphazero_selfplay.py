"""AlphaZero on the HIP env: PUCT self-play into an outcome-labelled ring (``SearchSelfPlay``), minibatches with the
board's symmetries (``SearchReplayBuffer.sample``), the loss -sum(pi * log p) + (v - z)^2 weighted by ``weight`` (0 for
records of games still running), and validation of the greedy network against ``RandomPolicy`` and ``TacticalPolicy``.
Root noise is Dirichlet noise mixed into the priors of the first evaluator call of every search, the one on the roots:
``--noise wrapper`` (the default) draws it in an evaluator wrapper (``RootNoise``) from torch's generator, ``--noise
builtin`` in the search itself (``SearchSelfPlay(root_noise=...)``: Philox-keyed by seed, row and ply, so a run can be
restored, sharded and captured without changing a draw), ``--noise off`` plays without.  ``--reuse`` keeps every search
tree from ply to ply (the subtree of the move that was played starts the next search; the roots' priors, and so the noise,
are renewed every ply) and drops the trees after each training round, since their statistics are the old weights'.
``--solver`` proves wins, draws and losses inside the search (``SearchSelfPlay(solver=True)``): the policy targets drop
the moves proven to lose.  ``--search gumbel`` searches with a Gumbel root (``SearchSelfPlay(gumbel=m)``): the Gumbel draw
is the exploration (no root noise, no temperature) and the targets are the improved policy; the default ``puct`` is the
run it was.  ``--fast-iterations F --full-prob P`` (both) play through ``AsyncSearchSelfPlay``: a ply is searched with
``--iterations`` with probability P and is then a policy and value target, with F otherwise and is then a value target
only, and every row plays on as soon as its own search is done (playout cap randomisation); the wrapper's root noise then
goes to the rows the player marks ``fresh``.  They combine with ``--noise builtin`` (``AsyncSearchSelfPlay(root_noise=...)``:
the noise is drawn inside the player's one launch, on the roots of the full plies), with ``--solver`` (a row whose root
is proven plays at once) and with ``--reuse`` (``AsyncSearchSelfPlay(keep_tree=True)``: a fast ply searches on top of the
subtree the searches before it left; the trees are dropped after each training round here too) and with ``--leaves L``
(``AsyncSearchSelfPlay(leaves=L)``: the network sees envs * L positions per call and a ply of budget B takes ceil(B / L) +
1 calls; the wrapper's noise then goes to slot 0 of the fresh rows, batch row i * L); not ``--leaves`` with ``--reuse``.
They combine with ``--search gumbel`` too (``AsyncSearchSelfPlay(gumbel=m)``: the Gumbel draw is made inside the player's one
launch, a fast ply plays a sample of the improved policy of its small search, and a full ply records that policy; no root
noise, as in the lockstep run).

    python examples/alphazero_selfplay.py --board 3x3x3 --rounds 12 [--reuse] [--solver]
    python examples/alphazero_selfplay.py --board 3x3x3 --rounds 12 --search gumbel --iterations 16
    python examples/alphazero_selfplay.py --board 3x3x3 --rounds 12 --fast-iterations 8 --full-prob 0.25
    python examples/alphazero_selfplay.py --board 3x3x3 --rounds 12 --fast-iterations 8 --full-prob 0.25 --noise builtin --solver
    python examples/alphazero_selfplay.py --board 3x3x3 --rounds 12 --fast-iterations 8 --full-prob 0.25 --reuse
    python examples/alphazero_selfplay.py --board 3x3x3 --rounds 12 --fast-iterations 6 --full-prob 0.25 --leaves 4 --noise builtin --solver
    python examples/alphazero_selfplay.py --board 3x3x3 --rounds 12 --search gumbel --iterations 16 --fast-iterations 4 --full-prob 0.25
    python examples/alphazero_selfplay.py --board 3x3x3 --rounds 12 --fpu 0.2 [--fpu-root 0.1] [--fast-iterations 8 --full-prob 0.25]
    python examples/alphazero_selfplay.py --board 3x3x3 --rounds 12 --forced 2 --noise builtin [--fast-iterations 8 --full-prob 0.25]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rl-selfplay-mnk_amd")]

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

import __graft_entry__ as entry  # noqa: E402


class PolicyValueNet(nn.Module):
    """a small MLP with a policy head (masked logits) and a tanh value head: ``model(obs, mask) -> (dist, value)``"""

    def __init__(self, cells, width=128):
        super().__init__()
        self.body = nn.Sequential(nn.Flatten(), nn.Linear(2 * cells, width), nn.ReLU(), nn.Linear(width, width), nn.ReLU())
        self.pi, self.v = nn.Linear(width, cells), nn.Linear(width, 1)

    def logits(self, obs, mask=None):
        h = self.body(obs.float())
        logits = self.pi(h)
        if mask is not None:
            logits = logits.masked_fill(~mask.bool(), -1e9)
        return logits, torch.tanh(self.v(h)).reshape(-1)

    def forward(self, obs, mask=None):
        logits, v = self.logits(obs, mask)
        return torch.distributions.Categorical(logits=logits, validate_args=False), v


class RootNoise:
    """(1 - eps) * P + eps * Dirichlet(alpha) on the legal cells, in the first of every ``period`` evaluator calls (the
    roots of a search: ``PUCTSearchPolicy.evaluations_per_act`` = iterations / leaves + 1); the other calls pass through"""

    def __init__(self, inner, period, alpha=0.3, eps=0.25):
        self.inner, self.period, self.alpha, self.eps, self.calls = inner, period, alpha, eps, 0

    def __call__(self, leaf_obs, leaf_mask):
        priors, values = self.inner(leaf_obs, leaf_mask)
        root = self.calls % self.period == 0
        self.calls += 1
        if not root or self.eps == 0:
            return priors, values
        conc = torch.full(priors.shape, self.alpha, dtype=torch.float32, device=priors.device)
        noise = torch.distributions.Dirichlet(conc, validate_args=False).sample() * leaf_mask
        noise = noise / noise.sum(dim=1, keepdim=True).clamp(min=1e-12)
        return (1 - self.eps) * priors.float() + self.eps * noise, values


class FreshRootNoise:
    """``RootNoise`` for ``AsyncSearchSelfPlay``, whose rows reach their roots at different calls: the noise goes to the rows
    of ``fresh()`` (uint8 [N], the player's ``fresh``), in every call; no host synchronisation.  With ``leaves`` = L
    positions per row the batch has N * L rows and a fresh row's root is its slot 0, batch row i * L"""

    def __init__(self, inner, alpha=0.3, eps=0.25, leaves=1):
        self.inner, self.alpha, self.eps, self.fresh, self.leaves = inner, alpha, eps, None, leaves

    def __call__(self, leaf_obs, leaf_mask):
        priors, values = self.inner(leaf_obs, leaf_mask)
        if self.fresh is None or self.eps == 0:
            return priors, values
        conc = torch.full(priors.shape, self.alpha, dtype=torch.float32, device=priors.device)
        noise = torch.distributions.Dirichlet(conc, validate_args=False).sample() * leaf_mask
        noise = noise / noise.sum(dim=1, keepdim=True).clamp(min=1e-12)
        eps = self.eps * self.fresh().to(torch.float32).unsqueeze(1)
        if self.leaves > 1:  # [N] -> [N * L]: slot 0 of every row
            eps = torch.cat([eps, eps.new_zeros(len(eps), self.leaves - 1)], dim=1).reshape(-1, 1)
        return (1 - eps) * priors.float() + eps * noise, values


def greedy(net):
    from selfplay.policy import Policy

    class Greedy(Policy):
        def act(self, obs, deterministic=False):
            with torch.no_grad():
                logits, _ = net.logits(obs["observation"], obs["action_mask"])
            return logits.argmax(dim=1)

    return Greedy()


def train(m=3, n=3, k=3, envs=256, iterations=32, rounds=12, plies=None, updates=40, batch=512, lr=2e-3, seed=0,
          noise=True, reuse=False, leaves=1, solver=False, search="puct", considered=4, fast_iterations=None,
          full_prob=None, fpu=None, forced=None, log=print):
    """self-play and training rounds; returns the network.  ``noise``: True / "wrapper" (``RootNoise``), "builtin" (the
    search's own root noise, same alpha and eps) or False / "off" (none).  ``search``: "puct", or "gumbel" -- a Gumbel
    root over ``considered`` moves (``SearchSelfPlay(gumbel=...)``): the exploration is the Gumbel draw and the targets are
    the improved policy, so ``noise`` is not used, and a small ``iterations`` (16) is what it is meant for.
    ``fast_iterations`` and ``full_prob`` (both, or neither): play through ``AsyncSearchSelfPlay`` with per-ply budgets.
    ``fpu``: None, a number or (fpu, fpu_root) -- first-play urgency (``SearchSelfPlay(fpu=...)``): an untried move is
    valued at its parent's mean value less a reduction, not at 0.  ``forced``: None or k -- forced playouts and policy
    target pruning (``SearchSelfPlay(forced=k)``; 2 is usual), what makes root noise useful as a policy target"""
    entry.build()
    from selfplay.policy import model_evaluator
    from selfplay.search_selfplay import SearchSelfPlay

    torch.manual_seed(seed)
    dev = torch.device("cuda", torch.cuda.current_device())
    C = m * n
    net = PolicyValueNet(C).to(dev)
    opt = torch.optim.Adam(net.parameters(), lr=lr)
    evaluator = model_evaluator(net)
    if search not in ("puct", "gumbel"):
        raise ValueError(f"search must be 'puct' or 'gumbel', got {search!r}")
    noise = "off" if search == "gumbel" else {True: "wrapper", False: "off"}.get(noise, noise)
    if noise not in ("wrapper", "builtin", "off"):
        raise ValueError(f"noise must be 'wrapper', 'builtin' or 'off', got {noise!r}")
    if (fast_iterations is None) != (full_prob is None):
        raise ValueError("fast_iterations and full_prob go together")
    if fast_iterations is not None:
        return _train_async(net, opt, evaluator, m, n, k, envs, iterations, fast_iterations, full_prob, rounds, plies,
                            updates, batch, seed, noise, solver, reuse, leaves,
                            considered if search == "gumbel" else None, fpu, forced, log)
    if noise == "wrapper":
        evaluator = RootNoise(evaluator, iterations // leaves + 1)
    sp = SearchSelfPlay(m, n, k, envs, evaluator=evaluator, iterations=iterations, temp_plies=max(1, C // 3),
                        capacity=2 * C, seed=seed, reuse=reuse, leaves=leaves, solver=solver,
                        root_noise=(0.3, 0.25) if noise == "builtin" else None,
                        gumbel=considered if search == "gumbel" else None, fpu=fpu, forced=forced)
    assert sp.policy.evaluations_per_act == iterations // leaves + 1
    plies = C if plies is None else plies
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    for r in range(rounds):
        net.eval()
        sp.play(plies)
        net.train()
        for _ in range(updates):
            b = sp.buffer.sample(batch, generator=gen)
            logits, v = net.logits(b["observation"], b["action_mask"])
            logp = torch.log_softmax(logits, dim=1)
            loss_pi = -(b["policy"] * logp.masked_fill(~b["action_mask"], 0.0)).sum(dim=1)
            loss = ((loss_pi + (v - b["value"]) ** 2) * b["weight"]).sum() / b["weight"].sum().clamp(min=1.0)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
        if reuse:
            sp.reset_trees()  # the kept visits and values are the old weights': search afresh with the new ones
        stats = sp.pop_game_stats()
        log(f"round {r}: games {stats['games']} black {stats['black_wins']} white {stats['white_wins']} "
            f"draws {stats['draws']} mean length {stats['mean_length']:.2f} loss {loss.item():.4f}")
    net.eval()
    return net


def _train_async(net, opt, evaluator, m, n, k, envs, iterations, fast_iterations, full_prob, rounds, plies, updates, batch,
                 seed, noise, solver, reuse, leaves, gumbel, fpu, forced, log):
    """``train`` through ``AsyncSearchSelfPlay``: a training round follows as many evaluator calls as ``plies`` plies of
    every row cost on average; the loss is ``train``'s (a fast ply's policy target is all zero: only its value counts).
    ``gumbel``: None, or the moves a Gumbel root considers (``train`` has turned the noise off then)"""
    from selfplay.search_selfplay import AsyncSearchSelfPlay

    if leaves != 1 and reuse:
        raise ValueError("per-ply budgets with leaves do not combine with reuse yet")
    dev = next(net.parameters()).device
    C = m * n
    if noise == "wrapper":
        evaluator = FreshRootNoise(evaluator, leaves=leaves)
    sp = AsyncSearchSelfPlay(m, n, k, envs, evaluator=evaluator, iterations=iterations, fast_iterations=fast_iterations,
                             full_prob=full_prob, temp_plies=max(1, C // 3), capacity=2 * C, seed=seed, solver=solver,
                             root_noise=(0.3, 0.25) if noise == "builtin" else None, keep_tree=reuse, leaves=leaves,
                             gumbel=gumbel, fpu=fpu, forced=forced)
    if noise == "wrapper":
        evaluator.fresh = lambda: sp.fresh
    # (evaluator calls per ply: ceil(B / L) + 1 for a budget of B)
    per_ply = full_prob * (-(-iterations // leaves) + 1) + (1 - full_prob) * (-(-fast_iterations // leaves) + 1)
    calls = max(1, round((C if plies is None else plies) * per_ply))
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    for r in range(rounds):
        net.eval()
        sp.advance(calls)
        net.train()
        for _ in range(updates):
            b = sp.buffer.sample(batch, generator=gen)
            logits, v = net.logits(b["observation"], b["action_mask"])
            logp = torch.log_softmax(logits, dim=1)
            loss_pi = -(b["policy"] * logp.masked_fill(~b["action_mask"], 0.0)).sum(dim=1)
            loss = ((loss_pi + (v - b["value"]) ** 2) * b["weight"]).sum() / b["weight"].sum().clamp(min=1.0)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
        if reuse:
            sp.reset_trees()  # the kept visits and values are the old weights': search afresh with the new ones
        stats = sp.pop_game_stats()
        log(f"round {r}: {calls} evaluator calls, plies {int(sp.row_plies.min())}..{int(sp.row_plies.max())} games "
            f"{stats['games']} black {stats['black_wins']} white {stats['white_wins']} draws {stats['draws']} mean length "
            f"{stats['mean_length']:.2f} loss {loss.item():.4f}")
    net.eval()
    return net


def validate(net, m, n, k, episodes=1024):
    from selfplay.policy import RandomPolicy, TacticalPolicy
    from selfplay.validation import validate_gpu

    out = {}
    for name, opp in (("random", RandomPolicy(m * n, seed=1)), ("tactical", TacticalPolicy(k, seed=2))):
        res = validate_gpu(greedy(net), opp, (m, n, k), n_episodes=episodes)
        out[name] = {key.split("/")[-1]: val for key, val in res.items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--board", default="3x3x3", help="MxNxK")
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--iterations", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--updates", type=int, default=40)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--reuse", action="store_true", help="keep the subtree of the move played for the next search")
    ap.add_argument("--noise", choices=("wrapper", "builtin", "off"), default="wrapper",
                    help="Dirichlet root noise: an evaluator wrapper on torch's generator, the search's own (Philox-keyed, "
                         "reproducible), or none")
    ap.add_argument("--leaves", type=int, default=1,
                    help="leaves per row and evaluator call (a divisor of --iterations, at most 16): the network sees "
                         "iterations / leaves + 1 batches of envs * leaves positions per move")
    ap.add_argument("--solver", action="store_true",
                    help="prove wins, draws and losses in the search tree; proven losses leave the policy targets")
    ap.add_argument("--search", choices=("puct", "gumbel"), default="puct",
                    help="gumbel: a Gumbel root with Sequential Halving and improved-policy targets (no root noise; try "
                         "--iterations 16)")
    ap.add_argument("--considered", type=int, default=4, help="--search gumbel: the root moves Sequential Halving considers")
    ap.add_argument("--fast-iterations", type=int, default=None,
                    help="with --full-prob: the budget of the plies that are not searched in full (value targets only)")
    ap.add_argument("--full-prob", type=float, default=None,
                    help="with --fast-iterations: the probability that a ply is searched with --iterations and becomes a "
                         "policy target; rows then play on as soon as their own search is done")
    ap.add_argument("--fpu", type=float, default=None,
                    help="first-play urgency: value an untried move at its parent's mean value less FPU * sqrt(visited "
                         "prior mass) instead of 0 (0.2 is usual; not with --search gumbel, nor with --leaves above 1 "
                         "under per-ply budgets)")
    ap.add_argument("--fpu-root", type=float, default=None, help="with --fpu: the reduction at the root (default: --fpu)")
    ap.add_argument("--forced", type=float, default=None, metavar="K",
                    help="forced playouts and policy target pruning: a visited root move is searched again while its "
                         "visits squared lie below K * prior * root visits, and the visits PUCT alone would not have spent "
                         "leave the policy target (2 is usual; meant for --noise builtin; not with --search gumbel, nor "
                         "with --reuse or --leaves above 1 under per-ply budgets)")
    a = ap.parse_args()
    if a.fpu_root is not None and a.fpu is None:
        ap.error("--fpu-root needs --fpu")
    fpu = None if a.fpu is None else (a.fpu, a.fpu if a.fpu_root is None else a.fpu_root)
    m, n, k = (int(x) for x in a.board.lower().split("x"))
    net = train(m, n, k, envs=a.envs, iterations=a.iterations, rounds=a.rounds, updates=a.updates, seed=a.seed,
                noise=a.noise, reuse=a.reuse, leaves=a.leaves, solver=a.solver, search=a.search, considered=a.considered,
                fast_iterations=a.fast_iterations, full_prob=a.full_prob, fpu=fpu, forced=a.forced)
    for name, res in validate(net, m, n, k).items():
        print(f"vs {name}: win {res['win_rate']:.3f} loss {res['loss_rate']:.3f} draw {res['draw_rate']:.3f} "
              f"score {res['score_rate']:.3f}")


if __name__ == "__main__":
    main()
