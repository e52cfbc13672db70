"""Developer tool: what the tactical opponent costs in the one-launch self-play step, against the random opponent.

A captured rollout (selfplay.graphed.GraphedRollout, uniform agent, T agent-steps) with RandomPolicy as the opponent (A:
k_selfplay_step_random) and with TacticalPolicy (B: k_selfplay_step_tactical) -- same wrapper seed, same board, same
batch -- timed with device events around graph replays, A and B alternating in one process (the order swapped every
repetition), so clocks and neighbours weigh on both alike.  A captured rollout has no host launch cost in it: what is
timed is the step kernel (the uniform agent's draw folded in) plus one copy of the carried-over observation per rollout,
the same in A and B.  The per-kernel split comes from a separate `rocprofv3 --kernel-trace --stats` run of this tool.

Boards: 9x9x5 at 65 536 envs, 19x19x5 at 32 768, 12x12x5 at 65 536 (no built-in variant: its run-time compiled kernels,
MNK_JIT_API=1).  Each board runs in a child process of its own under a time limit; the parent stops at the first failure.

usage: python tools/exp_tactical.py [--reps 15] [--steps 16] [--out profiles/exp_tactical.json]
       (child: python tools/exp_tactical.py child m n k envs reps steps)"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rl-selfplay-mnk_amd")]
BOARDS = ((9, 9, 5, 65536), (19, 19, 5, 32768), (12, 12, 5, 65536))
CHILD_TIMEOUT_S = 300


def child(m, n, k, nenv, reps, steps):
    os.environ["MNK_JIT_API"] = "1"  # 12x12x5: the board's own kernels from the first launch (read once, before loading)
    import statistics

    import torch

    from alg.rollout_buffer import RolloutBuffer
    from env.torch_vector_mnk_env import TorchVectorMnkEnv
    from selfplay.graphed import GraphedRollout
    from selfplay.policy import RandomPolicy, TacticalPolicy
    from selfplay.torch_self_play_wrapper import TorchSelfPlayWrapper

    dev = "cuda:0"
    rolls = {}
    for name, opp in (("random", RandomPolicy(m * n, seed=3)), ("tactical", TacticalPolicy(k, seed=3))):
        w = TorchSelfPlayWrapper(TorchVectorMnkEnv(m, n, k, nenv, device=dev), seed=5)
        w.set_opponent(opp)
        buf = RolloutBuffer(steps, nenv, (2, m, n), m * n, device=dev)
        rolls[name] = GraphedRollout(w, buf, None, seed=11)
    for r in rolls.values():  # warm
        for _ in range(3):
            r.run()
    torch.cuda.synchronize()
    us = {name: [] for name in rolls}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for rep in range(reps):
        order = ("random", "tactical") if rep % 2 == 0 else ("tactical", "random")
        for name in order:
            e0.record()
            rolls[name].run()
            e1.record()
            e1.synchronize()
            us[name].append(e0.elapsed_time(e1) * 1e3 / steps)
    out = {"board": f"{m}x{n}x{k}", "envs": nenv, "steps_per_rollout": steps, "reps": reps}
    for name, v in us.items():
        out[name] = {"median_us_per_step": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
    out["ratio_median"] = round(out["tactical"]["median_us_per_step"] / out["random"]["median_us_per_step"], 3)
    out["extra_us_median"] = round(out["tactical"]["median_us_per_step"] - out["random"]["median_us_per_step"], 3)
    print(json.dumps(out), flush=True)


def main():
    args = sys.argv[1:]
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 15
    steps = int(args[args.index("--steps") + 1]) if "--steps" in args else 16
    out = args[args.index("--out") + 1] if "--out" in args else None
    lines = []
    for m, n, k, nenv in BOARDS:
        cmd = [sys.executable, os.path.abspath(__file__), "child", str(m), str(n), str(k), str(nenv), str(reps), str(steps)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            print(f"{m}x{n}x{k}: no result within {CHILD_TIMEOUT_S} s -- stopping", file=sys.stderr)
            return 124
        if p.returncode != 0:
            print(f"{m}x{n}x{k}: child exited with {p.returncode} -- stopping\n{p.stderr[-3000:]}", file=sys.stderr)
            return p.returncode if p.returncode > 0 else 1
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
        print(line, flush=True)
        lines.append(json.loads(line))
    if out:
        with open(out, "w") as f:
            json.dump(lines, f, indent=1)
    return 0


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "child":
        child(*(int(v) for v in sys.argv[2:8]))
    else:
        sys.exit(main())
