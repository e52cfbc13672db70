"""Developer tool: what the PUCT search player (PUCTSearchPolicy / mnk_puct_step) costs per act().

``PUCTSearchPolicy.act`` on N rows of random mid-game positions (up to half the board filled by uniformly random play,
tests/tactical_rule.random_positions), timed with device events around ``reps`` back-to-back calls after a warm-up, in
two forms: eager (I + 2 env-side launches and I + 1 evaluator calls issued from Python) and captured (one act() in a
``torch.cuda.graph``, replayed).  Two evaluators: ``conv``, a small AlphaZero-style conv net (4 conv layers of 64
channels, a policy and a value head; f32), and ``trivial``, uniform priors and value 0 in two torch ops -- the env-side
cost with next to nothing on the other side.

``--profile``: one captured-free pass of each case for ``rocprofv3 --kernel-trace --stats`` (run it under the profiler,
in a run of its own); the split between k_puct_step and the evaluator's kernels is read from the kernel stats.

usage: python tools/exp_puct.py [--reps 5] [--out profiles/exp_puct.json] [--profile]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rl-selfplay-mnk_amd"), os.path.join(ROOT, "tests")]
# (m, n, k, rows, I)
CASES = ((9, 9, 5, 1024, 256), (19, 19, 5, 256, 256))


def conv_net(cells, width=64):
    import torch
    import torch.nn as nn

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            layers, cin = [], 2
            for _ in range(4):
                layers += [nn.Conv2d(cin, width, 3, padding=1), nn.ReLU()]
                cin = width
            self.body = nn.Sequential(*layers)
            self.pi = nn.Conv2d(width, 1, 1)
            self.v = nn.Linear(width, 1)

        def forward(self, obs, mask):
            h = self.body(obs)
            logits = torch.where(mask, self.pi(h).flatten(1), torch.full((1,), -torch.inf, device=obs.device))
            return torch.softmax(logits, dim=1), torch.tanh(self.v(h.mean(dim=(2, 3)))).reshape(-1)

    return Net().to("cuda:0").eval()


def evaluator(kind, cells):
    import torch

    if kind == "trivial":
        return lambda obs, mask: (mask.float(), torch.zeros(len(mask), device=mask.device))
    net = conv_net(cells)

    def evaluate(obs, mask):
        with torch.no_grad():
            return net(obs, mask)

    return evaluate


def timing(m, n, k, rows, I, kind, reps):
    import numpy as np
    import torch

    from selfplay.policy import PUCTSearchPolicy
    from tactical_rule import random_positions

    obs_np = random_positions(m, n, k, rows, np.random.default_rng(m * n + I), max_fill=0.5)
    obs = {"observation": torch.from_numpy(obs_np).to("cuda:0")}
    pol = PUCTSearchPolicy(k, evaluator=evaluator(kind, m * n), iterations=I, seed=1)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            pol.act(obs)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        pol.act(obs)
    e1.record()
    e1.synchronize()
    eager = e0.elapsed_time(e1) * 1e3 / reps
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pol.act(obs)
    graph.replay()
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        graph.replay()
    e1.record()
    e1.synchronize()
    captured = e0.elapsed_time(e1) * 1e3 / reps
    return {"board": f"{m}x{n}x{k}", "rows": rows, "iterations": I, "evaluator": kind, "us_per_act_eager": round(eager, 1),
            "us_per_act_captured": round(captured, 1), "us_per_iteration_captured": round(captured / (I + 1), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exp_puct.json"))
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    import __graft_entry__ as entry

    entry.build_hip()
    import torch

    torch.backends.cudnn.benchmark = False
    if args.profile:  # one eager act of each case; the profiler does the timing
        import numpy as np

        from selfplay.policy import PUCTSearchPolicy
        from tactical_rule import random_positions

        for m, n, k, rows, I in CASES:
            obs_np = random_positions(m, n, k, rows, np.random.default_rng(1), max_fill=0.5)
            obs = {"observation": torch.from_numpy(obs_np).to("cuda:0")}
            PUCTSearchPolicy(k, evaluator=evaluator("conv", m * n), iterations=I, seed=1).act(obs)
        torch.cuda.synchronize()
        print("profile pass done")
        return
    rows = []
    for m, n, k, r, I in CASES:
        for kind in ("conv", "trivial"):
            row = timing(m, n, k, r, I, kind, args.reps)
            print(json.dumps(row), flush=True)
            rows.append(row)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
