"""Developer tool: what search self-play (SearchSelfPlay.play / mnk_search_selfplay_step, SearchReplayBuffer.sample /
mnk_search_gather) costs.

``play`` on 9x9x5 x 1 024 boards with I = 64 and I = 256, timed with device events around ``plies`` back-to-back eager
plies after a warm-up, with the two evaluators of tools/exp_puct.py (``conv``: 4 conv layers of 64 channels and two
heads; ``trivial``: uniform priors, value 0).  The gather: one ``mnk_search_gather`` launch of B = 65 536 samples with
symmetries from a ring that self-play has filled, f32 observations, timed over ``reps`` launches; its bytes are what the
kernel must move (per sample: the 16*W B of planes, the 2C B of visits and the z byte read; 8C + C + 4C + 8 B written).

``--profile``: a short untimed pass of each case for ``rocprofv3 --kernel-trace --stats`` (run it under the profiler, in
a run of its own); the share of the two new kernels in a ply is read from the kernel stats.

usage: python tools/exp_search_selfplay.py [--plies 8] [--out profiles/exp_search_selfplay.json] [--profile]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rl-selfplay-mnk_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
M, N_, K, ENVS = 9, 9, 5, 1024
HBM_PEAK_GBPS = 8000.0  # MI355X HBM3E


def selfplay(kind, I):
    from exp_puct import evaluator

    from selfplay.search_selfplay import SearchSelfPlay

    return SearchSelfPlay(M, N_, K, ENVS, evaluator=evaluator(kind, M * N_), iterations=I, temp_plies=8, seed=1)


def time_play(kind, I, plies):
    import torch

    sp = selfplay(kind, I)
    sp.play(2)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    sp.play(plies)
    e1.record()
    e1.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / plies
    return {"board": f"{M}x{N_}x{K}", "envs": ENVS, "iterations": I, "evaluator": kind, "us_per_ply": round(us, 1),
            "us_per_iteration": round(us / (I + 1), 2)}, sp


def time_gather(sp, B, reps):
    import torch

    buf = sp.buffer
    dev = buf.device
    C, W = buf.C, buf.W
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    filled = min(buf.plies_host, buf.capacity) * buf.num_envs
    idx = torch.randint(0, filled, (B,), device=dev, generator=g)
    sym = torch.randint(0, buf.symmetries, (B,), dtype=torch.int8, device=dev, generator=g)
    out = {"observation": torch.empty((B, 2, M, N_), device=dev), "action_mask": torch.empty((B, C), dtype=torch.bool, device=dev),
           "policy": torch.empty((B, C), device=dev), "value": torch.empty(B, device=dev), "weight": torch.empty(B, device=dev)}
    for _ in range(3):
        buf.gather(idx, sym, out)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        buf.gather(idx, sym, out)
    e1.record()
    e1.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / reps
    per = 16 * W + 2 * C + 1 + 8 + (8 * C + C + 4 * C + 8) + 1
    gbps = per * B / us / 1e3
    buf.check_errors()
    return {"B": B, "us": round(us, 1), "bytes_per_sample": per, "GBps": round(gbps, 1),
            "share_of_hbm_peak": round(gbps / HBM_PEAK_GBPS, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plies", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exp_search_selfplay.json"))
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    import __graft_entry__ as entry

    entry.build_hip()
    import torch

    torch.backends.cudnn.benchmark = False
    if args.profile:  # a few eager plies of each case and one gather; the profiler does the timing
        for kind in ("conv", "trivial"):
            for I in (64, 256):
                sp = selfplay(kind, I)
                sp.play(3)
        sp.buffer.sample(65536)
        torch.cuda.synchronize()
        print("profile pass done")
        return
    rows, sp = [], None
    for kind in ("conv", "trivial"):
        for I in (64, 256):
            row, sp = time_play(kind, I, args.plies)
            print(json.dumps(row), flush=True)
            rows.append(row)
    gat = time_gather(sp, 65536, args.reps)
    print(json.dumps(gat), flush=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "play": rows, "gather": gat}, f, indent=1)


if __name__ == "__main__":
    main()
