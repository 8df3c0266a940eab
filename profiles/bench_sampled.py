#!/usr/bin/env python3
"""Per-launch time of the fused rollout at the BASELINE shapes, ring-fed (nig_rollout) or sampled (nig_rollout_sampled):
250-step launches with full outputs (reward + flag rows + row-major trajectory), every launch timed by its own pair of events.

    python profiles/bench_sampled.py --mode ring|sampled [--tree DIR] [--tag NAME] [--launches 10] [--warmup 3] [--shapes ...]

--tree: the checkout whose package and library are used (default: this one).  A checkout of the parent commit has no
rollout_sampled: only --mode ring works there -- that is the baseline of profiles/sampled_ab.sh.
Prints one JSON line per shape: {"tag", "mode", "shape", "kernel_us": [...], "median_us", "min_us", "max_us"}.
"""
import argparse
import json
import os
import statistics
import sys

SHAPES = {   # name: (env id, lanes, action ring layout)
    "cr65536": ("ChemicalReactor-v0", 65536, "rows"),
    "pg262144": ("PowerGrid-v0", 262144, "rows"),
    "pg262144_rowmajor": ("PowerGrid-v0", 262144, "aos"),
    "ra262144": ("RobotAssembly-v0", 262144, "rows"),
    "ra65536": ("RobotAssembly-v0", 65536, "rows"),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["ring", "sampled"], required=True)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--tag", default="this")
    ap.add_argument("--steps", type=int, default=250)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    a = ap.parse_args()
    sys.path.insert(0, a.tree)
    os.environ.setdefault("NIG_NO_AUTOBUILD", "1")
    import torch
    import neorl_industrial_gym_amd as ni
    dev = torch.device("cuda:0")
    for name in a.shapes:
        env_id, B, layout = SHAPES[name]
        if a.mode == "sampled" and layout == "aos":
            continue                               # (no ring, no ring layout)
        env = ni.make_batched(env_id, B, device=dev, autoreset=True)
        P, S, A, ld = a.steps, env.state_dim, env.action_dim, env.ld
        rew = torch.empty(P, ld, dtype=torch.float32, device=dev)
        fl = torch.empty(P, ld, dtype=torch.int32, device=dev)
        traj = torch.empty(P, B, S, dtype=torch.float32, device=dev)
        ring = None
        if a.mode == "ring":
            rows = torch.empty(P, A, ld, dtype=torch.float32, device=dev)
            for s in range(P):
                env.fill_actions(1 + s, rows[s])
            ring = rows if layout == "rows" else rows[:, :, :B].permute(0, 2, 1).contiguous()
            del rows
        env.reset()
        launch = (lambda: env.rollout(P, ring, rew, fl, traj)) if a.mode == "ring" else (lambda: env.rollout_sampled(P, rew, fl, traj))
        for _ in range(a.warmup):
            launch()
        torch.cuda.synchronize()
        us = []
        for _ in range(a.launches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); launch(); e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3)
        print(json.dumps({"tag": a.tag, "mode": a.mode, "shape": name, "lanes": B, "steps": P, "kernel_us": [round(x, 1) for x in us],
                          "median_us": round(statistics.median(us), 1), "min_us": round(min(us), 1), "max_us": round(max(us), 1),
                          "version": ni._lib.lib().nig_version().decode()}), flush=True)
        env.close()
        del rew, fl, traj, ring
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
