#!/usr/bin/env python3
"""The fused constraint projection against the shield it extends (GPU box): what does "nig-project-v1" cost per step, and per
gradient step?

One session, one box, per env (ChemicalReactor, PowerGrid) at --batch lanes, --steps env.step per launch, HIP events around each
of --launches launches after --warmup, every series bracketed by bench.py's shader-clock stamps.  The series alternate through
--repeats rounds, so a drift of the box shows as the spread of a series' own repeats:
  mlp        nig_rollout_mlp                    the actor alone (shield - mlp = one critic pass, the yardstick of a pass)
  shield     nig_rollout_mlp_safe               A: the parent's entry point, same process, same handle
  keep       nig_rollout_mlp_projected          (a) a threshold no p reaches: nothing is projected, one forward pass and the vote
  walk_K     nig_rollout_mlp_projected          (b) threshold 0 and a tolerance no logit satisfies, max_iters = K (1, 3, 10): every
                                                lane of every block walks K gradient steps, K backward + forward pairs
What the structure predicts: keep within a few percent of the shield's step; a backward + forward pair about two critic passes.
No outputs are written by any series (the rollouts' own default), so the figures are the kernels' compute cost.

usage: python profiles/bench_project.py [--out-dir DIR]   ->  DIR/ab.jsonl (one line per series), DIR/ab.txt (the table)"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import neorl_industrial_gym_amd as ni
from bench import ClockProbe

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=65536)
ap.add_argument("--steps", type=int, default=250)
ap.add_argument("--launches", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--envs", default="ChemicalReactor-v0,PowerGrid-v0")
ap.add_argument("--iters", default="1,3,10")
ap.add_argument("--outputs", type=int, default=3)
ap.add_argument("--out-dir", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "project"))
args = ap.parse_args()
B, T, N = args.batch, args.steps, args.launches
KS = [int(x) for x in args.iters.split(",")]
os.makedirs(args.out_dir, exist_ok=True)
rows = []


def net(D, O, seed, head):
    rng = np.random.default_rng(seed)
    return [(rng.normal(0, 0.02 / np.sqrt(D), (D, 256)).astype(np.float32), np.zeros(256, np.float32)),
            (rng.normal(0, 1 / 16, (256, 256)).astype(np.float32), np.zeros(256, np.float32)),
            (rng.normal(0, head, (256, O)).astype(np.float32), np.zeros(O, np.float32))]


def timed(env, name, series, launch, repeat):
    probe = ClockProbe(ni, torch, env.device)
    for _ in range(args.warmup):
        launch()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(N)]
    probe.stamp(0)
    for a, b in ev:
        a.record(); launch(); b.record()
    probe.stamp(1)
    torch.cuda.synchronize()
    us = np.array([a.elapsed_time(b) for a, b in ev]) * 1e3 / T
    row = {"env": name, "series": series, "repeat": repeat, "batch": B, "steps_per_launch": T, "launches": N,
           "us_per_step_median": float(np.median(us)), "us_per_step_min": float(us.min()), "us_per_step_max": float(us.max()),
           "clock": probe.read()}
    rows.append(row)
    print(json.dumps(row), flush=True)


for name in args.envs.split(","):
    env = ni.make_batched(name, B, autoreset=True, tally=True)
    S, A = env.state_dim, env.action_dim
    env.set_mlp_policy(net(S, A, 10, 1 / 16))
    env.set_mlp_safety(net(S + A, 1, 20, 1 / 2), 2.0)
    predictor = net(S + A, args.outputs, 30, 0.04)
    env.reset()

    def keep():
        env.set_mlp_constraint(predictor, 2.0, 0.01)                 # no sigmoid reaches 2
        return lambda: env.rollout_mlp_projected(T, 10, 0.1)

    def walk(K):
        env.set_mlp_constraint(predictor, 0.0, -1.0e30)              # no p is below 0, no finite logit below -1e30
        return lambda: env.rollout_mlp_projected(T, K, 0.01)
    for rep in range(args.repeats):
        timed(env, name, "mlp", lambda: env.rollout_mlp(T), rep)
        timed(env, name, "shield", lambda: env.rollout_mlp_safe(T), rep)
        timed(env, name, "keep", keep(), rep)
        for K in KS:
            timed(env, name, f"walk_{K}", walk(K), rep)
    env.close()

with open(os.path.join(args.out_dir, "ab.jsonl"), "w") as f:
    for r in rows:
        f.write(json.dumps(r) + "\n")
lines = [f"batch {B}, auto-reset, {T} steps per launch, {N} timed launches after {args.warmup}, {args.repeats} alternating repeats, a head of {args.outputs} rows; "
         "microseconds per step, median of the launches, per repeat", f"{torch.cuda.get_device_name(0)}; {ni._lib.lib().nig_version().decode()}", ""]
for name in args.envs.split(","):
    mine = [r for r in rows if r["env"] == name]
    med = {}
    for r in mine:
        med.setdefault(r["series"], []).append(r["us_per_step_median"])
    mlp, shield = np.median(med["mlp"]), np.median(med["shield"])
    yard = shield - mlp
    lines.append(f"{name}: one critic pass = shield - mlp = {yard:.2f} us (medians of the repeats)")
    prev = None
    for series in ["mlp", "shield", "keep"] + [f"walk_{K}" for K in KS]:
        x = med[series]
        clk = [r["clock"].get("shader_clock_mhz", float("nan")) for r in mine if r["series"] == series]
        txt = f"  {series:8s} {', '.join(f'{v:8.2f}' for v in x)} us   spread {100 * (max(x) - min(x)) / min(x):5.2f} %   {np.median(clk):.0f} MHz"
        if series == "keep":
            txt += f"   / shield: {np.median(x) / shield:.3f}"
            prev = (0, np.median(x))
        if series.startswith("walk_"):
            K = int(series[5:])
            per = (np.median(x) - prev[1]) / (K - prev[0])
            txt += f"   / shield: {np.median(x) / shield:.3f}   per further backward + forward pair {per:.2f} us = {per / yard:.3f} x one critic pass"
            prev = (K, np.median(x))
        lines.append(txt)
    lines.append("")
open(os.path.join(args.out_dir, "ab.txt"), "w").write("\n".join(lines))
print("\n".join(lines))
