#!/usr/bin/env python3
"""The disturbed closed-loop rollouts against their undisturbed twins (GPU box): what does "nig-disturb-v1" cost per step?

One session, one box, per env (ChemicalReactor, PowerGrid) at --batch lanes, --steps env.step per launch, HIP events around each
of --launches launches after --warmup, every series bracketed by bench.py's shader-clock stamps.  The series alternate A B A B
through --repeats rounds, so a drift of the box shows as the spread of a series' own repeats:
  mlp              nig_rollout_mlp                       (A: the parent's entry point, same process)
  mlp_disturbed    nig_rollout_mlp_disturbed             observation + action noise, hold = step / episode
  policy           nig_rollout_policy, "MPC" proportional law (the batch's own kernel form: three-wave / paired at this size)
  policy_disturbed nig_rollout_policy_disturbed          (always the one-wave form)
  policy_onewave   nig_rollout_policy with nig_tune(split_blocks = 0): the undisturbed ONE-WAVE kernel, the disturbed kernel's parent
No outputs are written by any series (the rollouts' own default), so the figures are the kernels' compute cost.

usage: python profiles/bench_disturbed.py [--out-dir DIR]   ->  DIR/ab.jsonl (one line per series), DIR/ab.txt (the table)"""
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
ap.add_argument("--out-dir", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "disturb"))
args = ap.parse_args()
B, T, N = args.batch, args.steps, args.launches
os.makedirs(args.out_dir, exist_ok=True)
rows = []


def actor(S, A, seed):
    rng = np.random.default_rng(seed)
    return [(rng.normal(0, 0.02 / np.sqrt(S), (S, 256)).astype(np.float32), np.zeros(256, np.float32)),
            (rng.normal(0, 1 / 16, (256, 256)).astype(np.float32), np.zeros(256, np.float32)),
            (rng.normal(0, 1 / 16, (256, A)).astype(np.float32), np.zeros(A, np.float32))]


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
    env.set_mlp_policy(actor(S, A, 10))
    env.set_policy(ni.mpc_agent(S, A))
    env.reset()
    dist = {h: ni.Disturbance(obs_noise=0.1, action_noise=0.1, hold=h) for h in ("step", "episode")}

    def disturbed(fn, hold):
        def go():
            fn(T)
        env.set_disturbance(dist[hold])
        return go

    def onewave():
        ni.tune(split_blocks=0)
        try:
            env.rollout_policy(T)
        finally:
            ni.tune(split_blocks=-1)
    for rep in range(args.repeats):
        timed(env, name, "mlp", lambda: env.rollout_mlp(T), rep)
        for h in ("step", "episode"):
            timed(env, name, f"mlp_disturbed_{h}", disturbed(env.rollout_mlp_disturbed, h), rep)
        timed(env, name, "policy", lambda: env.rollout_policy(T), rep)
        timed(env, name, "policy_onewave", onewave, rep)
        for h in ("step", "episode"):
            timed(env, name, f"policy_disturbed_{h}", disturbed(env.rollout_policy_disturbed, h), rep)
    env.close()

with open(os.path.join(args.out_dir, "ab.jsonl"), "w") as f:
    for r in rows:
        f.write(json.dumps(r) + "\n")
lines = [f"batch {B}, {T} steps per launch, {N} timed launches after {args.warmup}, {args.repeats} alternating repeats; microseconds per step, "
         "median of the launches, per repeat", f"{torch.cuda.get_device_name(0)}; {ni._lib.lib().nig_version().decode()}", ""]
for name in args.envs.split(","):
    mine = [r for r in rows if r["env"] == name]
    med = {}
    for r in mine:
        med.setdefault(r["series"], []).append(r["us_per_step_median"])
    lines.append(name)
    for series, base in (("mlp", None), ("mlp_disturbed_step", "mlp"), ("mlp_disturbed_episode", "mlp"), ("policy", None),
                         ("policy_onewave", "policy"), ("policy_disturbed_step", "policy_onewave"), ("policy_disturbed_episode", "policy_onewave")):
        x = med[series]
        clk = [r["clock"].get("shader_clock_mhz", float("nan")) for r in mine if r["series"] == series]
        txt = f"  {series:26s} {', '.join(f'{v:8.2f}' for v in x)} us   spread {100 * (max(x) - min(x)) / min(x):5.2f} %   {np.median(clk):.0f} MHz"
        if base:
            txt += f"   / {base}: {np.median(x) / np.median(med[base]):.3f} (medians of the repeats)"
        lines.append(txt)
    lines.append("")
open(os.path.join(args.out_dir, "ab.txt"), "w").write("\n".join(lines))
print("\n".join(lines))
