#!/usr/bin/env python3
"""The MLP actor on the bf16 matrix unit against the float32 MFMA actor (GPU box).

One session, one process, per env (ChemicalReactor, PowerGrid) at --batch lanes, --steps env.step per launch: the two arms
  (f32)   nig_rollout_mlp        v_mfma_f32_32x32x2_f32, the parity path
  (bf16)  nig_rollout_mlp_bf16   v_mfma_f32_32x32x16_bf16, "nig-mlp-bf16-v1"
ALTERNATE, --repeats rounds of --launches launches each after --warmup, HIP events around every launch, every series bracketed
by bench.py's shader-clock stamps (the clock the chip held is recorded per arm and round).  Both arms run the same handle, the
same weights (the bf16 arm rounds them) and auto-reset, from whatever states the previous series left: the time per step does
not depend on the state.  Per series: median / min / max microseconds per step over the launches.  The table gives each arm's
spread over its rounds and the ratio f32 / bf16, from the rounds' medians.

usage: python profiles/bench_bf16.py [--out-dir DIR]   ->  DIR/ab.jsonl (one line per series), DIR/ab.txt (the table)"""
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
ap.add_argument("--out-dir", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "bf16"))
args = ap.parse_args()
B, T, N = args.batch, args.steps, args.launches
os.makedirs(args.out_dir, exist_ok=True)
rows = []


def actor(S, A, seed):
    rng = np.random.default_rng(seed)
    return [(rng.normal(0, 0.02 / np.sqrt(S), (S, 256)).astype(np.float32), np.zeros(256, np.float32)),
            (rng.normal(0, 1 / 16, (256, 256)).astype(np.float32), np.zeros(256, np.float32)),
            (rng.normal(0, 1 / 16, (256, A)).astype(np.float32), np.zeros(A, np.float32))]


def timed(env, name, arm, rnd, launch, flops):
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
    row = {"env": name, "arm": arm, "round": rnd, "batch": B, "steps_per_launch": T, "launches": N,
           "us_per_step_median": float(np.median(us)), "us_per_step_min": float(us.min()), "us_per_step_max": float(us.max()),
           "useful_TFLOPs": float(flops * B / np.median(us) / 1e6), "clock": probe.read()}
    rows.append(row)
    print(json.dumps(row), flush=True)


for name in args.envs.split(","):
    env = ni.make_batched(name, B, autoreset=True, tally=True)
    S, A = env.state_dim, env.action_dim
    flops = 2.0 * (S * 256 + 256 * 256 + 256 * A)
    ws = actor(S, A, 10)
    env.set_mlp_policy(ws)
    env.set_mlp_policy_bf16(ws)
    env.reset()
    for rnd in range(args.repeats):
        timed(env, name, "f32", rnd, lambda: env.rollout_mlp(T), flops)
        timed(env, name, "bf16", rnd, lambda: env.rollout_mlp_bf16(T), flops)
    env.close()

with open(os.path.join(args.out_dir, "ab.jsonl"), "w") as f:
    for r in rows:
        f.write(json.dumps(r) + "\n")
lines = [f"batch {B}, {T} steps per launch, {args.repeats} alternating rounds of {N} timed launches after {args.warmup}; microseconds per step",
         f"{torch.cuda.get_device_name(0)}; {ni._lib.lib().nig_version().decode()}", ""]
for name in args.envs.split(","):
    med = {}
    for arm in ("f32", "bf16"):
        mine = [r for r in rows if r["env"] == name and r["arm"] == arm]
        med[arm] = [r["us_per_step_median"] for r in mine]
        for r in mine:
            clk = r["clock"].get("shader_clock_mhz", float("nan"))
            lines.append(f"{name:20s} {arm:5s} round {r['round']}  {r['us_per_step_median']:8.2f} us ({r['us_per_step_min']:.2f} .. {r['us_per_step_max']:.2f})  "
                         f"{r['useful_TFLOPs']:7.1f} useful TFLOP/s  {clk:.0f} MHz")
    spread = {arm: 100 * (max(v) - min(v)) / min(v) for arm, v in med.items()}
    ratio = [a / b for a, b in zip(med["f32"], med["bf16"])]
    lines.append(f"{name}: f32 / bf16 per round {', '.join(f'{x:.2f}' for x in ratio)}; spread of the rounds: f32 {spread['f32']:.2f} %, bf16 {spread['bf16']:.2f} %; "
                 f"bf16 below f32 in every round: {all(b < a for a, b in zip(med['f32'], med['bf16']))}")
    lines.append("")
open(os.path.join(args.out_dir, "ab.txt"), "w").write("\n".join(lines))
print("\n".join(lines))
