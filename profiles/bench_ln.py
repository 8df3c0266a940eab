#!/usr/bin/env python3
"""The LayerNorm MFMA actor ("nig-mlp-ln-v1") against the plain 256 x 256 kernel and against the host route it replaces (GPU box).

One session, one process, per env (ChemicalReactor, PowerGrid) at --batch lanes: three arms
  (a)  nig_rollout_mlp with a LayerNorm actor installed by nig_set_mlp_policy_ln (the new kernel), --steps steps per launch
  (b)  nig_rollout_mlp with the plain (256, 256) actor of nig_set_mlp_policy: the same 32 x 32 x 2 MFMA count, two blocks per CU
  (c)  the route the parent commit takes for such an agent: LayerNormMLPPolicy.predict_device (torch GEMMs and reductions) + one
       env.step launch per step, as _evaluate_batched's host loop does it; --host-steps steps per timed series
ALTERNATE, --repeats rounds of --launches timed series each after --warmup, HIP events around every series, every arm bracketed by
bench.py's shader-clock stamps (profiles/bench_shapes.py's procedure).  All arms run the same handle with auto-reset, from whatever
states the previous series left.  The table gives each arm's median per round, its spread over the rounds, (a) / (b), (c) / (a) and
the routing condition: (a) below (c) by more than the two spreads together.

Run it under a time limit of its own:
    timeout -k 10 300 python profiles/bench_ln.py --out-dir DIR
usage: python profiles/bench_ln.py [--out-dir DIR]   ->  DIR/ab.jsonl, DIR/ab.txt"""
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
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--host-steps", type=int, default=20)
ap.add_argument("--launches", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--envs", default="ChemicalReactor-v0,PowerGrid-v0")
ap.add_argument("--out-dir", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "ln"))
args = ap.parse_args()
B, T, N = args.batch, args.steps, args.launches
os.makedirs(args.out_dir, exist_ok=True)
rows = []


def actor(S, A, seed):
    rng = np.random.default_rng(seed)
    f = np.float32
    ws = [(rng.normal(0, 0.02 / np.sqrt(S), (S, 256)).astype(f), rng.normal(0, 0.05, 256).astype(f)),
          (rng.normal(0, 1.0 / 16, (256, 256)).astype(f), rng.normal(0, 0.05, 256).astype(f)),
          (rng.normal(0, 1.0 / 16, (256, A)).astype(f), np.zeros(A, f))]
    norms = [((1.0 + 0.3 * rng.normal(0, 1, 256)).astype(f), (0.2 * rng.normal(0, 1, 256)).astype(f)) for _ in range(2)]
    return ws, norms


def timed(env, name, arm, rnd, series, steps):
    probe = ClockProbe(ni, torch, env.device)
    for _ in range(args.warmup):
        series()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(N)]
    probe.stamp(0)
    for a, b in ev:
        a.record(); series(); b.record()
    probe.stamp(1)
    torch.cuda.synchronize()
    us = np.array([a.elapsed_time(b) for a, b in ev]) * 1e3 / steps
    row = {"env": name, "arm": arm, "round": rnd, "batch": B, "steps_per_series": steps, "series": N,
           "us_per_step_median": float(np.median(us)), "us_per_step_min": float(us.min()), "us_per_step_max": float(us.max()), "clock": probe.read()}
    rows.append(row)
    print(json.dumps(row), flush=True)


for name in args.envs.split(","):
    env = ni.make_batched(name, B, autoreset=True, tally=True)
    S, A = env.state_dim, env.action_dim
    ws, norms = actor(S, A, 11)
    pol = ni.LayerNormMLPPolicy(ws, norms, device=env.device)
    env.reset()

    def host_loop():
        for _ in range(args.host_steps):
            env.step(pol.predict_device(env.obs), layout="aos")
    for rnd in range(args.repeats):
        env.set_mlp_policy_ln(pol)
        timed(env, name, "a", rnd, lambda: env.rollout_mlp(T), T)
        env.set_mlp_policy(ws)
        timed(env, name, "b", rnd, lambda: env.rollout_mlp(T), T)
        timed(env, name, "c", rnd, host_loop, args.host_steps)
    env.close()

with open(os.path.join(args.out_dir, "ab.jsonl"), "w") as f:
    for r in rows:
        f.write(json.dumps(r) + "\n")
lines = [f"batch {B}; (a), (b): {T} steps per launch, (c): {args.host_steps} host steps per series; {args.repeats} alternating rounds of {N} timed series "
         f"after {args.warmup}; microseconds per step, median of a round (min .. max over the rounds' medians)",
         f"{torch.cuda.get_device_name(0)}; {ni._lib.lib().nig_version().decode()}",
         "(a) nig_rollout_mlp, LayerNorm actor   (b) nig_rollout_mlp, plain 256 x 256 actor   (c) predict_device + nig_step per step", ""]
for name in args.envs.split(","):
    med = {arm: [r["us_per_step_median"] for r in rows if r["env"] == name and r["arm"] == arm] for arm in "abc"}
    clk = [r["clock"].get("shader_clock_mhz", float("nan")) for r in rows if r["env"] == name]
    m = {arm: float(np.median(v)) for arm, v in med.items()}
    sp = {arm: max(v) - min(v) for arm, v in med.items()}
    lines.append(f"{name:19s} " + "  ".join(f"({arm}) {m[arm]:8.2f} ({min(med[arm]):.2f} .. {max(med[arm]):.2f})" for arm in "abc")
                 + f"  clock {min(clk):.0f} .. {max(clk):.0f} MHz")
    lines.append(f"{'':19s} (a)/(b) {m['a'] / m['b']:.3f} at equal MFMA counts;  (c)/(a) {m['c'] / m['a']:.2f};  "
                 f"(a) < (c) by more than both spreads: {m['c'] - m['a'] > sp['a'] + sp['c']}")
    lines.append("")
open(os.path.join(args.out_dir, "ab.txt"), "w").write("\n".join(lines))
print("\n".join(lines))
