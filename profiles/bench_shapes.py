#!/usr/bin/env python3
"""The shaped MFMA actor ("nig-mlp-shape-v1") against the 256 x 256 kernel and against the host route it replaces (GPU box).

One session, one process, per env (ChemicalReactor, PowerGrid) at --batch lanes and per shape class: three arms
  (a)  nig_rollout_mlp with the class's actor installed by nig_set_mlp_policy_dims (the new kernel), --steps steps per launch
  (b)  nig_rollout_mlp with the (256, 256) actor (what zero-padding into the existing kernel costs)
  (c)  the route the parent commit takes for that agent: MLPPolicy.predict_device (torch GEMMs) + one env.step launch per step,
       as _evaluate_batched's host loop does it; --host-steps steps per timed series
ALTERNATE, --repeats rounds of --launches timed series each after --warmup, HIP events around every series, every arm bracketed by
bench.py's shader-clock stamps.  All arms run the same handle with auto-reset, from whatever states the previous series left: the
time per step does not depend on the state.  The table gives each arm's median per round, its spread over the rounds, the ratio
(a) / (b) beside the ratio of the 32 x 32 x 2 MFMA counts per step, (c) / (a), and the issue's conditions: (a) below (c), and for
128x128 below (b), by more than the two spreads together.

Run it under a time limit of its own, one process per class:
    timeout -k 10 300 python profiles/bench_shapes.py --classes 128x128 --out-dir DIR
usage: python profiles/bench_shapes.py [--classes A,B] [--out-dir DIR]   ->  DIR/ab_<classes>.jsonl, DIR/ab_<classes>.txt"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import neorl_industrial_gym_amd as ni
from bench import ClockProbe

CLASSES = {"128x128": (128, 128), "512x256": (512, 256), "512x512": (512, 512), "256x256x256": (256, 256, 256)}
ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=65536)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--host-steps", type=int, default=20)
ap.add_argument("--launches", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--envs", default="ChemicalReactor-v0,PowerGrid-v0")
ap.add_argument("--classes", default=",".join(CLASSES))
ap.add_argument("--out-dir", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "shapes"))
args = ap.parse_args()
B, T, N = args.batch, args.steps, args.launches
os.makedirs(args.out_dir, exist_ok=True)
rows = []


def actor(S, A, dims, seed):
    rng = np.random.default_rng(seed)
    ws, K = [], S
    for H in dims:
        ws.append((rng.normal(0, (0.02 if K == S else 1.0) / np.sqrt(K), (K, H)).astype(np.float32), np.zeros(H, np.float32)))
        K = H
    ws.append((rng.normal(0, 1.0 / np.sqrt(K), (K, A)).astype(np.float32), np.zeros(A, np.float32)))
    return ws


def mfmas(S, dims):
    """32 x 32 x 2 instructions per step of the padded network (counted from the stream)"""
    t = [d // 32 for d in dims]
    return t[0] * (S // 2 + 1) + sum(t[l] * (16 * t[l - 1] + 1) for l in range(1, len(t)))


def timed(env, name, cls, arm, rnd, series, steps):
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
    row = {"env": name, "class": cls, "arm": arm, "round": rnd, "batch": B, "steps_per_series": steps, "series": N,
           "us_per_step_median": float(np.median(us)), "us_per_step_min": float(us.min()), "us_per_step_max": float(us.max()), "clock": probe.read()}
    rows.append(row)
    print(json.dumps(row), flush=True)


for name in args.envs.split(","):
    env = ni.make_batched(name, B, autoreset=True, tally=True)
    S, A = env.state_dim, env.action_dim
    reference = actor(S, A, (256, 256), 10)
    env.reset()
    for cls in args.classes.split(","):
        ws = actor(S, A, CLASSES[cls], 11)
        pol = ni.MLPPolicy(ws, device=env.device)

        def host_loop():
            for _ in range(args.host_steps):
                env.step(pol.predict_device(env.obs), layout="aos")
        for rnd in range(args.repeats):
            env.set_mlp_policy_dims(ws)
            timed(env, name, cls, "a", rnd, lambda: env.rollout_mlp(T), T)
            env.set_mlp_policy(reference)
            timed(env, name, cls, "b", rnd, lambda: env.rollout_mlp(T), T)
            timed(env, name, cls, "c", rnd, host_loop, args.host_steps)
    env.close()

tag = args.classes.replace(",", "_")
with open(os.path.join(args.out_dir, f"ab_{tag}.jsonl"), "w") as f:
    for r in rows:
        f.write(json.dumps(r) + "\n")
lines = [f"batch {B}; (a), (b): {T} steps per launch, (c): {args.host_steps} host steps per series; {args.repeats} alternating rounds of {N} timed series "
         f"after {args.warmup}; microseconds per step, median of a round (min .. max over the rounds' medians)",
         f"{torch.cuda.get_device_name(0)}; {ni._lib.lib().nig_version().decode()}", ""]
for name in args.envs.split(","):
    S = int(ni._lib.env_spec(ni.batched.ENV_IDS[name]).state_dim)
    for cls in args.classes.split(","):
        med = {arm: [r["us_per_step_median"] for r in rows if r["env"] == name and r["class"] == cls and r["arm"] == arm] for arm in "abc"}
        clk = [r["clock"].get("shader_clock_mhz", float("nan")) for r in rows if r["env"] == name and r["class"] == cls]
        m = {arm: float(np.median(v)) for arm, v in med.items()}
        sp = {arm: max(v) - min(v) for arm, v in med.items()}
        expected = mfmas(S, CLASSES[cls]) / mfmas(S, (256, 256))
        lines.append(f"{name:19s} {cls:12s} " + "  ".join(f"({arm}) {m[arm]:8.2f} ({min(med[arm]):.2f} .. {max(med[arm]):.2f})" for arm in "abc")
                     + f"  clock {min(clk):.0f} .. {max(clk):.0f} MHz")
        lines.append(f"{'':32s} (a)/(b) measured {m['a'] / m['b']:.3f}, from the MFMA count {expected:.3f} ({mfmas(S, CLASSES[cls])} / {mfmas(S, (256, 256))});  "
                     f"(c)/(a) {m['c'] / m['a']:.2f};  (a) < (c) by more than both spreads: {m['c'] - m['a'] > sp['a'] + sp['c']};  "
                     f"(a) < (b) by more than both spreads: {m['b'] - m['a'] > sp['a'] + sp['b']}")
    lines.append("")
open(os.path.join(args.out_dir, f"ab_{tag}.txt"), "w").write("\n".join(lines))
print("\n".join(lines))
