#!/usr/bin/env python3
"""The fused ensemble actor against the single actor and against the device path an ensemble takes without it (GPU box).

One session, one box, per env (ChemicalReactor, PowerGrid) at --batch lanes, --steps env.step per launch, HIP events around
each of --launches launches after --warmup, every series bracketed by bench.py's shader-clock stamps:
  (a) single_actor     nig_rollout_mlp, repeated --repeats times through the session (its own run-to-run spread)
  (b) ensemble         nig_rollout_mlp_ensemble at K = 1, 2, 5, 8 members for "mean" (float64 action) and "voting" (float32)
  (c) torch_ensemble   K MLPPolicy.predict_device passes, the average in torch (float64), benv.step on float64 actions
Per series: median / min / max microseconds per step over the launches, useful MFMA TFLOP/s (K x the actor's flop count / time).
The acceptance figure of the feature is t(K = 5) <= 5 x (a), both from this session.

usage: python profiles/bench_ensemble.py [--out-dir DIR]   ->  DIR/ab.jsonl (one line per series), DIR/ab.txt (the table)"""
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
ap.add_argument("--launches", type=int, default=20)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--torch-steps", type=int, default=50)
ap.add_argument("--envs", default="ChemicalReactor-v0,PowerGrid-v0")
ap.add_argument("--members", default="1,2,5,8")
ap.add_argument("--out-dir", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "ensemble"))
args = ap.parse_args()
B, T, N = args.batch, args.steps, args.launches
os.makedirs(args.out_dir, exist_ok=True)
rows = []


def actor(S, A, seed):
    rng = np.random.default_rng(seed)
    return [(rng.normal(0, 0.02 / np.sqrt(S), (S, 256)).astype(np.float32), np.zeros(256, np.float32)),
            (rng.normal(0, 1 / 16, (256, 256)).astype(np.float32), np.zeros(256, np.float32)),
            (rng.normal(0, 1 / 16, (256, A)).astype(np.float32), np.zeros(A, np.float32))]


def timed(env, name, series, launch, steps, K, flops, extra=None):
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
    us = np.array([a.elapsed_time(b) for a, b in ev]) * 1e3 / steps
    row = {"env": name, "series": series, "members": K, "batch": B, "steps_per_launch": steps, "launches": N,
           "us_per_step_median": float(np.median(us)), "us_per_step_min": float(us.min()), "us_per_step_max": float(us.max()),
           "useful_mfma_TFLOPs": float(K * flops * B / np.median(us) / 1e6), "clock": probe.read()}
    row.update(extra or {})
    rows.append(row)
    print(json.dumps(row), flush=True)
    return row


for name in args.envs.split(","):
    env = ni.make_batched(name, B, autoreset=True, tally=True)
    S, A = env.state_dim, env.action_dim
    flops = 2.0 * (S * 256 + 256 * 256 + 256 * A)
    nets = [actor(S, A, 10 + k) for k in range(8)]
    env.set_mlp_policy(nets[0])
    env.reset()
    Ks = [int(k) for k in args.members.split(",")]
    singles = [timed(env, name, "single_actor", lambda: env.rollout_mlp(T), T, 1, flops, {"repeat": 0})]
    for method in ("mean", "voting"):
        for K in Ks:
            pol = ni.EnsemblePolicy(nets[:K], method=method, device=env.device)
            pol.install(env)
            timed(env, name, f"ensemble_{method}", lambda: env.rollout_mlp_ensemble(T), T, K, flops)
        if len(singles) < args.repeats:
            singles.append(timed(env, name, "single_actor", lambda: env.rollout_mlp(T), T, 1, flops, {"repeat": len(singles)}))
    for K in Ks:
        if K < 2:
            continue
        pol = ni.EnsemblePolicy(nets[:K], method="mean", device=env.device)
        Tt = args.torch_steps

        def loop():
            for _ in range(Tt):
                env.step(pol.predict_device(env.obs), layout="aos")
        timed(env, name, "torch_ensemble_mean", loop, Tt, K, flops)
    while len(singles) < args.repeats:
        singles.append(timed(env, name, "single_actor", lambda: env.rollout_mlp(T), T, 1, flops, {"repeat": len(singles)}))
    env.close()

with open(os.path.join(args.out_dir, "ab.jsonl"), "w") as f:
    for r in rows:
        f.write(json.dumps(r) + "\n")
lines = [f"batch {B}, {T} steps per launch, {N} timed launches after {args.warmup}; microseconds per step (median, min .. max over the launches)",
         f"{torch.cuda.get_device_name(0)}; {ni._lib.lib().nig_version().decode()}", ""]
for name in args.envs.split(","):
    mine = [r for r in rows if r["env"] == name]
    a = [r["us_per_step_median"] for r in mine if r["series"] == "single_actor"]
    lines.append(f"{name}: single actor (a) {', '.join(f'{x:.2f}' for x in a)} us  (spread of the repeats {100 * (max(a) - min(a)) / min(a):.2f} %)")
    for r in mine:
        if r["series"] == "single_actor":
            continue
        K = r["members"]
        clk = r["clock"].get("shader_clock_mhz", float("nan"))
        lines.append(f"  {r['series']:22s} K={K}  {r['us_per_step_median']:9.2f} us ({r['us_per_step_min']:.2f} .. {r['us_per_step_max']:.2f})  "
                     f"t/K {r['us_per_step_median'] / K:8.2f}  t / (K x (a) max) {r['us_per_step_median'] / (K * max(a)):.3f}  "
                     f"t / (K x (a) min) {r['us_per_step_median'] / (K * min(a)):.3f}  {r['useful_mfma_TFLOPs']:7.1f} TFLOP/s  {clk:.0f} MHz")
    for method in ("mean", "voting"):
        t5 = [r["us_per_step_median"] for r in mine if r["series"] == f"ensemble_{method}" and r["members"] == 5]
        if t5 and a:
            verdict = "met" if t5[0] <= 5 * min(a) else ("inside the spread of (a)" if t5[0] <= 5 * max(a) else "NOT met")
            lines.append(f"  acceptance t(5) <= 5 x (a), {method}: {t5[0]:.2f} us against {5 * min(a):.2f} .. {5 * max(a):.2f} us: {verdict}")
    lines.append("")
open(os.path.join(args.out_dir, "ab.txt"), "w").write("\n".join(lines))
print("\n".join(lines))
