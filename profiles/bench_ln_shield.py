#!/usr/bin/env python3
"""The fused shield of LayerNorm agents ("nig-mlp-ln-shield-v1") against its parts and against the host route it replaces (GPU box).

One session, one process, per env (ChemicalReactor, PowerGrid) at --batch lanes: four arms
  (a)  nig_rollout_mlp_safe with a LayerNorm actor and a LayerNorm critic (the new kernel), --steps steps per launch
  (b)  nig_rollout_mlp with the same LayerNorm actor (the kernel of "nig-mlp-ln-v1": half the passes)
  (c)  nig_rollout_mlp_safe with the plain (256, 256) actor and the plain critic: the plain shield, two blocks per CU
  (d)  the route the parent commit takes for such an agent: LayerNormMLPPolicy.predict_with_safety_device (torch GEMMs and
       reductions for actor and critic) + one env.step launch per step, as _evaluate_batched's host loop does it;
       --host-steps steps per timed series
ALTERNATE, --repeats rounds of --launches timed series each after --warmup, HIP events around every series, every arm bracketed by
bench.py's shader-clock stamps (profiles/bench_ln.py's procedure).  All arms run the same handle with auto-reset, from whatever
states the previous series left.  The table gives each arm's median per round, its spread over the rounds, (a) / (b) beside the ratio
of the two kernels' MFMA counts per step, (a) / (c), (d) / (a) and the routing condition: (a) below (d) by more than the two spreads
together.

Run it under a time limit of its own:
    timeout -k 10 420 python profiles/bench_ln_shield.py --out-dir DIR
usage: python profiles/bench_ln_shield.py [--out-dir DIR]   ->  DIR/ab.jsonl, DIR/ab.txt"""
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
ap.add_argument("--out-dir", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "ln_shield"))
args = ap.parse_args()
B, T, N = args.batch, args.steps, args.launches
os.makedirs(args.out_dir, exist_ok=True)
rows = []
ARMS = "abcd"


def network(IN, OUT, seed):
    rng = np.random.default_rng(seed)
    f = np.float32
    ws = [(rng.normal(0, 0.02 / np.sqrt(IN), (IN, 256)).astype(f), rng.normal(0, 0.05, 256).astype(f)),
          (rng.normal(0, 1.0 / 16, (256, 256)).astype(f), rng.normal(0, 0.05, 256).astype(f)),
          (rng.normal(0, 1.0 / 16, (256, OUT)).astype(f), np.zeros(OUT, f))]
    norms = [((1.0 + 0.3 * rng.normal(0, 1, 256)).astype(f), (0.2 * rng.normal(0, 1, 256)).astype(f)) for _ in range(2)]
    return ws, norms


def mfma_per_step(IN):
    """32 x 32 x 2 MFMAs a lane pair issues per step for one LayerNorm network of IN inputs (the head's small MFMAs apart): eight
    layer-1 tiles of (padded IN) / 2 weight records and a bias record, eight layer-2 tiles of 129 records"""
    return 8 * (((IN + 1) & ~1) // 2 + 1) + 8 * 129


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


ratio = {}
for name in args.envs.split(","):
    env = ni.make_batched(name, B, autoreset=True, tally=True)
    S, A = env.state_dim, env.action_dim
    ws, norms = network(S, A, 11)
    cw, cn = network(S + A, 1, 12)
    pol = ni.LayerNormMLPPolicy(ws, norms, device=env.device, safety_weights=cw, safety_norms=cn, constraint_threshold=0.5)
    ratio[name] = (mfma_per_step(S) + mfma_per_step(S + A)) / mfma_per_step(S)
    env.reset()

    def host_loop():
        for _ in range(args.host_steps):
            env.step(pol.predict_with_safety_device(env.obs)[0], layout="aos")
    for rnd in range(args.repeats):
        env.set_mlp_policy_ln(pol)
        env.set_mlp_safety_ln(pol, 0.5)
        timed(env, name, "a", rnd, lambda: env.rollout_mlp_safe(T), T)
        timed(env, name, "b", rnd, lambda: env.rollout_mlp(T), T)
        env.set_mlp_policy(ws)
        env.set_mlp_safety(cw, 0.5)
        timed(env, name, "c", rnd, lambda: env.rollout_mlp_safe(T), T)
        timed(env, name, "d", rnd, host_loop, args.host_steps)
    env.close()

with open(os.path.join(args.out_dir, "ab.jsonl"), "w") as f:
    for r in rows:
        f.write(json.dumps(r) + "\n")
lines = [f"batch {B}; (a), (b), (c): {T} steps per launch, (d): {args.host_steps} host steps per series; {args.repeats} alternating rounds of {N} timed "
         f"series after {args.warmup}; microseconds per step, median of a round (min .. max over the rounds' medians)",
         f"{torch.cuda.get_device_name(0)}; {ni._lib.lib().nig_version().decode()}",
         "(a) nig_rollout_mlp_safe, LayerNorm actor + LayerNorm critic   (b) nig_rollout_mlp, the same LayerNorm actor",
         "(c) nig_rollout_mlp_safe, plain 256 x 256 actor + critic        (d) predict_with_safety_device + nig_step per step", ""]
for name in args.envs.split(","):
    med = {arm: [r["us_per_step_median"] for r in rows if r["env"] == name and r["arm"] == arm] for arm in ARMS}
    clk = [r["clock"].get("shader_clock_mhz", float("nan")) for r in rows if r["env"] == name]
    m = {arm: float(np.median(v)) for arm, v in med.items()}
    sp = {arm: max(v) - min(v) for arm, v in med.items()}
    lines.append(f"{name:19s} " + "  ".join(f"({arm}) {m[arm]:8.2f} ({min(med[arm]):.2f} .. {max(med[arm]):.2f})" for arm in ARMS)
                 + f"  clock {min(clk):.0f} .. {max(clk):.0f} MHz")
    lines.append(f"{'':19s} (a)/(b) {m['a'] / m['b']:.3f} beside an MFMA-count ratio of {ratio[name]:.3f};  (a)/(c) {m['a'] / m['c']:.3f};  "
                 f"(d)/(a) {m['d'] / m['a']:.2f};  (a) < (d) by more than both spreads: {m['d'] - m['a'] > sp['a'] + sp['d']}")
    lines.append("")
open(os.path.join(args.out_dir, "ab.txt"), "w").write("\n".join(lines))
print("\n".join(lines))
