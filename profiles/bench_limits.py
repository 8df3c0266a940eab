#!/usr/bin/env python3
"""The closed-loop rollouts under added box constraints against their parents (GPU box): what does "nig-limits-v1" cost per step?

One session, one box, per env (ChemicalReactor, PowerGrid) at --batch lanes, --steps env.step per launch, HIP events around each
of --launches launches (--policy-launches for the policy series, whose launches are a millisecond: a timed window of a tenth of a
second and more) after --warmup, every series bracketed by bench.py's shader-clock stamps.  The series alternate A B A B
through --repeats rounds, so a drift of the box shows as the spread of a series' own repeats:
  mlp              nig_rollout_mlp                       (A: the parent's entry point, same process, no limits installed)
  mlp_limited_1/4  nig_rollout_mlp_limited               one / four added constraints
  policy           nig_rollout_policy, "MPC" proportional law (the batch's own kernel form: three-wave / paired at this size)
  policy_onewave   nig_rollout_policy with nig_tune(split_blocks = 0): the ONE-WAVE kernel, the limited kernel's parent
  policy_limited_1/4  nig_rollout_policy_limited         (always the one-wave form)
The constraints are boxes over one state row and one action row each, with bounds that a few per cent of the steps violate (none
critical: the episodes keep the parents' lengths).  No outputs are written by any series (the rollouts' own default), so the
figures are the kernels' compute cost.

usage: python profiles/bench_limits.py [--out-dir DIR]   ->  DIR/ab.jsonl (one line per series), DIR/ab.txt (the table)"""
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
ap.add_argument("--policy-launches", type=int, default=200)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--envs", default="ChemicalReactor-v0,PowerGrid-v0")
ap.add_argument("--out-dir", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "limits"))
args = ap.parse_args()
B, T, N = args.batch, args.steps, args.launches
os.makedirs(args.out_dir, exist_ok=True)
rows = []


def actor(S, A, seed):
    rng = np.random.default_rng(seed)
    return [(rng.normal(0, 0.02 / np.sqrt(S), (S, 256)).astype(np.float32), np.zeros(256, np.float32)),
            (rng.normal(0, 1 / 16, (256, 256)).astype(np.float32), np.zeros(256, np.float32)),
            (rng.normal(0, 1 / 16, (256, A)).astype(np.float32), np.zeros(A, np.float32))]


def timed(env, name, series, launch, repeat, N=N):
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


SERIES = (("mlp", None), ("mlp_limited_1", "mlp"), ("mlp_limited_4", "mlp"), ("policy", None), ("policy_onewave", "policy"),
          ("policy_limited_1", "policy_onewave"), ("policy_limited_4", "policy_onewave"))

for name in args.envs.split(","):
    env = ni.make_batched(name, B, autoreset=True, tally=True)
    S, A = env.state_dim, env.action_dim
    env.set_mlp_policy(actor(S, A, 10))
    env.set_policy(ni.mpc_agent(S, A))
    env.reset()
    state = env.get_state().cpu().numpy()
    boxes = []
    for c in range(4):      # state row c within its 2 % .. 98 % quantiles at reset, action row c % A within [-0.9, 0.9]
        lo, hi = np.quantile(state[:, c].astype(np.float64), [0.02, 0.98])
        boxes.append(ni.BoxConstraint(f"box_{c}", {("state", c): (lo, max(hi, lo)), ("action", c % A): (-0.9, 0.9)}, -1.0))

    def limited(fn, n):
        def go():
            fn(T)
        for b in list(env.safety_constraints):
            if isinstance(b, ni.BoxConstraint):
                env.remove_safety_constraint(b.name)
        for b in boxes[:n]:
            env.add_safety_constraint(b)
        return go

    def parent(fn):
        for b in list(env.safety_constraints):
            if isinstance(b, ni.BoxConstraint):
                env.remove_safety_constraint(b.name)
        return lambda: fn(T)

    NP = args.policy_launches
    for rep in range(args.repeats):
        timed(env, name, "mlp", parent(env.rollout_mlp), rep)
        for n in (1, 4):
            timed(env, name, f"mlp_limited_{n}", limited(env.rollout_mlp_limited, n), rep)
        timed(env, name, "policy", parent(env.rollout_policy), rep, NP)
        ni.tune(split_blocks=0)                      # the one-wave form: the knob is set around the series, not inside its timed launches
        try:
            timed(env, name, "policy_onewave", parent(env.rollout_policy), rep, NP)
        finally:
            ni.tune(split_blocks=-1)
        for n in (1, 4):
            timed(env, name, f"policy_limited_{n}", limited(env.rollout_policy_limited, n), rep, NP)
    env.close()

with open(os.path.join(args.out_dir, "ab.jsonl"), "w") as f:
    for r in rows:
        f.write(json.dumps(r) + "\n")
lines = [f"batch {B}, {T} steps per launch, {N} timed launches ({args.policy_launches} for the policy series) after {args.warmup}, {args.repeats} alternating repeats; microseconds per step, "
         "median of the launches, per repeat", f"{torch.cuda.get_device_name(0)}; {ni._lib.lib().nig_version().decode()}", ""]
for name in args.envs.split(","):
    mine = [r for r in rows if r["env"] == name]
    med = {}
    for r in mine:
        med.setdefault(r["series"], []).append(r["us_per_step_median"])
    lines.append(name)
    for series, base in SERIES:
        x = med[series]
        clk = [r["clock"].get("shader_clock_mhz", float("nan")) for r in mine if r["series"] == series]
        txt = f"  {series:26s} {', '.join(f'{v:8.2f}' for v in x)} us   spread {100 * (max(x) - min(x)) / min(x):5.2f} %   {np.median(clk):.0f} MHz"
        if base:
            txt += f"   / {base}: {np.median(x) / np.median(med[base]):.3f} (medians of the repeats)"
        lines.append(txt)
    lines.append("")
open(os.path.join(args.out_dir, "ab.txt"), "w").write("\n".join(lines))
print("\n".join(lines))
