#!/usr/bin/env python3
"""The distributional safety critic ("nig-categorical-v1") against the sigmoid shield it shares a slot with (GPU box): a
same-session A/B on one handle.

Per env (ChemicalReactor, PowerGrid) at --batch lanes, auto-reset on, HIP events around each of --launches launches after
--warmup, every series bracketed by bench.py's shader-clock stamps, threshold 2.0 throughout (no lane is shielded, so both
critics drive the same trajectories):
  plain    nig_rollout_mlp                                       the actor alone
  shield   nig_rollout_mlp_safe with the sigmoid critic, repeated through the session (its own run-to-run spread): the parent
  cat      nig_rollout_mlp_safe with the 51-atom categorical critic, as often, interleaved with the sigmoid repeats
  eval     nig_mlp_violation_prob at n = 65 536 and 1 048 576 columns (microseconds per call, and per 65 536 columns)
Expectation from the MFMA count (cycles per wave): the sigmoid critic's pass is layer 1 (8 tiles x (width / 2 + 1) x 64), layer 2
(8 x 129 x 64 = 66 048) and the 4 x 4 x 1 head (8 x 16 x 8 = 1 024): 71 680 for ChemicalReactor, 77 824 for PowerGrid.  The categorical
head is four 32-cycle instructions per hidden register, 8 x 16 x 128 = 16 384: a pass of 87 040 / 93 184 cycles, i.e.
(cat - plain) / (shield - plain) = 1.214 / 1.197 and, a critic pass being about half a step, a step of about 1.11 / 1.10 x the parent's.

The parts of the pass (profiles/categorical/parts.txt): the same run on libraries whose categorical units are compiled with
-DNIG_CAT_PARTS=1 / 2 / 3 (profiles/mkvariant.sh catparts<k> "categorical_cr categorical_pg" -DNIG_CAT_PARTS=<k>; NIG_LIB_PATH), with
--repeats 1 --eval-n "".

usage: python profiles/bench_categorical.py [--out-dir DIR]   ->  DIR/ab.jsonl (one line per series), DIR/ab.txt (the table)"""
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
ap.add_argument("--launches", type=int, default=8)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--atoms", type=int, default=51)
ap.add_argument("--envs", default="ChemicalReactor-v0,PowerGrid-v0")
ap.add_argument("--eval-n", default="65536,1048576")
ap.add_argument("--out-dir", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "categorical"))
args = ap.parse_args()
B, T, NL = args.batch, args.steps, args.launches
os.makedirs(args.out_dir, exist_ok=True)
rows = []


def net(D, O, seed, head):
    rng = np.random.default_rng(seed)
    return [(rng.normal(0, 0.02 / np.sqrt(D), (D, 256)).astype(np.float32), np.zeros(256, np.float32)),
            (rng.normal(0, 1 / 16, (256, 256)).astype(np.float32), np.zeros(256, np.float32)),
            (rng.normal(0, head, (256, O)).astype(np.float32), np.zeros(O, np.float32))]


def timed(env, name, series, launch, per, extra=None):
    """`per`: what one launch is divided by (its steps; 1 for the evaluator: microseconds per call)"""
    probe = ClockProbe(ni, torch, env.device)
    for _ in range(args.warmup):
        launch()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(NL)]
    probe.stamp(0)
    for a, b in ev:
        a.record(); launch(); b.record()
    probe.stamp(1)
    torch.cuda.synchronize()
    us = np.array([a.elapsed_time(b) for a, b in ev]) * 1e3 / per
    row = {"env": name, "series": series, "batch": B, "per": per, "launches": NL, "us_median": float(np.median(us)),
           "us_min": float(us.min()), "us_max": float(us.max()), "clock": probe.read()}
    row.update(extra or {})
    rows.append(row)
    print(json.dumps(row), flush=True)
    return row


for name in args.envs.split(","):
    env = ni.make_batched(name, B, autoreset=True, tally=True)
    S, A = env.state_dim, env.action_dim
    ws, sw, cw = net(S, A, 10, 1 / 16), net(S + A, 1, 20, 1 / 2), net(S + A, args.atoms, 30, 1 / 8)
    env.set_mlp_policy(ws)
    env.reset()
    timed(env, name, "plain", lambda: env.rollout_mlp(T), T)
    for rep in range(args.repeats):
        env.set_mlp_safety(sw, 2.0)
        timed(env, name, "shield", lambda: env.rollout_mlp_safe(T), T, {"repeat": rep})
        env.set_mlp_safety_categorical(cw, 2.0)
        timed(env, name, "cat", lambda: env.rollout_mlp_safe(T), T, {"repeat": rep, "atoms": args.atoms})
    for n in [int(x) for x in args.eval_n.split(",") if x]:
        obs = torch.randn(S, n, device=env.device)
        act = torch.rand(A, n, device=env.device) * 2 - 1
        out = torch.empty(n, device=env.device)
        timed(env, name, "eval", lambda: env.violation_prob(obs, act, out, layout="soa"), 1, {"n": n, "atoms": args.atoms})
    env.close()

with open(os.path.join(args.out_dir, "ab.jsonl"), "w") as f:
    for r in rows:
        f.write(json.dumps(r) + "\n")
lines = [f"batch {B}, auto-reset, {NL} timed launches of {T} steps after {args.warmup}; microseconds per env step of the whole batch (median, min .. max over the launches)",
         f"{torch.cuda.get_device_name(0)}; {ni._lib.lib().nig_version().decode()}; {args.atoms} atoms", ""]
for name in args.envs.split(","):
    mine = [r for r in rows if r["env"] == name]
    get = lambda s: [r for r in mine if r["series"] == s]
    plain = get("plain")[0]["us_median"]
    sh, ct = [r["us_median"] for r in get("shield")], [r["us_median"] for r in get("cat")]
    mhz = lambda r: r["clock"].get("shader_clock_mhz", float("nan"))
    lines.append(f"{name}: plain actor {plain:.2f} us")
    lines.append(f"  sigmoid shield (the parent)  {', '.join(f'{x:.2f}' for x in sh)} us   spread of the repeats {100 * (max(sh) - min(sh)) / min(sh):.2f} %   "
                 f"({', '.join(f'{mhz(r):.0f}' for r in get('shield'))} MHz)")
    lines.append(f"  categorical shield           {', '.join(f'{x:.2f}' for x in ct)} us   spread of the repeats {100 * (max(ct) - min(ct)) / min(ct):.2f} %   "
                 f"({', '.join(f'{mhz(r):.0f}' for r in get('cat'))} MHz)")
    ms, mc = float(np.median(sh)), float(np.median(ct))
    lines.append(f"  step: categorical / sigmoid = {mc / ms:.3f};  critic pass: (cat - plain) / (shield - plain) = {(mc - plain) / (ms - plain):.3f}  "
                 f"({mc - plain:.2f} us against {ms - plain:.2f} us)")
    for r in get("eval"):
        lines.append(f"  nig_mlp_violation_prob n = {r['n']:>8d}: {r['us_median']:10.2f} us per call ({r['us_min']:.2f} .. {r['us_max']:.2f}), "
                     f"{r['us_median'] * 65536 / r['n']:.2f} us per 65 536 columns")
    lines.append("")
open(os.path.join(args.out_dir, "ab.txt"), "w").write("\n".join(lines))
print("\n".join(lines))
