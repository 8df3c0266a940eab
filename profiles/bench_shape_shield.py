#!/usr/bin/env python3
"""The fused shield of shaped agents ("nig-mlp-shape-shield-v1") against its parts and against the host route it replaces (GPU box).

One session, one process, per env (ChemicalReactor, PowerGrid) and per shape class at --batch lanes: four arms
  (a)  nig_rollout_mlp_safe with a shaped actor and a shaped critic of the class (the new kernel), --steps steps per launch
  (b)  nig_rollout_mlp with the same shaped actor (the kernel of "nig-mlp-shape-v1": half the passes)
  (c)  nig_rollout_mlp_safe with the plain (256, 256) actor and the plain critic: the plain shield
  (d)  the route the parent commit takes for such an agent: MLPPolicy.predict_with_safety_device (torch GEMMs for actor and
       critic) + one env.step launch per step, as _evaluate_batched's host loop does it; --host-steps steps per timed series
ALTERNATE, --repeats rounds of --launches timed series each after --warmup, HIP events around every series, every arm bracketed by
bench.py's shader-clock stamps (profiles/bench_ln_shield.py's procedure).  All arms run the same handle with auto-reset, from
whatever states the previous series left.  The table gives each arm's median per round, its spread over the rounds, (a) / (b) beside
the ratio of the two kernels' MFMA counts per step (the plans' 32 x 32 x 2 instructions and the heads' small ones), (a) / (c),
(d) / (a) and the routing condition: EVERY round of (a) below EVERY round of (d).

Run it under a time limit of its own:
    timeout -k 10 420 python profiles/bench_shape_shield.py --out-dir DIR
usage: python profiles/bench_shape_shield.py [--out-dir DIR]   ->  DIR/ab.jsonl, DIR/ab.txt"""
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
ap.add_argument("--out-dir", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "shape_shield"))
args = ap.parse_args()
B, T, N = args.batch, args.steps, args.launches
os.makedirs(args.out_dir, exist_ok=True)
rows = []
ARMS = "abcd"


def network(IN, OUT, dims, seed):
    rng = np.random.default_rng(seed)
    f = np.float32
    ws, K = [], IN
    for i, H in enumerate(dims):
        ws.append((rng.normal(0, (0.02 if i == 0 else 1.0) / np.sqrt(K), (K, H)).astype(f), rng.normal(0, 0.05, H).astype(f)))
        K = H
    ws.append((rng.normal(0, 1.0 / np.sqrt(K), (K, OUT)).astype(f), np.zeros(OUT, f)))
    return ws


def mfma_per_step(dims, IN):
    """MFMAs a lane pair issues per step for one network of the class at IN inputs: shape_mfmas of csrc/nig_mlp_shape_stream.hpp (32 x
    32 x 2: layer-1 tiles of padded IN / 2 weight records and a bias record, later tiles of 16 per input tile and a bias record) and
    the head's 16 per last-layer tile and one for its bias"""
    t = [d // 32 for d in dims]
    n = t[0] * (((IN + 1) & ~1) // 2 + 1)
    for l in range(1, len(t)):
        n += t[l] * (16 * t[l - 1] + 1)
    return n, 16 * t[-1] + 1


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


ratio = {}
for name in args.envs.split(","):
    env = ni.make_batched(name, B, autoreset=True, tally=True)
    S, A = env.state_dim, env.action_dim
    ref_ws, ref_cw = network(S, A, (256, 256), 11), network(S + A, 1, (256, 256), 12)
    env.reset()
    for cls in args.classes.split(","):
        dims = CLASSES[cls]
        ws, cw = network(S, A, dims, 13), network(S + A, 1, dims, 14)
        pol = ni.MLPPolicy(ws, device=env.device, safety_weights=cw, constraint_threshold=0.5)
        (ma, ha), (mc, hc) = mfma_per_step(dims, S), mfma_per_step(dims, S + A)
        ratio[name, cls] = ((ma + mc) / ma, (ma + ha + mc + hc) / (ma + ha))

        def host_loop():
            for _ in range(args.host_steps):
                env.step(pol.predict_with_safety_device(env.obs)[0], layout="aos")
        for rnd in range(args.repeats):
            env.set_mlp_policy_dims(ws)
            env.set_mlp_safety_dims(cw, 0.5)
            timed(env, name, cls, "a", rnd, lambda: env.rollout_mlp_safe(T), T)
            timed(env, name, cls, "b", rnd, lambda: env.rollout_mlp(T), T)
            env.set_mlp_policy(ref_ws)
            env.set_mlp_safety(ref_cw, 0.5)
            timed(env, name, cls, "c", rnd, lambda: env.rollout_mlp_safe(T), T)
            timed(env, name, cls, "d", rnd, host_loop, args.host_steps)
    env.close()

with open(os.path.join(args.out_dir, "ab.jsonl"), "w") as f:
    for r in rows:
        f.write(json.dumps(r) + "\n")
lines = [f"batch {B}; (a), (b), (c): {T} steps per launch, (d): {args.host_steps} host steps per series; {args.repeats} alternating rounds of {N} timed "
         f"series after {args.warmup}; microseconds per step, median of a round (min .. max over the rounds' medians)",
         f"{torch.cuda.get_device_name(0)}; {ni._lib.lib().nig_version().decode()}",
         "(a) nig_rollout_mlp_safe, shaped actor + shaped critic of the class   (b) nig_rollout_mlp, the same shaped actor",
         "(c) nig_rollout_mlp_safe, plain 256 x 256 actor + critic              (d) predict_with_safety_device + nig_step per step",
         "expected (a)/(b): the MFMA-count ratio of the two kernels, heads included (before the heads in brackets)", ""]
for name in args.envs.split(","):
    for cls in args.classes.split(","):
        sel = [r for r in rows if r["env"] == name and r["class"] == cls]
        med = {arm: [r["us_per_step_median"] for r in sel if r["arm"] == arm] for arm in ARMS}
        clk = [r["clock"].get("shader_clock_mhz", float("nan")) for r in sel]
        m = {arm: float(np.median(v)) for arm, v in med.items()}
        lines.append(f"{name:19s} {cls:12s} " + "  ".join(f"({arm}) {m[arm]:8.2f} ({min(med[arm]):.2f} .. {max(med[arm]):.2f})" for arm in ARMS)
                     + f"  clock {min(clk):.0f} .. {max(clk):.0f} MHz")
        lines.append(f"{'':32s} (a)/(b) {m['a'] / m['b']:.3f} beside an MFMA-count ratio of {ratio[name, cls][1]:.3f} [{ratio[name, cls][0]:.3f}];  "
                     f"(a)/(c) {m['a'] / m['c']:.3f};  (d)/(a) {m['d'] / m['a']:.2f};  every round of (a) below every round of (d): {max(med['a']) < min(med['d'])}")
    lines.append("")
open(os.path.join(args.out_dir, "ab.txt"), "w").write("\n".join(lines))
print("\n".join(lines))
