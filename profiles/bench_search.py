#!/usr/bin/env python3
"""The fused safe-action search against the shield it extends (GPU box): a same-session A/B on one handle.

Per env (ChemicalReactor, PowerGrid) at --batch lanes, auto-reset on, HIP events around each of --launches launches after
--warmup, every series bracketed by bench.py's shader-clock stamps:
  plain    nig_rollout_mlp                                   the actor alone
  shield   nig_rollout_mlp_safe, repeated through the session (its own run-to-run spread); shield - plain = one critic pass,
           the yardstick of a candidate pass
  (a)      nig_rollout_mlp_search, threshold 2.0 (no block ever searches), N = 100: the price of the search-capable kernel over
           the shield -- expected: the one exposed fill per step behind the block's vote
  (b)      nig_rollout_mlp_search, threshold 0.0 (every live lane searches), N = 1, 8, 100: cost per candidate pass
           = (t(N) - t(a)) / N, against the yardstick
  (c)      nig_rollout_mlp_search, threshold 0.1 (the reference agent's default), N = 100, on the random critic: time and the
           share of 128-lane block-steps that ran candidate passes (from the flag rows)
Launches of the searching series are shortened to about --steps / (N + 1) steps, so that every launch costs about the same.

usage: python profiles/bench_search.py [--out-dir DIR]   ->  DIR/ab.jsonl (one line per series), DIR/ab.txt (the table)"""
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
ap.add_argument("--candidates", default="1,8,100")
ap.add_argument("--out-dir", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "search"))
args = ap.parse_args()
B, T, NL = args.batch, args.steps, args.launches
os.makedirs(args.out_dir, exist_ok=True)
rows = []


def net(D, O, seed, head):
    rng = np.random.default_rng(seed)
    return [(rng.normal(0, 0.02 / np.sqrt(D), (D, 256)).astype(np.float32), np.zeros(256, np.float32)),
            (rng.normal(0, 1 / 16, (256, 256)).astype(np.float32), np.zeros(256, np.float32)),
            (rng.normal(0, head, (256, O)).astype(np.float32), np.zeros(O, np.float32))]


def timed(env, name, series, launch, steps, N, extra=None):
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
    us = np.array([a.elapsed_time(b) for a, b in ev]) * 1e3 / steps
    row = {"env": name, "series": series, "n_candidates": N, "batch": B, "steps_per_launch": steps, "launches": NL,
           "us_per_step_median": float(np.median(us)), "us_per_step_min": float(us.min()), "us_per_step_max": float(us.max()),
           "clock": probe.read()}
    row.update(extra or {})
    rows.append(row)
    print(json.dumps(row), flush=True)
    return row


for name in args.envs.split(","):
    env = ni.make_batched(name, B, autoreset=True, tally=True)
    S, A = env.state_dim, env.action_dim
    ws, cw = net(S, A, 10, 1 / 16), net(S + A, 1, 20, 1 / 2)
    env.set_mlp_policy(ws)
    env.reset()
    timed(env, name, "plain", lambda: env.rollout_mlp(T), T, 0)
    shield = []

    def shield_once():
        env.set_mlp_safety(cw, 2.0)
        shield.append(timed(env, name, "shield", lambda: env.rollout_mlp_safe(T), T, 0, {"repeat": len(shield)}))
    shield_once()
    env.set_mlp_safety(cw, 2.0)
    timed(env, name, "search_never", lambda: env.rollout_mlp_search(T, 100), T, 100, {"threshold": 2.0})
    for N in [int(x) for x in args.candidates.split(",")]:
        env.set_mlp_safety(cw, 0.0)
        Ts = max(2, T // (N + 1))
        timed(env, name, "search_always", lambda: env.rollout_mlp_search(Ts, N), Ts, N, {"threshold": 0.0})
        if len(shield) < args.repeats:
            shield_once()
    env.set_mlp_safety(cw, 0.1)
    Ts = max(2, T // 101)
    fl = torch.zeros(Ts, env.ld, dtype=torch.int32, device=env.device)
    rw = torch.zeros(Ts, env.ld, dtype=torch.float32, device=env.device)
    r = timed(env, name, "search_default", lambda: env.rollout_mlp_search(Ts, 100, rw, fl), Ts, 100, {"threshold": 0.1})
    sh = (fl[:, :B] & ni._lib.FLAG_SHIELDED) != 0
    pad = (-B) % 128
    blocks = torch.nn.functional.pad(sh, (0, pad)).reshape(Ts, -1, 128).any(dim=2)
    r["lane_steps_searched"], r["block_steps_searched"] = float(sh.float().mean()), float(blocks.float().mean())
    while len(shield) < args.repeats:
        shield_once()
    env.close()

with open(os.path.join(args.out_dir, "ab.jsonl"), "w") as f:
    for r in rows:
        f.write(json.dumps(r) + "\n")
lines = [f"batch {B}, auto-reset, {NL} timed launches after {args.warmup}; microseconds per env step of the whole batch (median, min .. max over the launches)",
         f"{torch.cuda.get_device_name(0)}; {ni._lib.lib().nig_version().decode()}", ""]
for name in args.envs.split(","):
    mine = [r for r in rows if r["env"] == name]
    get = lambda s: [r for r in mine if r["series"] == s]
    plain = get("plain")[0]["us_per_step_median"]
    sh = [r["us_per_step_median"] for r in get("shield")]
    never = get("search_never")[0]
    yard = min(sh) - plain
    fmt = lambda r: f"{r['us_per_step_median']:10.2f} us ({r['us_per_step_min']:.2f} .. {r['us_per_step_max']:.2f}; {r['steps_per_launch']} steps per launch; {r['clock'].get('shader_clock_mhz', float('nan')):.0f} MHz)"
    lines.append(f"{name}: plain actor {plain:.2f} us; shield {', '.join(f'{x:.2f}' for x in sh)} us (spread of the repeats "
                 f"{100 * (max(sh) - min(sh)) / min(sh):.2f} %); one critic pass = shield - plain = {yard:.2f} us")
    lines.append(f"  (a) never searches, thr 2.0, N = 100   {fmt(never)}   ratio to the shield {never['us_per_step_median'] / max(sh):.3f} .. {never['us_per_step_median'] / min(sh):.3f}")
    for r in get("search_always"):
        N = r["n_candidates"]
        per = (r["us_per_step_median"] - never["us_per_step_median"]) / N
        lines.append(f"  (b) always searches, thr 0.0, N = {N:<3d}  {fmt(r)}   per candidate pass {per:.2f} us = {per / yard:.3f} x the yardstick")
    r = get("search_default")[0]
    lines.append(f"  (c) thr 0.1, N = 100, random critic    {fmt(r)}   lane-steps searched {100 * r['lane_steps_searched']:.1f} %, "
                 f"block-steps searched {100 * r['block_steps_searched']:.1f} %")
    lines.append("")
open(os.path.join(args.out_dir, "ab.txt"), "w").write("\n".join(lines))
print("\n".join(lines))
