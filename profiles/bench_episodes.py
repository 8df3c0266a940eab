#!/usr/bin/env python3
"""Per-episode records (GPU box), two same-session A/B measurements:

 1. collect   nig_collect_episodes on [--steps, --batch] reward / flag rows (the rows of one rollout_sampled launch of an
              auto-reset handle) against the torch reduction uniform_action_statistics runs on the same rows (about fifteen passes
              over [P, B] temporaries; it returns sums, no per-episode value).  HIP events around each of --launches calls after
              --warmup, the two series alternating through --repeats rounds.
 2. evaluate  ni.evaluate_episodes in QUOTA mode (auto-reset handle, --chunk steps per launch, every lane plays
              n_episodes / batch episodes back to back) against the parent commit's ni.evaluate_with_safety ROUNDS (one episode per
              lane per round, a round = max_episode_steps steps), same n_episodes, same mpc_agent, on RobotAssembly (short
              episodes) and ChemicalReactor (episodes that mostly run to the cap).  Host wall clock around the whole call, ending in a
              device synchronise; a fresh handle per call, made outside the clock; alternating A B through --repeats rounds after one warm-up call each.
Every series is bracketed by bench.py's shader-clock stamps; the DPM state (sclk / mclk / power) is sampled once per series.

usage: python profiles/bench_episodes.py [--out-dir DIR]   ->  DIR/ab.jsonl (one line per series and repeat), DIR/ab.txt"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import neorl_industrial_gym_amd as ni
from bench import ClockProbe, dpm_sample, gpu_sysfs_dir

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=65536)
ap.add_argument("--steps", type=int, default=250)
ap.add_argument("--chunk", type=int, default=250)
ap.add_argument("--launches", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--episodes-per-lane", type=int, default=16)
ap.add_argument("--envs", default="RobotAssembly-v0,ChemicalReactor-v0")
ap.add_argument("--out-dir", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "episodes"))
args = ap.parse_args()
B, P, N = args.batch, args.steps, args.launches
os.makedirs(args.out_dir, exist_ok=True)
L = ni._lib
rows = []
sysfs = gpu_sysfs_dir(torch, 0)


def record(row, probe):
    row.update(clock=probe.read(), dpm=dpm_sample(sysfs))
    rows.append(row)
    print(json.dumps(row), flush=True)


def torch_reduction(fl, rew, epcount, acc, ret, hist, K):
    """the body of uniform_action_statistics' loop, as it stands there"""
    f = fl[:, :B]
    done = (f & (L.FLAG_TERMINATED | L.FLAG_TRUNCATED)) != 0
    cum = done.cumsum(0, dtype=torch.int32)
    valid = (epcount.unsqueeze(0) + cum - done.to(torch.int32)) < K
    acc["steps"] += valid.sum()
    acc["viol"] += ((((f >> L.FLAG_NVIOL_SHIFT) & 3) + ((f >> 13) & 1) * 4) * valid).sum()
    acc["crit"] += (((f >> L.FLAG_NCRIT_SHIFT) & 3) * valid).sum()
    for k in range(3):
        acc[f"c{k}"] += (((f >> (L.FLAG_VIOL_SHIFT + k)) & 1) * valid).sum()
    ret += (rew[:, :B].to(torch.float64) * valid).sum()
    dv = done & valid
    acc["episodes"] += dv.sum()
    acc["term"] += (dv & ((f & L.FLAG_TERMINATED) != 0)).sum()
    acc["trunc"] += (dv & ((f & L.FLAG_TRUNCATED) != 0)).sum()
    acc["shut"] += (dv & ((f & L.FLAG_SHUTDOWN) != 0)).sum()
    hist += torch.bincount(((f >> L.FLAG_STEP_SHIFT) & 0xFFFF)[dv].to(torch.int64), minlength=hist.numel())[:hist.numel()]
    epcount += cum[-1]


# ---- 1. the collect kernel against the torch reduction, same rows ----------------------------------------------------------------
for name in args.envs.split(","):
    env = ni.make_batched(name, B, autoreset=True)
    env.reset()
    rew = torch.empty(P, env.ld, dtype=torch.float32, device=env.device)
    fl = torch.empty(P, env.ld, dtype=torch.int32, device=env.device)
    env.rollout_sampled(P, rew, fl)
    K = 1 << 20                                            # every step stays "valid": the reduction's cost does not depend on it
    log = env.episode_log(8)
    epcount = torch.zeros(B, dtype=torch.int32, device=env.device)
    acc = {k: torch.zeros((), dtype=torch.int64, device=env.device) for k in ("steps", "viol", "crit", "c0", "c1", "c2", "episodes", "term", "trunc", "shut")}
    ret = torch.zeros((), dtype=torch.float64, device=env.device)
    hist = torch.zeros(env.max_episode_steps + 1, dtype=torch.int64, device=env.device)
    series = {"collect_kernel": lambda: env.collect_episodes(log, P, rew, fl),
              "torch_reduction": lambda: torch_reduction(fl, rew, epcount, acc, ret, hist, K)}
    for rep in range(args.repeats):
        for sname, call in series.items():
            probe = ClockProbe(ni, torch, env.device)
            for _ in range(args.warmup):
                call()
            torch.cuda.synchronize()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(N)]
            probe.stamp(0)
            for a, b in ev:
                a.record(); call(); b.record()
            probe.stamp(1)
            torch.cuda.synchronize()
            us = np.array([a.elapsed_time(b) for a, b in ev]) * 1e3
            record({"measurement": "collect", "env": name, "series": sname, "repeat": rep, "batch": B, "rows": P, "calls": N,
                    "us_per_call_median": float(np.median(us)), "us_per_call_min": float(us.min()), "us_per_call_max": float(us.max()),
                    "row_bytes": 8 * P * B}, probe)
    env.close()

# ---- 2. evaluate_episodes (quota) against evaluate_with_safety (rounds) ------------------------------------------------------------
n_episodes = B * args.episodes_per_lane


def quota(name):
    env = ni.make_batched(name, B, autoreset=True)
    return env, lambda: ni.evaluate_episodes(ni.mpc_agent(env.state_dim, env.action_dim), env, n_episodes, chunk=args.chunk)


def rounds(name):
    env = ni.make_batched(name, B, autoreset=False, tally=True)
    return env, lambda: ni.evaluate_with_safety(ni.mpc_agent(env.state_dim, env.action_dim), env, n_episodes)


def evaluate(make, name):
    """a fresh handle (made outside the clock), then the whole evaluation call, ending in a device synchronise"""
    env, call = make(name)
    probe = ClockProbe(ni, torch, env.device)
    torch.cuda.synchronize()
    probe.stamp(0)
    t0 = time.perf_counter()
    m = call()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    probe.stamp(1)
    torch.cuda.synchronize()
    env.close()
    return m, dt, probe


for name in args.envs.split(","):
    for make in (quota, rounds):                           # warm-up: code objects, allocator
        evaluate(make, name)
    for rep in range(args.repeats):
        for sname, make in (("evaluate_episodes_quota", quota), ("evaluate_with_safety_rounds", rounds)):
            m, dt, probe = evaluate(make, name)
            record({"measurement": "evaluate", "env": name, "series": sname, "repeat": rep, "batch": B, "n_episodes": n_episodes,
                    "seconds": dt, "return_mean": float(m["return_mean"]), "length_mean": float(m["length_mean"]),
                    "launches": m.get("launches")}, probe)

with open(os.path.join(args.out_dir, "ab.jsonl"), "w") as f:
    for r in rows:
        f.write(json.dumps(r) + "\n")
lines = [f"{torch.cuda.get_device_name(0)}; {ni._lib.lib().nig_version().decode()}; batch {B}", ""]
for name in args.envs.split(","):
    lines.append(name)
    for meas, key, unit, a, b in (("collect", "us_per_call_median", "us per call", "collect_kernel", "torch_reduction"),
                                  ("evaluate", "seconds", "s per call", "evaluate_episodes_quota", "evaluate_with_safety_rounds")):
        med = {}
        for s in (a, b):
            mine = [r for r in rows if r["env"] == name and r["measurement"] == meas and r["series"] == s]
            x = [r[key] for r in mine]
            med[s] = float(np.median(x))
            clk = np.median([r["clock"].get("shader_clock_mhz", float("nan")) for r in mine])
            dpm = mine[-1]["dpm"]
            lines.append(f"  {s:30s} {', '.join(f'{v:10.4g}' for v in x)} {unit}   spread {100 * (max(x) - min(x)) / min(x):5.1f} %   "
                         f"{clk:.0f} MHz shader clock; sclk {dpm.get('sclk_mhz')} mclk {dpm.get('mclk_mhz')} MHz, {dpm.get('power_w')} W")
        lines.append(f"  {a} / {b}: {med[a] / med[b]:.3f} (medians of the repeats)")
    lines.append("")
open(os.path.join(args.out_dir, "ab.txt"), "w").write("\n".join(lines))
print("\n".join(lines))
