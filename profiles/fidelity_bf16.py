#!/usr/bin/env python3
"""How far the bf16 actor ("nig-mlp-bf16-v1") is from the float32 actor, for the reader who has to decide whether to trust a
sweep (GPU box).  Nothing is asserted.  Per env (ChemicalReactor, PowerGrid, RobotAssembly), weights
tests/closed_loop_matrix.random_actor:
  * |a_bf16 - a_f32| on the SAME observation rows: the float32 loop's obs_out rows of --steps steps at --batch lanes are set as
    the state of a second handle, which takes one bf16 step on them; maximum and quantiles over all lanes, steps and action rows;
  * evaluate_with_safety's dict from both actors, --episodes episodes each, side by side.

usage: python profiles/fidelity_bf16.py [--out-dir DIR]   ->  DIR/fidelity.txt"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import neorl_industrial_gym_amd as ni
from closed_loop_matrix import random_actor

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--steps", type=int, default=8)
ap.add_argument("--episodes", type=int, default=4096)
ap.add_argument("--envs", default="ChemicalReactor-v0,PowerGrid-v0,RobotAssembly-v0")
ap.add_argument("--out-dir", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "bf16"))
args = ap.parse_args()
B, T = args.batch, args.steps
os.makedirs(args.out_dir, exist_ok=True)
lines = [f"{torch.cuda.get_device_name(0)}; {ni._lib.lib().nig_version().decode()}",
         f"weights: closed_loop_matrix.random_actor(S, A, 21); action differences over {B} lanes x {T} steps; {args.episodes} episodes per actor", ""]
for name in args.envs.split(","):
    a = ni.make_batched(name, B, autoreset=True, seed=0x5EED)
    b = ni.make_batched(name, B, autoreset=True, seed=0x5EED)
    S, A, dev = a.state_dim, a.action_dim, a.device
    ws = random_actor(S, A, 21)
    a.set_mlp_policy(ws)
    b.set_mlp_policy_bf16(ws)
    a.reset()
    obs = torch.zeros(T, B, S, dtype=torch.float32, device=dev)
    act = torch.zeros(T, A, a.ld, dtype=torch.float32, device=dev)
    a.rollout_mlp(T, None, None, obs, act)
    act16 = torch.zeros(1, A, b.ld, dtype=torch.float32, device=dev)
    b.reset()
    diffs = []
    for k in range(T):
        b.set_state(obs[k], current_step=0, violation_count=0, done=False)
        b.rollout_mlp_bf16(1, None, None, None, act16)
        diffs.append((act16[0, :, :B] - act[k, :, :B]).abs().double().flatten().cpu().numpy())
    torch.cuda.synchronize()
    d = np.concatenate(diffs)
    qs = [0.5, 0.9, 0.99, 0.999]
    lines.append(f"{name}: |a_bf16 - a_f32| on the same observation rows ({d.size} values, |a| <= 1; mean |a_f32| {float(act[:, :, :B].abs().mean()):.3f})")
    lines.append("  max %.3e   " % d.max() + "   ".join(f"q{q:g} {np.quantile(d, q):.3e}" for q in qs))
    a.close(); b.close()
    pol = ni.MLPPolicy(ws)
    res = {}
    for arm, p in (("f32", pol), ("bf16", pol.bf16())):
        env = ni.make_batched(name, min(B, args.episodes), tally=True, autoreset=False, seed=0x5EED)
        res[arm] = ni.evaluate_with_safety(p, env, n_episodes=args.episodes)
        env.close()
    lines.append(f"  evaluate_with_safety, {args.episodes} episodes:   {'f32':>16s} {'bf16':>16s}")
    for k in res["f32"]:
        lines.append(f"    {k:34s} {float(res['f32'][k]):16.6g} {float(res['bf16'][k]):16.6g}")
    lines.append("")
open(os.path.join(args.out_dir, "fidelity.txt"), "w").write("\n".join(lines))
print("\n".join(lines))
