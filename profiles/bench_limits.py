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

usage: python profiles/bench_limits.py [--out-dir DIR]   ->  DIR/ab.jsonl (one line per series), DIR/ab.txt (the table)

--families: the _limited twins of the other closed-loop families instead, each against its OWN parent family in the same session
(DIR/ab_families.jsonl, DIR/ab_families.txt), the plain pair mlp / mlp_limited beside them:
  safe, search (3 candidates), gated (2 members of 2 rows), projected (3 iterations), ensemble ("voting", 3 members),
  disturbed (sigma 0.1 on observation and action, hold "step"), policy_disturbed (the "MPC" law; one-wave form in both)
  and <family>_limited_1 / _limited_4.  Thresholds of 0.5 / an uncertainty limit of 0.2 on random critics: some lanes of nearly
  every block take the correction, so the block-voted passes of the search and the projection run in parent and twin alike (the
  boxes are not critical: the twin plays the parent's trajectory).
Expectation, written before the first measurement: the added constraints are checked once per STEP, whatever the number of network
passes of the step, so a twin's absolute overhead per step should equal the plain form's (mlp_limited - mlp) of the same session,
and its relative overhead should be smaller than the plain form's 1.01 - 1.05 x.  A twin whose absolute overhead is more than twice
the plain form's is a finding to explain from its listing."""
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
ap.add_argument("--families", action="store_true", help="time the _limited twins of the other families against their parents")
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


def critic(S, A, seed, n_out=1):
    rng, D = np.random.default_rng(seed), S + A
    return [(rng.normal(0, 0.02 / np.sqrt(D), (D, 256)).astype(np.float32), np.zeros(256, np.float32)),
            (rng.normal(0, 1 / 16, (256, 256)).astype(np.float32), np.zeros(256, np.float32)),
            (rng.normal(0, 1 / 16, (256, n_out)).astype(np.float32), np.zeros(n_out, np.float32))]


def run_families():
    """Every family's parent and its _limited twin with one and four boxes, alternating through the repeats."""
    FAMILIES = ("mlp", "safe", "search", "gated", "projected", "ensemble", "disturbed", "policy_disturbed")
    for name in args.envs.split(","):
        env = ni.make_batched(name, B, autoreset=True, tally=True)
        S, A = env.state_dim, env.action_dim
        env.set_mlp_policy(actor(S, A, 10))
        env.set_policy(ni.mpc_agent(S, A))
        env.set_mlp_safety(critic(S, A, 11), 0.5)
        env.set_mlp_safety_ensemble([critic(S, A, 12, 2), critic(S, A, 13, 2)], 1.0, 0.5, 0.2)
        env.set_mlp_constraint(critic(S, A, 14, 2), 0.5, 0.0)
        env.set_mlp_ensemble([actor(S, A, 10 + k) for k in range(3)], None, None, "voting", 0.2)
        env.set_disturbance(ni.Disturbance(obs_noise=0.1, action_noise=0.1, hold="step"))
        env.reset()
        state = env.get_state().cpu().numpy()
        boxes = []
        for c in range(4):      # the boxes of the plain series
            lo, hi = np.quantile(state[:, c].astype(np.float64), [0.02, 0.98])
            boxes.append(ni.BoxConstraint(f"box_{c}", {("state", c): (lo, max(hi, lo)), ("action", c % A): (-0.9, 0.9)}, -1.0))
        call = {
            "mlp": lambda sfx: getattr(env, "rollout_mlp" + sfx)(T),
            "safe": lambda sfx: getattr(env, "rollout_mlp_safe" + sfx)(T),
            "search": lambda sfx: getattr(env, "rollout_mlp_search" + sfx)(T, 3),
            "gated": lambda sfx: getattr(env, "rollout_mlp_gated" + sfx)(T),
            "projected": lambda sfx: getattr(env, "rollout_mlp_projected" + sfx)(T, 3, 0.1),
            "ensemble": lambda sfx: getattr(env, "rollout_mlp_ensemble" + sfx)(T),
            "disturbed": lambda sfx: getattr(env, "rollout_mlp_disturbed" + sfx)(T),
            "policy_disturbed": lambda sfx: getattr(env, "rollout_policy_disturbed" + sfx)(T),
        }

        def install(n):
            for b in list(env.safety_constraints):
                if isinstance(b, ni.BoxConstraint):
                    env.remove_safety_constraint(b.name)
            for b in boxes[:n]:
                env.add_safety_constraint(b)

        for rep in range(args.repeats):
            for fam in FAMILIES:
                NL = args.policy_launches if fam == "policy_disturbed" else N
                install(0)
                timed(env, name, fam, lambda: call[fam](""), rep, NL)
                for n in (1, 4):
                    install(n)
                    timed(env, name, f"{fam}_limited_{n}", lambda: call[fam]("_limited"), rep, NL)
        env.close()
    with open(os.path.join(args.out_dir, "ab_families.jsonl"), "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    lines = [f"batch {B}, {T} steps per launch, {N} timed launches ({args.policy_launches} for policy_disturbed) after {args.warmup}, {args.repeats} alternating "
             "repeats; microseconds per step, median of the launches, per repeat; overhead = twin - its own parent (medians of the repeats)",
             f"{torch.cuda.get_device_name(0)}; {ni._lib.lib().nig_version().decode()}", ""]
    for name in args.envs.split(","):
        med = {}
        for r in rows:
            if r["env"] == name:
                med.setdefault(r["series"], []).append(r["us_per_step_median"])
        lines.append(name)
        plain = {n: np.median(med[f"mlp_limited_{n}"]) - np.median(med["mlp"]) for n in (1, 4)}
        for fam in FAMILIES:
            for series in (fam, f"{fam}_limited_1", f"{fam}_limited_4"):
                x = med[series]
                txt = f"  {series:28s} {', '.join(f'{v:8.2f}' for v in x)} us   spread {100 * (max(x) - min(x)) / min(x):5.2f} %"
                if series != fam:
                    n = int(series[-1])
                    over = np.median(x) - np.median(med[fam])
                    txt += f"   / {fam}: {np.median(x) / np.median(med[fam]):.3f}   overhead {over:+7.2f} us"
                    if fam not in ("mlp", "policy_disturbed"):
                        txt += f" = {over / plain[n]:5.2f} x the plain form's {plain[n]:+.2f} us" if plain[n] > 0 else f" (the plain form's: {plain[n]:+.2f} us)"
                lines.append(txt)
        lines.append("")
    open(os.path.join(args.out_dir, "ab_families.txt"), "w").write("\n".join(lines))
    print("\n".join(lines))


if args.families:
    run_families()
    sys.exit(0)

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
