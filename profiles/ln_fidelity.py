#!/usr/bin/env python3
"""How far the law "nig-mlp-ln-v1" is from its formula in float64, and the bound it is held to (no GPU needed).

The cases of tests/test_mlp_ln_host.py (tests/mlp_ln_ref.py: the host restatement of the law, the float64 model, the derived
forward-error bound of the head pre-activations), and beside them -- without a bar -- an actor whose first bias is shifted by 50,
where flax's one-pass variance E[z^2] - E[z]^2 in float32 loses the layer and the law's two-pass variance does not.
usage: python profiles/ln_fidelity.py   ->  profiles/ln/fidelity.txt"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
import numpy as np

import mlp_ln_ref as ref

lines = ["head pre-activations of the law (tests/mlp_ln_ref.c) against the formula in NumPy float64, 4096 observations per case;",
         "bound: tests/mlp_ln_ref.py pre_bound (gamma_n of every fma chain, propagated through 1 / sigma); actions: |tanh(pre) - tanh(pre64)|",
         "",
         f"{'case':32s} {'max |err|':>11s} {'max bound':>11s} {'max err/bound':>14s} {'max action err':>15s}"]
for label, S, A, ws, norms, obs in ref.fidelity_cases():
    m = ref.model64(ws, norms, obs)
    pre = ref.pre(ws, norms, obs).astype(np.float64)
    err, bound = np.abs(pre - m["pre"]), ref.pre_bound(m, S)
    lines.append(f"{label:32s} {err.max():11.3g} {bound.max():11.3g} {np.max(err / bound):14.3g} {np.abs(np.tanh(pre) - m['action']).max():15.3g}")
S, A, ws, norms, obs = ref.shifted_bias_case()
m = ref.model64(ws, norms, obs)
two = np.abs(ref.pre(ws, norms, obs).astype(np.float64) - m["pre"])
one = np.abs(ref.one_pass_f32(ws, norms, obs).astype(np.float64) - m["pre"])
plain_ws = [(ws[0][0], (ws[0][1] - np.float32(50)).astype(np.float32)), ws[1], ws[2]]
plain = np.abs(ref.one_pass_f32(plain_ws, norms, obs).astype(np.float64) - ref.model64(plain_ws, norms, obs)["pre"])
lines += ["",
          f"first bias shifted by 50 (S={S} A={A}, obs~N(0,1)); no bar, shown for the choice of the two-pass variance:",
          f"  the law (two-pass variance)                  max |err| {two.max():.3g}   (bound {ref.pre_bound(m, S).max():.3g})",
          f"  one-pass E[z^2] - E[z]^2 in float32 NumPy    max |err| {one.max():.3g}",
          f"  the same one-pass form without the shift     max |err| {plain.max():.3g}"]
os.makedirs(os.path.join(HERE, "ln"), exist_ok=True)
open(os.path.join(HERE, "ln", "fidelity.txt"), "w").write("\n".join(lines) + "\n")
print("\n".join(lines))
