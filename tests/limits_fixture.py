"""The added-box-constraint fixtures (tests/golden/limits_<key>.npz, made by tests/gen_limits_golden.py from the reference) and
the law they pin, restated in NumPy.  A plain helper module (no fixtures, no collection hooks) shared by test_limits_host.py
and test_gpu_limits.py."""
import os

import numpy as np

from conftest import GOLDEN

f32 = np.float32
_CACHE = {}


def load(key):
    if key not in _CACHE:
        d = dict(np.load(os.path.join(GOLDEN, f"limits_{key}.npz")))
        for v in d.values():
            v.setflags(write=False)
        _CACHE[key] = d
    return _CACHE[key]


def tuples(d, prefix):
    """The tuple arrays stored under `prefix` ("s1_", "s2_a64_", ...) without it."""
    names = ("state_pre", "action", "noise", "step_pre", "viol_pre", "state_next", "reward", "terminated", "truncated", "viol",
             "crit", "viol_bits", "violations_after", "reward_raw", "action64")
    return {n: d[prefix + n] for n in names if prefix + n in d}


def boxes(ni, d, k, S, A):
    """Constraint set k of the fixture as ni.BoxConstraint objects, in installation order."""
    out = []
    for c in range(4):
        mask = int(d[f"s{k}_mask"][c])
        bounds = {}
        for r in range(S + A):
            if (mask >> r) & 1:
                bounds[("state", r) if r < S else ("action", r - S)] = (d[f"s{k}_lo"][c][r], d[f"s{k}_hi"][c][r])
        out.append(ni.BoxConstraint(f"added_{c}", bounds, float(d[f"s{k}_penalty"][c]), bool(d[f"s{k}_critical"][c])))
    return out


def reward_law(raw, builtin_bits, builtin_penalty, builtin_critical, added_bits, added_penalty, added_critical, rtype):
    """include/nig.h "nig-limits-v1": r = raw; r = R(r + R(penalty)) for each violated built-in, then for each violated added
    constraint in installation order; then r - 1000 once if any critical constraint of either kind was violated.  Arrays over
    tuples; rtype np.float32 or np.float64.  Returns the rewards as float64."""
    r = np.asarray(raw, dtype=np.float64).astype(rtype)
    for k in range(3):
        r = np.where(builtin_bits[:, k] != 0, (r + rtype(builtin_penalty[k])).astype(rtype), r)
    for c in range(added_bits.shape[1]):
        r = np.where(added_bits[:, c] != 0, (r + rtype(added_penalty[c])).astype(rtype), r)
    crit = (builtin_bits[:, :3] * np.asarray(builtin_critical)[None, :3]).sum(axis=1) + (added_bits * np.asarray(added_critical)[None, :]).sum(axis=1)
    r = np.where(crit > 0, (r - rtype(1000)).astype(rtype), r)
    return r.astype(np.float64), crit
