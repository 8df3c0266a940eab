#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY (never collected) -- golden vectors for the added box constraints ("nig-limits-v1", include/nig.h
nig_set_limits), made by RUNNING the reference where it exists:  python tests/gen_limits_golden.py

For each NumPy env the reference env gets four added constraints, SafetyConstraint(check_fn=<the box law>), and teacher-forced
single steps are recorded in the StepLog shape of oracle/gen_golden.py's G1 (pre-state, action, draws, next state, reward,
terminated, truncated, violation_count, critical_violations, per-constraint bits -- here seven: the built-ins, then the added
ones -- and reward_raw, the reference's _compute_reward of the same transition, i.e. the reward before any penalty).  Output: tests/golden/limits_{cr,pg,ra}.npz, data only.

  set 1: four non-critical constraints -- a state row with an upper bound, an action row with a band, a multi-row box over a
         state row and an action row, a state row with a lower bound;
  set 2: two non-critical (a state row, an action row) and two critical (a state row, an action row).
Bounds are quantiles of the reference's own UNCONSTRAINED rollout under the same action mixture.

Per set: `s<k>_*` a rollout under uniform and over-range actions plus forced corner tuples (pool states pushed over a built-in
critical limit; for ChemicalReactor uniform rollouts never reach one), `s<k>_a64_*` the first tuples again with genuine float64
actions (the G6 construction).  `eval_*`: the reference's evaluate_with_safety dict for gen_golden's stub agent under set 2,
with every draw (the G4 layout).  The assertions at the end are on the reference alone."""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from oracle import gen_golden as G  # noqa: E402
from oracle.ref_import import NoiseTap, load_reference  # noqa: E402

f32 = np.float32
OUT = os.path.join(ROOT, "tests", "golden")
ROWS = 48                 # NIG_LIMIT_ROWS
N_ROLL, N_FORCED, N_A64 = 600, 96, 150
KR = {"cr": 8, "pg": 31, "ra": 7}
# state rows the sets bound (rows that vary under a uniform rollout) and how a pool state is pushed over a built-in critical limit
STATE_ROWS = {"cr": (0, 10, 2, 4), "pg": (0, 9, 17, 25), "ra": (0, 2, 7, 8)}
PUSH = {"cr": lambda s, rng: s.__setitem__(0, f32(rng.uniform(350.5, 356))) if rng.random() < 0.5 else s.__setitem__(1, f32(rng.uniform(507000, 520000))),
        "pg": lambda s, rng: s.__setitem__(0, f32(rng.choice([-1, 1]) * rng.uniform(0.55, 0.9))),
        "ra": lambda s, rng: s.__setitem__(18, f32(rng.choice([-1, 1]) * rng.uniform(55, 90)))}


def box_holds(mask, lo, hi, S):
    """The box law as a check_fn: every listed row x has lo <= x and x <= hi (float32 bounds; NumPy widens them for a
    float64 action element)."""
    rows = [r for r in range(ROWS) if (mask >> r) & 1]

    def check(state, action):
        for r in rows:
            x = state[r] if r < S else action[r - S]
            if not (lo[r] <= x and x <= hi[r]):
                return False
        return True
    return check


def make_sets(pool_s, pool_a, pool_t, key):
    """The two constraint sets from the unconstrained pool's quantiles: (mask, lo, hi, penalty, critical) x 4 each.  Set 2's
    critical constraints end an episode within a few steps, so its bounds are quantiles of the pool's first three episode steps."""
    S, A = pool_s.shape[1], pool_a.shape[1]
    r0, r1, r2, r3 = STATE_ROWS[key]
    q = lambda x, p: f32(np.quantile(x.astype(np.float64), p))
    inf = f32(np.inf)

    def one(rows, penalty, critical):
        mask, lo, hi = 0, np.zeros(ROWS, f32), np.zeros(ROWS, f32)
        for r, (a, b) in rows.items():
            mask |= 1 << r
            lo[r], hi[r] = a, b
        return (mask, lo, hi, float(penalty), int(critical))

    s, a = pool_s, pool_a
    set1 = [one({r0: (-inf, q(s[:, r0], 0.65))}, -7.5, 0),
            one({S + 0: (q(a[:, 0], 0.2), q(a[:, 0], 0.8))}, -3.0, 0),
            one({r1: (q(s[:, r1], 0.12), q(s[:, r1], 0.88)), S + 1: (q(a[:, 1], 0.1), q(a[:, 1], 0.9))}, -12.25, 0),
            one({r2: (q(s[:, r2], 0.3), inf)}, -0.1, 0)]
    s, a = pool_s[pool_t <= 2], pool_a[pool_t <= 2]
    set2 = [one({r0: (-inf, q(s[:, r0], 0.6))}, -5.0, 0),
            one({S + A - 1: (q(a[:, A - 1], 0.25), q(a[:, A - 1], 0.75))}, -2.5, 0),
            one({r3: (q(s[:, r3], 0.1), q(s[:, r3], 0.9))}, -40.0, 1),
            one({S + 1: (q(a[:, 1], 0.15), q(a[:, 1], 0.85))}, -60.0, 1)]
    return [set1, set2]


def add_set(utils, env, cset):
    SC = type(env.safety_constraints[0])             # the reference's own SafetyConstraint
    for c, (mask, lo, hi, pen, crit) in enumerate(cset):
        env.add_safety_constraint(SC(name=f"added_{c}", check_fn=box_holds(mask, lo, hi, env.state_dim), penalty=pen, critical=bool(crit)))
    return env


class Log:
    KEYS = ("state_pre", "action", "noise", "step_pre", "viol_pre", "state_next", "reward", "terminated", "truncated", "viol",
            "crit", "viol_bits", "violations_after", "reward_raw")

    def __init__(self):
        self.rows = {k: [] for k in self.KEYS}
        self.action64 = []

    def arrays(self, prefix, S, A, K):
        r, n = self.rows, len(self.rows["reward"])
        out = {"state_pre": np.asarray(r["state_pre"], f32).reshape(n, S), "action": np.asarray(r["action"], f32).reshape(n, A),
               "noise": np.asarray(r["noise"], np.float64).reshape(n, K), "step_pre": np.asarray(r["step_pre"], np.int32),
               "viol_pre": np.asarray(r["viol_pre"], np.int32), "state_next": np.asarray(r["state_next"], f32).reshape(n, S),
               "reward": np.asarray(r["reward"], np.float64), "terminated": np.asarray(r["terminated"], np.uint8),
               "truncated": np.asarray(r["truncated"], np.uint8), "viol": np.asarray(r["viol"], np.int32),
               "crit": np.asarray(r["crit"], np.int32), "viol_bits": np.asarray(r["viol_bits"], np.uint8).reshape(n, 7),
               "violations_after": np.asarray(r["violations_after"], np.int32),
               "reward_raw": np.asarray(r["reward_raw"], np.float64)}
        if self.action64:
            out["action64"] = np.asarray(self.action64, np.float64).reshape(n, A)
        return {prefix + k: v for k, v in out.items()}


def step_rec(env, tap, action, log, K):
    """One reference env.step() with recording; `action` float32, or float64 (then also kept as given)."""
    state_pre = env.state.copy()
    step_pre, viol_pre = env.current_step, env.violation_count
    a_clip = np.clip(action, env.action_space.low, env.action_space.high)
    vbits = [0 if bool(c.check_fn(state_pre, a_clip)) else 1 for c in env.safety_constraints]
    tap.take()
    obs, reward, term, trunc, info = env.step(action)
    noise = tap.take()
    assert noise.size == K
    raw = env._compute_reward(state_pre, a_clip, obs)      # base.py:176: the reward before any penalty, from the reference's own hook
    tap.take()
    sm = info["safety_metrics"]
    assert len(vbits) == 7 and sm.total_constraints == 7 and sm.violation_count == sum(vbits)
    assert sm.critical_violations == sum(b for b, c in zip(vbits, env.safety_constraints) if c.critical)
    if action.dtype == np.float64:
        log.action64.append(action.copy())
    for k, v in (("state_pre", state_pre), ("action", action.astype(f32)), ("noise", noise), ("step_pre", step_pre),
                 ("viol_pre", viol_pre), ("state_next", obs.copy()), ("reward", float(reward)), ("terminated", int(bool(term))),
                 ("truncated", int(bool(trunc))), ("viol", sm.violation_count), ("crit", sm.critical_violations),
                 ("viol_bits", vbits), ("violations_after", info["violations"]), ("reward_raw", float(raw))):
        log.rows[k].append(v)
    return obs, term or trunc


def actions(rng, A):
    return (rng.uniform(-1, 1, A) if rng.random() < 0.7 else rng.uniform(-2.5, 2.5, A)).astype(f32)


def unconstrained_pool(utils, key, seed, n=2500):
    env = utils.make(G.ENVS[key])
    rng = np.random.Generator(np.random.PCG64(seed))
    S, A = env.state_dim, env.action_dim
    ps, pa, pt = [], [], []
    with NoiseTap(seed) as tap:
        done = True
        while len(ps) < n:
            if done:
                env.reset()
            a = actions(rng, A)
            ps.append(env.state.copy()); pa.append(np.clip(a, -1, 1)); pt.append(env.current_step)
            _, _, te, tr, _ = env.step(a)
            done = te or tr
        tap.take()
    return np.asarray(ps, f32), np.asarray(pa, f32), np.asarray(pt)


def record_set(utils, key, cset, pool_s, seed):
    env = add_set(utils, utils.make(G.ENVS[key]), cset)
    S, A = env.state_dim, env.action_dim
    rng = np.random.Generator(np.random.PCG64(seed))
    log, log64 = Log(), Log()
    with NoiseTap(seed) as tap:
        env.reset(); tap.take()
        env.step(np.zeros(A, f32)); K = tap.take().size
        done = True
        for _ in range(N_ROLL):                      # the constrained rollout: episodes end by their own causes, added critical ones included
            if done:
                env.reset(); tap.take()
            _, done = step_rec(env, tap, actions(rng, A), log, K)
        for i in range(N_FORCED):                    # a built-in critical violation forced onto pool states, any episode step
            s = pool_s[rng.integers(len(pool_s))].copy()
            PUSH[key](s, rng)
            G.force(env, s, step=int(rng.integers(0, 400)), viol=int(rng.integers(0, 40)))
            step_rec(env, tap, actions(rng, A), log, K)
        r = log.rows
        for i in range(N_A64):                       # genuine float64 actions on recorded states with their recorded draws
            j = (i * 5) % len(r["reward"])
            G.force(env, r["state_pre"][j], r["step_pre"][j], r["viol_pre"][j])
            tap.forced = list(np.asarray(r["noise"][j], np.float64).ravel())
            a64 = r["action"][j].astype(np.float64) * (1.3 if i % 3 == 0 else 0.9) + rng.normal(0.0, 1e-3, A)
            step_rec(env, tap, a64, log64, K)
            tap.forced = None
    return log, log64, S, A, K


def record_eval(utils, key, cset, seed):
    proxy = types.SimpleNamespace(make=lambda name: add_set(utils, utils.make(name), cset), evaluate_with_safety=utils.evaluate_with_safety)
    K = {"cr": 2, "pg": 23, "ra": 0}[key]
    return G.record_rollouts(proxy, key, 20, seed, None, KR[key], K, use_eval=True)


def main():
    utils = load_reference()
    for key in G.ENVS:
        pool_s, pool_a, pool_t = unconstrained_pool(utils, key, 7100 + ord(key[0]))
        sets = make_sets(pool_s, pool_a, pool_t, key)
        out = {}
        for k, cset in enumerate(sets, start=1):
            log, log64, S, A, K = record_set(utils, key, cset, pool_s, 7200 + 10 * k + ord(key[0]))
            p = f"s{k}_"
            out.update(log.arrays(p, S, A, K)); out.update(log64.arrays(p + "a64_", S, A, K))
            out[p + "mask"] = np.asarray([c[0] for c in cset], np.uint64)
            out[p + "lo"] = np.stack([c[1] for c in cset]); out[p + "hi"] = np.stack([c[2] for c in cset])
            out[p + "penalty"] = np.asarray([c[3] for c in cset], np.float64)
            out[p + "critical"] = np.asarray([c[4] for c in cset], np.uint8)
            # ---- what the fixture must contain, asserted on the reference alone
            vb, n = out[p + "viol_bits"], len(out[p + "reward"])
            rate = vb[:N_ROLL, 3:].mean(axis=0)
            assert ((rate >= 0.1) & (rate <= 0.9)).all(), (key, k, rate)
            base_crit = np.asarray([c.critical for c in utils.make(G.ENVS[key]).safety_constraints], bool)
            builtin_crit = (vb[:, :3] * base_crit).sum(axis=1) > 0
            both = builtin_crit & (vb[:, 3:].sum(axis=1) > 0)
            assert both.sum() >= 32, (key, k, int(both.sum()))
            crit_added = (vb[:, 3:] * out[p + "critical"]).sum(axis=1) > 0
            alone = crit_added & ~builtin_crit & (out[p + "terminated"] == 1)
            if k == 2:
                assert alone.sum() >= 32, (key, k, int(alone.sum()))
            assert (out[p + "terminated"][builtin_crit | crit_added] == 1).all()
            assert (out[p + "viol"] == vb.sum(axis=1)).all()
            print(key, "set", k, "tuples", n, "a64", len(out[p + "a64_reward"]), "rates", np.round(rate, 3), "built-in critical + added:",
                  int(both.sum()), "ended by an added critical alone:", int(alone.sum()))
        ev = record_eval(utils, key, sets[1], 7400 + ord(key[0]))
        out.update({"eval_" + k: v for k, v in ev.items()})
        print(key, "eval", bytes(ev["result_json"]).decode())
        path = os.path.join(OUT, f"limits_{key}.npz")
        np.savez_compressed(path, **out)
        assert os.path.getsize(path) < 1_000_000, os.path.getsize(path)
        print(key, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
