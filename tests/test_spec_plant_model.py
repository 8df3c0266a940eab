"""The CPU statement of the four build-specified plants against the float64 model of their written spec.

tests/spec_plant_model.py evaluates the docstring model of spec_plants.py from its dicts, by name, in float64, and
derives the float32 forward-error bound that serves as the tolerance.  Here the oracle's float32 statement (both math
flavours) is held against it on dense rows, on exact one-ulp threshold rows, on edge and special values, in its
structure (which input moves which row, by how much) and in its reset; and the comparison itself is shown to be sharp:
deliberately wrong models fail it.  The kernels meet the same model in test_gpu_spec_plant_model.py.
"""
import numpy as np
import pytest

import spec_plant_model as M

FLAVORS = [0, 1]          # oracle.MATH_LIBM, oracle.MATH_POLY


def _got(oracle, P, st, act, nz, step_pre, flavor=0, max_steps=None, dt=None):
    r = oracle.step(P["name"], st, act, nz, step_pre, max_steps=max_steps, dt=dt, flavor=flavor)
    return dict(state_next=r["state_next"], reward=r["reward"], bits=r["bits"] == 0, viol=r["viol"], crit=r["crit"],
                terminated=r["terminated"] != 0, truncated=r["truncated"] != 0, shutdown=r["shutdown"] != 0)


@pytest.mark.parametrize("flavor", FLAVORS)
@pytest.mark.parametrize("key", M.KEYS)
def test_dense_rows_within_the_derived_bound(oracle, key, flavor):
    """40 000 mixed rows per plant, step_pre over 0 .. max_steps + 1: continuous outputs within the bound, pre-state bits,
    counts, shutdown and truncation exactly, next-state decisions under the margin rule."""
    P = M.plant(key)
    st, act, nz, sp = M.dense_rows(P, 40000, seed=1)
    out = M.check(M.step(P, st, act, nz, sp), _got(oracle, P, st, act, nz, sp, flavor), f"{key} dense flavour {flavor}")
    assert out["worst"] < 1.0
    ref = M.step(P, st, act, nz, sp)
    assert ref["bits"].any(axis=0).all() and ref["terminated"].any() and (~ref["terminated"]).any()      # the sample exercises every constraint
    assert ref["truncated"].any() and (~ref["truncated"]).any()


@pytest.mark.parametrize("key", M.KEYS)
@pytest.mark.parametrize("cmask", [0, 1, 2, 5, 6])
def test_constraint_mask_and_time_step(oracle, key, cmask):
    """The CPU statement has no constraint mask of its own: a masked-out constraint that did not fire leaves the step as it
    is, so on those rows the statement must equal the masked model in everything, and on all rows in the next state (the
    dynamics do not see the mask) and in the enabled bits.  (The kernels' own mask is checked on the GPU.)  A non-default
    dt and max_steps go through both."""
    P = M.plant(key)
    st, act, nz, sp = M.dense_rows(P, 6000, seed=2)
    dt, max_steps = 0.05 + 0.05 * (cmask % 3), 37
    sp = sp % 40
    ref = M.step(P, st, act, nz, sp, max_steps=max_steps, dt=dt, cmask=cmask)
    got = _got(oracle, P, st, act, nz, sp, 1, max_steps=max_steps, dt=dt)
    full = M.step(P, st, act, nz, sp, max_steps=max_steps, dt=dt)
    same = ~(full["bits"] & ~ref["bits"]).any(axis=1)
    assert same.any() and (~same).any()
    sel = lambda d, m: {k: (v[m] if isinstance(v, np.ndarray) else v) for k, v in d.items()}
    M.check(sel(ref, same), sel(got, same), f"{key} cmask {cmask} dt {dt:.2f}")
    part = M.compare(ref, dict(state_next=got["state_next"], reward=np.where(same, got["reward"], ref["reward"])))
    assert not part["failures"], part["failures"][:5]
    enabled = np.array([(cmask >> c) & 1 for c in range(3)], dtype=bool)
    assert np.array_equal(got["bits"] & enabled, ref["bits"])


@pytest.mark.parametrize("flavor", FLAVORS)
@pytest.mark.parametrize("key", M.KEYS)
def test_threshold_rows_exact(oracle, key, flavor):
    """Every constraint, every row of its run, both finite bounds: the pre-state value at float32(bound), one ulp below,
    one ulp above.  33 / 15 / 48 / 105 rows; every output under the rules, and no row undecidable."""
    P = M.plant(key)
    st, act, nz, sp = M.threshold_rows(P)
    assert len(st) == {"hvac": 33, "water": 15, "steel": 48, "supply": 105}[key]
    ref = M.step(P, st, act, nz, sp)
    out = M.check(ref, _got(oracle, P, st, act, nz, sp, flavor), f"{key} thresholds flavour {flavor}")
    assert out["undecidable"] == 0
    # at the bound: inside (inclusive); one ulp outside: violated -- each constraint sees both
    for c in range(3):
        assert ref["bits"][:, c].any() and (~ref["bits"][:, c]).any()


@pytest.mark.parametrize("flavor", FLAVORS)
@pytest.mark.parametrize("key", M.KEYS)
def test_edge_and_special_rows(oracle, key, flavor):
    """Saturating actuators, process variables at ymin / ymax, step_pre around max_steps, a critical with a non-critical
    violation, and the special values (+-0, NaN, +-inf, +-1e30, denormals) in process variables and actuator positions."""
    P = M.plant(key)
    st, act, nz, sp = M.edge_rows(P)
    ref = M.step(P, st, act, nz, sp)
    M.check(ref, _got(oracle, P, st, act, nz, sp, flavor), f"{key} edges flavour {flavor}")
    both = (ref["crit"] > 0) & (ref["viol"] > ref["crit"])
    assert both.any() and np.all(ref["reward"][both] < -1000.0)
    assert ref["truncated"].sum() == 2                                   # max_steps - 1 and max_steps, not max_steps - 2
    assert np.all(np.isfinite(ref["state_next"]))                        # a clipped row is never NaN / infinite
    NP, A, S = M.dims(P)
    sat = ref["state_next"][:12, NP:NP + A]                              # positions at 0 / 1 pushed by six action values
    assert np.all((sat >= 0.0) & (sat <= 1.0)) and (sat == 0.0).any() and (sat == 1.0).any()


def _moved(oracle, P, st, act, nz, st2, act2, nz2):
    """(difference of the two next states in float64, summed bounds of the two evaluations, bit-equality per element)"""
    z = np.zeros(len(st), dtype=np.int32)
    a = oracle.step(P["name"], st, act, nz, z, flavor=1)["state_next"]
    b = oracle.step(P["name"], st2, act2, nz2, z, flavor=1)["state_next"]
    tol = M.step(P, st, act, nz, z)["bound_state"] + M.step(P, st2, act2, nz2, z)["bound_state"]
    return b.astype(np.float64) - a.astype(np.float64), tol, a.view(np.uint32) == b.view(np.uint32)


@pytest.mark.parametrize("key", M.KEYS)
def test_structure_one_input_at_a_time(oracle, key):
    """Every non-zero gain, every coupling, both noise rows: perturbing that one input moves exactly the process rows the
    dict names -- by G dp dt / cpl dy dt / dnoise dt within the bound -- and no other process row by a single bit."""
    P = M.plant(key)
    NP, A, S = M.dims(P)
    n = 48
    rng = np.random.default_rng(9)
    st = np.tile(M.operating_point(P), (n, 1))
    st[:, :NP] += (0.5 * np.array([y["sd0"] for y in P["y"]]) * rng.standard_normal((n, NP))).astype(np.float32)
    st[:, NP:NP + A] = rng.uniform(0.3, 0.6, (n, A)).astype(np.float32)
    act = np.zeros((n, A), dtype=np.float32)                             # zero action: p' = p, unclipped
    nz = np.zeros((n, 2))
    dt = float(np.float32(0.1))
    f = lambda x: float(np.float32(x))
    cases = 0
    for j, actu in enumerate(P["act"]):                                  # gains, by actuator NAME
        st2 = st.copy(); st2[:, NP + j] += np.float32(0.125)
        dp = st2[:, NP + j].astype(np.float64) - st[:, NP + j]
        d, tol, same = _moved(oracle, P, st, act, nz, st2, act, nz)
        for i, y in enumerate(P["y"]):
            g = y["gains"].get(actu["name"], 0.0)
            if g != 0.0:
                assert np.all(np.abs(d[:, i] - f(g) * dp * dt) <= tol[:, i]), (key, actu["name"], y["name"])
                assert np.all(d[:, i] != 0.0)
                cases += 1
            else:
                assert same[:, i].all(), (key, actu["name"], y["name"])
    assert cases == sum(1 for y in P["y"] for g in y["gains"].values() if g != 0.0)
    for c in range(NP):                                                  # couplings: who reads y_c
        st2 = st.copy(); st2[:, c] += np.float32(0.5 * P["y"][c]["sd0"])
        dy = st2[:, c].astype(np.float64) - st[:, c]
        d, tol, same = _moved(oracle, P, st, act, nz, st2, act, nz)
        for i, y in enumerate(P["y"]):
            reads = y["cpl"] != 0.0 and y["cidx"] == c and i != c
            if i == c:
                own = 1.0 - (f(y["k"]) + (f(y["cpl"]) if y["cidx"] not in (None, c) else 0.0)) * dt
                assert np.all(np.abs(d[:, i] - own * dy) <= tol[:, i]), (key, y["name"])
            elif reads:
                assert np.all(np.abs(d[:, i] - f(y["cpl"]) * dy * dt) <= tol[:, i]) and np.all(d[:, i] != 0.0), (key, y["name"], c)
            else:
                assert same[:, i].all(), (key, y["name"], c)
    for r in range(2):                                                   # the two noise rows
        nz2 = nz.copy(); nz2[:, r] = float(np.float32(P["noise_sd"][r]))
        d, tol, same = _moved(oracle, P, st, act, nz, st, act, nz2)
        assert np.all(np.abs(d[:, r] - nz2[:, r] * dt) <= tol[:, r])
        assert np.all(d[:, r] != 0.0) and same[:, [i for i in range(NP) if i != r]].all()


@pytest.mark.parametrize("key", M.KEYS)
def test_reset_bit_for_bit(oracle, key):
    P = M.plant(key)
    NP, A, S = M.dims(P)
    z = np.random.default_rng(4).standard_normal((4096, NP)).astype(np.float32) * np.float32(1.7)
    sd0 = np.array([y["sd0"] for y in P["y"]], dtype=np.float32).astype(np.float64)
    want = M.reset(P, z)
    got = oracle.reset(P["name"], sd0 * z.astype(np.float64))
    assert want.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.all(want[:, NP:NP + A] == 0.5) and np.all(want[:, NP + A:] == 0.0)
    # the generator's draws are such products: reset(draws=) and reset(z) agree on them
    draws = np.stack([oracle.gen_reset_noise(P["name"], 0x5EED, i, 3) for i in range(64)])
    zz = (draws / sd0).astype(np.float32)
    assert np.array_equal(sd0 * zz.astype(np.float64), draws)
    assert np.array_equal(M.reset(P, zz).view(np.uint32), M.reset(P, draws=draws).view(np.uint32))
    assert np.array_equal(oracle.reset(P["name"], draws).view(np.uint32), M.reset(P, draws=draws).view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------
# the comparison is sharp: a deliberately wrong model fails it
# ------------------------------------------------------------------------------------------------------------------
def _smallest_gain_negated(P):
    i, nm = min(((i, nm) for i, y in enumerate(P["y"]) for nm, g in y["gains"].items() if g != 0.0),
                key=lambda q: abs(P["y"][q[0]]["gains"][q[1]]))
    P["y"][i]["gains"][nm] = -P["y"][i]["gains"][nm]


def _cidx_moved(P):
    i = [i for i, y in enumerate(P["y"]) if y["cpl"] != 0.0][0]
    P["y"][i]["cidx"] = (P["y"][i]["cidx"] + 1) % len(P["y"])


def _gain_on_the_next_actuator(P):
    i, nm = [(i, nm) for i, y in enumerate(P["y"]) for nm, g in y["gains"].items() if g != 0.0][0]
    names = [a["name"] for a in P["act"]]
    P["y"][i]["gains"][names[(names.index(nm) + 1) % len(names)]] = P["y"][i]["gains"].pop(nm)


def _run_shortened(P):
    c = max(range(3), key=lambda c: P["constraints"][c][2])
    t = P["constraints"][c]
    P["constraints"][c] = t[:2] + (t[2] - 1,) + t[3:]


def _strict_bound(P):
    c, first, count, lo, hi, _, _ = (0,) + tuple(P["constraints"][0][1:])
    return (0, "hi" if abs(hi) < 9e29 else "lo")


MUTATIONS = {
    "smallest gain negated": (_smallest_gain_negated, {}),
    "gain on the next actuator": (_gain_on_the_next_actuator, {}),
    "cidx moved by one": (_cidx_moved, {}),
    "coupling reads the updated neighbour": (None, dict(coupling_new=True)),
    "constraints on the next state": (None, dict(constraints_on_next=True)),
    "bonus on the pre-state": (None, dict(bonus_on_pre=True)),
    "inclusive bound made strict": (None, "strict"),
    "constraint run one row short": (_run_shortened, {}),
}


@pytest.mark.parametrize("mutation", list(MUTATIONS))
@pytest.mark.parametrize("key", M.KEYS)
def test_wrong_models_fail_the_comparison(oracle, key, mutation):
    """The bound is tight enough to notice a subtly wrong kernel: each mutation of the model makes the dense or the
    threshold comparison against the (unchanged) CPU statement fail.  The unmutated model passes the same rows."""
    mutate, kw = MUTATIONS[mutation]
    P, Pm = M.plant(key), M.plant(key, mutate)
    if kw == "strict":
        kw = dict(strict=_strict_bound(P))
    failures = {}
    for label, rows in (("dense", M.dense_rows(P, 4000, seed=3)), ("threshold", M.threshold_rows(P))):
        got = _got(oracle, P, *rows, flavor=1)
        assert not M.compare(M.step(P, *rows), got)["failures"]
        failures[label] = len(M.compare(M.step(Pm, *rows, **kw), got)["failures"])
    print(f"{key}: {mutation}: failures {failures}")
    assert failures["dense"] + failures["threshold"] > 0
    if mutation == "inclusive bound made strict":
        assert failures["threshold"] > 0
