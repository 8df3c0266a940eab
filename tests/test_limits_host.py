"""not-gpu: the added box constraints ("nig-limits-v1", include/nig.h nig_set_limits) against the reference's recorded steps
(tests/golden/limits_<key>.npz: the reference env with four added SafetyConstraints, tests/gen_limits_golden.py) -- the box
law as BoxConstraint.check_fn states it, the reward order restated in NumPy, the ABI's declarations and the Python surface's
refusals.  The device side is tests/test_gpu_limits.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import limits_fixture as F
from conftest import ENV_NAME, KEYS, ROOT, RTOL, rel_err

SETS = ("s1_", "s2_", "s1_a64_", "s2_a64_")


@pytest.fixture(scope="module")
def ni():
    import neorl_industrial_gym_amd as ni
    return ni


@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("prefix", SETS)
def test_check_fn_reproduces_every_recorded_added_bit(ni, key, prefix):
    """BoxConstraint.check_fn on (pre-state, clipped action) is the reference's recorded bit of every added constraint on every
    tuple, float32 and genuine float64 actions; each constraint fires somewhere and holds somewhere."""
    d = F.load(key)
    t = F.tuples(d, prefix)
    S, A = t["state_pre"].shape[1], t["action"].shape[1]
    cons = F.boxes(ni, d, int(prefix[1]), S, A)
    act = t["action64"] if "action64" in t else t["action"]
    clipped = np.clip(act, act.dtype.type(-1), act.dtype.type(1))
    assert clipped.dtype == act.dtype
    got = np.array([[0 if c.check_fn(s, a) else 1 for c in cons] for s, a in zip(t["state_pre"], clipped)], dtype=np.uint8)
    assert np.array_equal(got, t["viol_bits"][:, 3:])
    assert (got.sum(axis=0) > 0).all() and (got.sum(axis=0) < len(got)).all()
    assert np.array_equal(t["viol"], t["viol_bits"].sum(axis=1))


@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("prefix", SETS)
def test_reward_order_reproduces_the_recorded_rewards(ni, key, prefix):
    """The reference's reward before penalties (recorded), then the penalties in base.py's order in the env's reward type, then
    ONE -1000: ChemicalReactor with float32 actions bit-exact in float32, otherwise float64 within the project's 1e-5 rule.
    The corner tuples (a built-in critical violation together with an added violation; an added critical violation alone)
    are in the set; terminated and the critical count follow the same bits."""
    d = F.load(key)
    t = F.tuples(d, prefix)
    k = int(prefix[1])
    sp = ni._lib.env_spec(ni.batched.ENV_IDS[ENV_NAME[key]])
    rtype = np.float32 if (key == "cr" and "action64" not in t) else np.float64
    vb = t["viol_bits"]
    want, crit = F.reward_law(t["reward_raw"], vb[:, :3], list(sp.penalty), list(sp.critical), vb[:, 3:], d[f"s{k}_penalty"],
                              d[f"s{k}_critical"], rtype)
    if rtype is np.float32:
        assert np.array_equal(want, t["reward"])
    else:
        assert rel_err(want, t["reward"]).max() <= RTOL
    assert np.array_equal(crit, t["crit"])
    assert (t["terminated"][crit > 0] == 1).all()
    builtin_crit = (vb[:, :3] * np.asarray(list(sp.critical))[None, :]).sum(axis=1) > 0
    assert (builtin_crit & (vb[:, 3:].sum(axis=1) > 0)).sum() >= (32 if "a64" not in prefix else 0)
    if prefix == "s2_":
        alone = ((vb[:, 3:] * d["s2_critical"][None, :]).sum(axis=1) > 0) & ~builtin_crit
        assert alone.sum() >= 32 and (t["terminated"][alone] == 1).all()


def test_the_abi_is_declared_bound_and_exported(ni):
    L = ni._lib.lib()
    hdr = open(os.path.join(ROOT, "include", "nig.h")).read()
    for name in ("nig_set_limits", "nig_get_limit_count", "nig_step_limited", "nig_step64_limited", "nig_rollout_policy_limited",
                 "nig_rollout_mlp_limited"):
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in ni._lib.PROTOTYPES and hasattr(L, name), name
    # the struct as the header lays it out: 8 + 2 * 4 * NIG_LIMIT_ROWS + 8 + 4 + 4 bytes, no padding
    rows = int(re.search(r"#define NIG_LIMIT_ROWS (\d+)", hdr).group(1))
    assert rows == ni._lib.LIMIT_ROWS >= 40 and int(re.search(r"#define NIG_MAX_LIMITS (\d+)", hdr).group(1)) == ni._lib.MAX_LIMITS == 4
    assert C.sizeof(ni._lib.LimitStruct) == 8 + 8 * rows + 16
    assert ni._lib.LimitStruct.penalty.offset == 8 + 8 * rows and ni._lib.LimitStruct.critical.offset == 16 + 8 * rows
    assert L.nig_get_limit_count(None) == -1
    assert L.nig_version().decode().startswith("nig 0.8.0")


def test_box_constraint_is_a_safety_constraint(ni):
    c = ni.BoxConstraint("band", {("state", 2): (-1.0, 1.0), ("action", 0): (-np.inf, 0.5)}, -3.0, critical=True, description="d")
    assert isinstance(c, ni.SafetyConstraint) and (c.name, c.penalty, c.critical, c.description) == ("band", -3.0, True, "d")
    s, a = np.zeros(4, np.float32), np.zeros(2, np.float32)
    assert c.check_fn(s, a) is True
    s[2] = np.nan
    assert c.check_fn(s, a) is False                    # a NaN in a listed row violates
    s[2], s[0] = 0.0, np.nan
    assert c.check_fn(s, a) is True                     # an unlisted row is never looked at
    a[0] = np.nextafter(np.float32(0.5), np.float32(1))
    assert c.check_fn(s, a) is False
    assert c.check_fn(s, np.array([0.5, 0.0])) is True and c.check_fn(s, np.array([0.5 + 1e-12, 0.0])) is False      # float64: the bound widened
    assert c.limit_rows(4, 2) == (0b010100, {2: (np.float32(-1), np.float32(1)), 4: (np.float32(-np.inf), np.float32(0.5))})
    with pytest.raises(ValueError):
        ni.BoxConstraint("bad", {("state", 0): (1.0, 0.0)}, 0.0)
    with pytest.raises(ValueError):
        ni.BoxConstraint("bad", {("state", 0): (np.nan, 0.0)}, 0.0)
    with pytest.raises(ValueError):
        ni.BoxConstraint("bad", {}, 0.0)
    with pytest.raises(ValueError):
        ni.BoxConstraint("bad", {("obs", 0): (0.0, 1.0)}, 0.0)
    with pytest.raises(ValueError):
        c.limit_rows(2, 2)


def test_the_batched_env_refuses_callables_that_are_not_boxes(ni):
    """add_safety_constraint is type-checked before anything touches the device: an arbitrary check_fn is a TypeError that
    points at the single env."""
    env = object.__new__(ni.BatchedIndustrialEnv)      # no handle: the refusal needs none
    env._added = []
    with pytest.raises(TypeError, match="single env"):
        env.add_safety_constraint(ni.SafetyConstraint("f", lambda s, a: True, -1.0))
    with pytest.raises(TypeError, match="BoxConstraint"):
        env.add_safety_constraint(lambda s, a: True)
    env._h = None
