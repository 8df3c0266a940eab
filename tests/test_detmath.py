"""not-gpu: the deterministic math library (csrc/nig_detmath.hpp) over its whole domain, on the oracle's restatement
(oracle/nig_oracle.c), which tests/test_gpu_detmath.py shows equal to the device bit for bit.  tests/detmath_check.c
sweeps every float32 input of exp, tanh, sigmoid and sin, every positive normal float for log, every float of the
Advanced envs' domains for pow, and structured float64 sets; the bounds asserted here are the
ones written in nig_detmath.hpp and DESIGN.md section 4.  Plus the MLP actor's tanh end at small pre-activations."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# divisors whose subnormal-side mismatch sets are pinned here (the device test checks every product divisor)
FDIV_PINNED = {"100": 335544, "418000": 320, "0.1": 8248796}


@pytest.fixture(scope="module")
def detmath(tmp_path_factory):
    exe = tmp_path_factory.mktemp("detmath") / "detmath_check"
    subprocess.run(["gcc", "-O2", "-std=gnu11", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-mfma", "-o", str(exe),
                    os.path.join(ROOT, "tests", "detmath_check.c"), "-lm"], check=True)
    out = subprocess.run([str(exe), "all"] + sorted(FDIV_PINNED), capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr
    res = {}
    for line in out.stdout.splitlines():
        name, worst, bad, n, at = line.split()
        res[name] = dict(worst=float(worst), bad=int(bad), n=int(n), at=at)
    return res


def _ok(r, name, bound):
    m = r[name]
    assert m["n"] > 0 and m["worst"] <= bound, (name, m)


def test_expf(detmath):
    _ok(detmath, "expf.normal", 1.5)               # ulp, every float with a normal result
    _ok(detmath, "expf.subnormal", 1.0)            # subnormal steps from RN(e^x)
    _ok(detmath, "expf.exact", 0)                  # inf above 88.72283, 0 below -104, 1 for |x| < 2^-25, NaN
    assert detmath["expf.normal"]["n"] + detmath["expf.subnormal"]["n"] + detmath["expf.exact"]["n"] == 2 ** 32


def test_logf(detmath):
    _ok(detmath, "logf.normal", 1.0)
    assert detmath["logf.normal"]["n"] == 254 * 2 ** 23


def test_tanhf(detmath):
    """<= 2 ulp everywhere including x -> 0 (the quotient form alone: 10 % at 1e-7, 0 below 3.7e-9), odd, |t| <= 1."""
    _ok(detmath, "tanhf.poly", 2.0)
    _ok(detmath, "tanhf.quot", 2.0)
    _ok(detmath, "tanhf.exact", 0)                 # tanh x == x below 2^-13, 1 from 9.1 on, NaN
    _ok(detmath, "tanhf.odd", 0)
    _ok(detmath, "tanhf.bounded", 0)
    assert detmath["tanhf.odd"]["n"] == 2 ** 31


def test_sigmoidf(detmath):
    _ok(detmath, "sigmoidf.normal", 3.0)
    _ok(detmath, "sigmoidf.subnormal", 1.0)
    _ok(detmath, "sigmoidf.exact", 0)              # +0 below -88.72283 (stated), 1 from 17.4, 1/2 for |x| < 2^-25
    _ok(detmath, "sigmoidf.monotone", 0)           # the shield's p < threshold relies on it
    assert detmath["sigmoidf.monotone"]["n"] == 2 ** 32 - (2 ** 24 - 2) - 1     # every float but NaN and +inf


def test_sinf(detmath):
    _ok(detmath, "sinf.abs", 8e-8)                 # |x| <= 1e4, the stated domain
    _ok(detmath, "sinf.exact", 0)


def test_powf(detmath):
    """The measured bounds over the Advanced envs' domains (nig_detmath.hpp det_powf)."""
    _ok(detmath, "powf.0.8.re", 24.0)              # Re^0.8, Re in [1, 2^29)
    _ok(detmath, "powf.0.8.below1", 128.0)         # Re below 1
    for y in ("1.2", "1.3", "1.5", "1.8"):
        _ok(detmath, f"powf.{y}.v", 2.5)           # V^alpha, V in [0.5, 2)


def test_exp64(detmath):
    _ok(detmath, "exp64.normal", 1.0)
    _ok(detmath, "exp64.subnormal", 1.0)
    _ok(detmath, "exp64.exact", 0)
    assert detmath["exp64.normal"]["n"] + detmath["exp64.subnormal"]["n"] >= 10 ** 7


def test_sincos(detmath):
    _ok(detmath, "sincos.abs", 2.3e-16)            # |x| <= 64
    _ok(detmath, "sincos.exact", 0)
    assert detmath["sincos.abs"]["n"] >= 10 ** 7


def test_fdiv_c_subnormal_side_is_the_stated_set(detmath):
    """Below |x| = 2^-100 the 4-instruction division differs from IEEE on a fixed, counted set per divisor (DESIGN.md
    section 4); the device test checks that the device has the same set."""
    for c, count in FDIV_PINNED.items():
        assert detmath[f"fdiv.{c}.tiny"]["bad"] == count, (c, detmath[f"fdiv.{c}.tiny"])


def _ulp32(v):
    """float32 ulp of float64 values v (not below the subnormal step)."""
    e = np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** -126)))
    return 2.0 ** (e - 23)


def scaled_head_actor(S, A, obs, seed=7):
    """An actor whose head pre-activations span about 1e-9 .. 3 on the observations obs: the head columns (W3 and b3) of a
    random actor rescaled so that the median |pre-activation| of action j is 1e-9 .. 1e-3 (geometric steps) and 3 for
    the last action (the range of tanh's quotient form)."""
    rng = np.random.default_rng(seed)
    ws = [(rng.normal(0, 1.0 / np.sqrt(S), (S, 256)).astype(np.float32) * np.float32(0.05), rng.normal(0, 0.05, 256).astype(np.float32)),
          (rng.normal(0, 1.0 / 16, (256, 256)).astype(np.float32), rng.normal(0, 0.05, 256).astype(np.float32)),
          (rng.normal(0, 1.0 / 8, (256, A)).astype(np.float32), rng.normal(0, 0.1, A).astype(np.float32))]
    h = np.asarray(obs, dtype=np.float64)
    for W, b in ws[:2]:
        h = np.maximum(h @ W.astype(np.float64) + b, 0.0)
    pre = h @ ws[2][0].astype(np.float64) + ws[2][1]
    target = np.append(np.geomspace(1e-9, 1e-3, A - 1), 3.0)
    scale = (target / np.median(np.abs(pre), axis=0)).astype(np.float32)
    ws[2] = ((ws[2][0] * scale[None, :]).astype(np.float32), (ws[2][1] * scale).astype(np.float32))
    return ws


def assert_tanh_end(pre, act):
    """every action within 2 float32 ulp of tanh(pre) in float64"""
    want = np.tanh(pre.astype(np.float64))
    err = np.abs(act.astype(np.float64) - want) / _ulp32(want)
    assert err.max() <= 2.0, (err.max(), pre.ravel()[np.argmax(err)])


def test_actor_tanh_end_at_small_preactivations(oracle):
    """CPU twin of test_gpu_parity.py's scaled-head test: the oracle's actor (the device's operation sequence) ends in
    det_tanhf, and its output is within 2 ulp of tanh of its own pre-activation wherever that lies in 1e-9 .. 3."""
    for key, S, A in (("cr", 12, 3), ("pg", 32, 8)):
        obs = np.random.default_rng(3).normal(0, 1, (4000, S)).astype(np.float32)
        ws = scaled_head_actor(S, A, obs)
        pre = oracle.mlp_preact(key, ws, obs)
        act = oracle.mlp_actions(key, ws, obs)
        small = np.abs(pre[:, :-1])
        assert small.min() < 1e-7 and small.max() < 1e-1 and np.abs(pre[:, -1]).max() > 1.0, (small.min(), small.max())
        assert_tanh_end(pre, act)
