"""The host restatement of "nig-mlp-ln-v1" (csrc/nig_mlp_ln.hpp) for test_mlp_ln_host.py, test_gpu_mlp_ln.py and test_gpu_rsqrt.py:
tests/mlp_ln_ref.c compiled once per session (gcc -O2 -ffp-contract=off -mfma, as tests/mlp_shape_ref.py compiles its restatement),
its routines behind ctypes; the network in NumPy float64; the forward-error bound of the law against that network; and the
networks the tests share.  A plain helper module (no fixtures, no collection hooks)."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

import closed_loop_matrix as M

f32 = np.float32
_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None
EPS = 1e-6                 # flax's LayerNorm epsilon
U = 2.0 ** -24             # float32 unit roundoff


def lib():
    global _LIB
    if _LIB is None:
        d = tempfile.mkdtemp(prefix="nig_ln_ref_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        so = os.path.join(d, "libmlp_ln_ref.so")
        subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-fopenmp", "-shared", "-fPIC", "-o", so,
                        os.path.join(_HERE, "mlp_ln_ref.c"), "-lm"], check=True)
        _LIB = C.CDLL(so)
        _LIB.ln_rsqrtf.restype, _LIB.ln_rsqrtf.argtypes = C.c_float, [C.c_float]
        _LIB.ln_rsqrt_mismatches.restype = C.c_int64
    return _LIB


def _arrays(weights, norms):
    (W1, b1), (W2, b2), (W3, b3) = [(np.ascontiguousarray(W, dtype=f32), np.ascontiguousarray(np.asarray(b, dtype=f32).reshape(-1))) for W, b in weights]
    W3 = np.ascontiguousarray(W3.reshape(256, -1))
    (g1, e1), (g2, e2) = [(np.ascontiguousarray(np.asarray(g, dtype=f32).reshape(-1)), np.ascontiguousarray(np.asarray(b, dtype=f32).reshape(-1)))
                          for g, b in norms]
    assert W1.shape[1] == 256 and W2.shape == (256, 256) and all(a.shape == (256,) for a in (b1, b2, g1, e1, g2, e2)) and b3.shape == (W3.shape[1],)
    return [W1, b1, g1, e1, W2, b2, g2, e2, W3, b3]


def pre(weights, norms, obs, eps=EPS, hidden=False):
    """The head's pre-activations [n, A] (float32) of the LayerNorm actor on obs [n, S], in the law's order; hidden=True: also
    (h1, h2) [n, 256] each, the normalised layers behind their ReLU."""
    arr = _arrays(weights, norms)
    obs = np.ascontiguousarray(obs, dtype=f32)
    n, S = obs.shape
    A = arr[8].shape[1]
    assert arr[0].shape[0] == S
    out = np.zeros((n, A), dtype=f32)
    hid = np.zeros((n, 2, 256), dtype=f32) if hidden else None
    rc = lib().ln_pre(C.c_int64(n), S, A, *[a.ctypes.data_as(C.c_void_p) for a in arr], C.c_float(eps), obs.ctypes.data_as(C.c_void_p),
                      out.ctypes.data_as(C.c_void_p), None if hid is None else hid.ctypes.data_as(C.c_void_p))
    assert rc == 0
    return (out, hid[:, 0], hid[:, 1]) if hidden else out


def act(oracle, weights, norms, obs, eps=EPS):
    """The law's actions [n, A]: the oracle's det_tanhf of pre()."""
    return oracle.detmath_unary("tanhf", pre(weights, norms, obs, eps))


def rsqrt(x):
    """The restatement's det_rsqrtf of a (small) float32 array, value by value."""
    x = np.ascontiguousarray(x, dtype=f32)
    return np.array([lib().ln_rsqrtf(C.c_float(float(v))) for v in x.ravel()], dtype=f32).reshape(x.shape)


def rsqrt_mismatches(base, got):
    """(count, first index) of the floats got[i] that are not, bit for bit, the restatement's det_rsqrtf of the float with bits base + i"""
    got = np.ascontiguousarray(got, dtype=f32)
    first = C.c_int64(0)
    bad = lib().ln_rsqrt_mismatches(C.c_uint32(base), C.c_int64(got.size), got.ctypes.data_as(C.c_void_p), C.byref(first))
    return int(bad), int(first.value)


def model64(weights, norms, x, eps=EPS):
    """The formula in NumPy float64 -- no tiles, no lanes, no order: a dict of every intermediate the bound reads."""
    f64 = np.float64
    (W1, b1), (W2, b2), (W3, b3) = [(np.asarray(W, dtype=f64).reshape(np.shape(W)[0], -1), np.asarray(b, dtype=f64).reshape(-1)) for W, b in weights]
    out, h = {}, np.asarray(x, dtype=f64)
    for i, ((W, b), (g, be)) in enumerate(zip(((W1, b1), (W2, b2)), norms), start=1):
        g, be = np.asarray(g, dtype=f64).reshape(-1), np.asarray(be, dtype=f64).reshape(-1)
        z = h @ W + b
        out[f"abs{i}"] = np.abs(h) @ np.abs(W) + np.abs(b)
        d = z - z.mean(axis=1, keepdims=True)
        var = (d * d).mean(axis=1, keepdims=True)
        rs = 1.0 / np.sqrt(var + eps)
        y = d * (rs * g) + be
        h = np.maximum(y, 0)
        out.update({f"z{i}": z, f"d{i}": d, f"var{i}": var, f"rs{i}": rs, f"y{i}": y, f"h{i}": h, f"g{i}": g})
    out["pre"] = h @ W3 + b3
    out["abs3"] = h @ np.abs(W3) + np.abs(b3)
    out["W"] = (W1, W2, W3)
    out["action"] = np.tanh(out["pre"])
    return out


def gamma(n):
    return n * U / (1.0 - n * U)


def pre_bound(m, S, eps=EPS):
    """A forward-error bound [n, A] of the law's head pre-activations against model64's, to first order in u = 2^-24 (the terms of
    order u^2 are below 1e-6 of it: the largest factor beside u is 1 / sigma, a few hundred at most), from model64's dict `m`:
      Dense       a chain of n fma steps: |dz| <= gamma_n (|W|^T |h| + |b|) + |W|^T |dh|; n = S + 2 (layer 1, its bias and pad step),
                  258 (layer 2), 130 (a head chain, its bias and the joining add).
      mean        128 adds, the join and an exact scaling: |dmean| <= mean|dz| + gamma_129 mean|z|.
      d           |dd| <= |dz| + |dmean| + u |d|.
      variance    129 fma steps, the join: |dvar| <= 2 mean(|d| |dd|) + gamma_130 var.
      1 / sigma   the add of eps (u), sqrt and division (u each): relative rho = |dvar| / (2 (var + eps)) + 3 u.
      y           |dy| <= |gamma| rs (|dd| + |d| (rho + u)) + u |y|; ReLU does not enlarge it."""
    W1, W2, W3 = m["W"]
    dh = 0.0
    for i, (W, n) in enumerate(((W1, S + 2), (W2, 258)), start=1):
        dz = gamma(n) * m[f"abs{i}"] + (dh @ np.abs(W) if i > 1 else 0.0)
        z, d, var, rs, y, g = (m[f"{k}{i}"] for k in ("z", "d", "var", "rs", "y", "g"))
        dmean = dz.mean(axis=1, keepdims=True) + gamma(129) * np.abs(z).mean(axis=1, keepdims=True)
        dd = dz + dmean + U * np.abs(d)
        dvar = 2.0 * (np.abs(d) * dd).mean(axis=1, keepdims=True) + gamma(130) * var
        rho = dvar / (2.0 * (var + eps)) + 3.0 * U
        dh = np.abs(g) * rs * (dd + np.abs(d) * (rho + U)) + U * np.abs(y)
    return (gamma(130) * m["abs3"] + dh @ np.abs(W3)) * (1.0 + 1e-3)


def random_ln_actor(S, A, seed):
    """closed_loop_matrix.random_actor's weights with gamma ~ 1 + 0.3 N(0, 1) and beta ~ 0.2 N(0, 1) on both LayerNorms: (weights, norms)"""
    ws = M.random_actor(S, A, seed)
    rng = np.random.default_rng(seed + 1000)
    norms = [((1.0 + 0.3 * rng.normal(0, 1, 256)).astype(f32), (0.2 * rng.normal(0, 1, 256)).astype(f32)) for _ in range(2)]
    return ws, norms


def one_pass_f32(weights, norms, x, eps=EPS):
    """flax's one-pass form E[z^2] - E[z]^2 in float32 NumPy: what the law is NOT (shown beside it in profiles/ln/fidelity.txt)."""
    h = np.asarray(x, dtype=f32)
    for (W, b), (g, be) in zip(weights[:2], norms):
        z = (h @ np.asarray(W, dtype=f32) + np.asarray(b, dtype=f32)).astype(f32)
        mean = z.mean(axis=1, keepdims=True, dtype=f32)
        var = np.maximum((z * z).mean(axis=1, keepdims=True, dtype=f32) - mean * mean, f32(0))
        h = np.maximum((z - mean) * (f32(1) / np.sqrt(var + f32(eps))) * np.asarray(g, dtype=f32) + np.asarray(be, dtype=f32), f32(0)).astype(f32)
    return (h @ np.asarray(weights[2][0], dtype=f32).reshape(256, -1) + np.asarray(weights[2][1], dtype=f32)).astype(f32)


FIDELITY_SHAPES = ((12, 3), (32, 8), (28, 10))


def fidelity_cases(n=4096):
    """The cases test_mlp_ln_host.py asserts and profiles/ln_fidelity.py prints: (label, S, A, weights, norms, obs)."""
    for S, A in FIDELITY_SHAPES:
        ws, norms = random_ln_actor(S, A, 40 + S)
        obs = np.random.default_rng(S).normal(0, 1, (n, S)).astype(f32)
        yield f"S={S} A={A} obs~N(0,1)", S, A, ws, norms, obs
        yield f"S={S} A={A} obs~100 N(0,1)", S, A, ws, norms, (obs * f32(100)).astype(f32)


def shifted_bias_case(n=4096):
    """An actor whose first bias is shifted by 50: the mean is large beside the spread, where the one-pass variance loses the layer."""
    S, A = 12, 3
    ws, norms = random_ln_actor(S, A, 52)
    ws = [(ws[0][0], (ws[0][1] + f32(50)).astype(f32)), ws[1], ws[2]]
    return S, A, ws, norms, np.random.default_rng(S).normal(0, 1, (n, S)).astype(f32)
