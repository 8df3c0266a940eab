"""The host restatement of the constraint projection ("nig-project-v1", include/nig.h) for test_projection_host.py and
test_gpu_projection.py: tests/mlp_project_ref.c compiled once per session (gcc -O2 -ffp-contract=off, as
tests/test_expf_scale.py compiles its checker), its two routines behind ctypes, the law around them with the oracle's
det_sigmoidf, and the law once more in NumPy float64 with the distance of every decision from its boundary.  A plain helper
module (no fixtures, no collection hooks)."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

f32 = np.float32
_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        d = tempfile.mkdtemp(prefix="nig_project_ref_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        so = os.path.join(d, "libmlp_project_ref.so")
        subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-mfma", "-fopenmp", "-shared", "-fPIC", "-o", so,
                        os.path.join(_HERE, "mlp_project_ref.c"), "-lm"], check=True)
        _LIB = C.CDLL(so)
    return _LIB


def _p(x):
    return x.ctypes.data_as(C.c_void_p)


def _w(layers):
    W = [np.ascontiguousarray(x, dtype=f32) for pair in layers for x in pair]
    W[4] = W[4].reshape(W[2].shape[0], -1)
    return W


def forward(layers, obs, act, masks=False):
    """(z [n, C], g [n, A]) -- the predictor's logits and dG/da at (obs, act) -- and, with masks, [n, 2, h] the ReLU masks."""
    W = _w(layers)
    h, Cn = W[0].shape[1], W[4].shape[1]
    obs, act = np.ascontiguousarray(obs, dtype=f32), np.ascontiguousarray(act, dtype=f32)
    n, S, A = obs.shape[0], obs.shape[1], act.shape[1]
    assert W[0].shape[0] == S + A
    z, g = np.zeros((n, Cn), dtype=f32), np.zeros((n, A), dtype=f32)
    mk = np.zeros((n, 2, h), dtype=np.uint8) if masks else None
    rc = lib().proj_forward(C.c_int64(n), h, S, A, Cn, *[_p(x) for x in W], _p(obs), _p(act), _p(z), _p(g), _p(mk) if masks else None)
    assert rc == 0
    return (z, g, mk) if masks else (z, g)


def law(oracle, layers, obs, a0, thr, tol, max_iters, step):
    """The law on (obs [n, S], a0 [n, A]): dict of p0 [n, C], projected [n], act [n, A] (what the env receives), iters [n],
    viol [n, C], grad [n, A] (the first gradient; NaN-free zeros where iters < 1) and z [n, C] (the final logits)."""
    W = _w(layers)
    h, Cn = W[0].shape[1], W[4].shape[1]
    obs, act = np.ascontiguousarray(obs, dtype=f32), np.array(a0, dtype=f32, order="C")
    n, S, A = obs.shape[0], obs.shape[1], act.shape[1]
    z0, _ = forward(layers, obs, act)
    p0 = oracle.detmath_unary("sigmoidf", z0)
    with np.errstate(invalid="ignore"):
        projected = ~(p0 < f32(thr)).all(axis=1)
    iters, z, g0 = np.zeros(n, dtype=np.int32), np.zeros((n, Cn), dtype=f32), np.zeros((n, A), dtype=f32)
    rc = lib().proj_loop(C.c_int64(n), h, S, A, Cn, *[_p(x) for x in W], _p(obs), _p(np.ascontiguousarray(projected, dtype=np.uint8)),
                         C.c_float(tol), int(max_iters), C.c_float(step), _p(act), _p(iters), _p(z), _p(g0))
    assert rc == 0
    return dict(p0=p0, projected=projected, act=act, iters=iters, viol=oracle.detmath_unary("sigmoidf", z), grad=g0, z=z)


def forward64(layers, obs, act):
    """The predictor in NumPy float64: (z, y1, y2) -- logits and the two hidden layers' pre-activations."""
    (W1, b1), (W2, b2), (W3, b3) = [(np.asarray(W, dtype=np.float64), np.asarray(b, dtype=np.float64)) for W, b in layers]
    x = np.concatenate([np.asarray(obs, dtype=np.float64), np.asarray(act, dtype=np.float64)], axis=1)
    y1 = x @ W1 + b1
    y2 = np.maximum(y1, 0) @ W2 + b2
    return np.maximum(y2, 0) @ W3.reshape(W2.shape[0], -1) + b3, y1, y2


def gradient64(layers, S, z, y1, y2):
    """dG/da in NumPy float64: W1[S:S+A, :] (m1 . (W2 (m2 . (W3 d)))), d = (z > 0)."""
    W1, W2, W3 = [np.asarray(W, dtype=np.float64) for W, _ in layers]
    W3 = W3.reshape(W2.shape[0], -1)
    g2 = ((z > 0).astype(np.float64) @ W3.T) * (y2 > 0)
    g1 = (g2 @ W2.T) * (y1 > 0)
    return g1 @ W1[S:].T


def law64(layers, obs, a0, thr, tol, max_iters, step):
    """The law in NumPy float64, and `margin` [n]: the least distance of anything a lane's decisions compare from its boundary
    over all of the lane's passes -- hidden pre-activations and logits from 0, logits from tol, sigmoid(z0) from thr.  A float32
    evaluation whose error stays below the margin takes the same branches."""
    obs = np.asarray(obs, dtype=np.float64)
    S = obs.shape[1]
    a = np.array(a0, dtype=np.float64)
    z, y1, y2 = forward64(layers, obs, a)

    def dist(z, y1, y2):
        return np.minimum(np.minimum(np.abs(y1).min(axis=1), np.abs(y2).min(axis=1)), np.minimum(np.abs(z).min(axis=1), np.abs(z - tol).min(axis=1)))
    p0 = 1.0 / (1.0 + np.exp(-z))
    margin = np.minimum(dist(z, y1, y2), np.abs(p0 - thr).min(axis=1))
    projected = ~(p0 < thr).all(axis=1)
    active = projected.copy()
    iters = np.where(projected, 0, -1)
    g_first = np.zeros_like(a)
    for k in range(max_iters):
        active &= ~(z < tol).all(axis=1)
        if not active.any():
            break
        g = gradient64(layers, S, z, y1, y2)
        if k == 0:
            g_first = np.where(active[:, None], g, 0.0)
        a = np.where(active[:, None], np.clip(a - step * g, -1.0, 1.0), a)
        iters = iters + active
        z2, u1, u2 = forward64(layers, obs, a)
        margin = np.where(active, np.minimum(margin, dist(z2, u1, u2)), margin)
        z, y1, y2 = np.where(active[:, None], z2, z), np.where(active[:, None], u1, y1), np.where(active[:, None], u2, y2)
    return dict(act=a, iters=iters, projected=projected, margin=margin, z=z, grad=g_first)
