"""The host restatement of "nig-mlp-shape-v1" (include/nig.h) for test_mlp_shape_host.py and test_gpu_mlp_shape.py:
tests/mlp_shape_ref.c compiled once per session (gcc -O2 -ffp-contract=off -mfma, as tests/projection_ref.py compiles its
restatement), its routine behind ctypes, and the network in NumPy float64 for any number of hidden layers.  A plain helper module
(no fixtures, no collection hooks)."""
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

# the classes of the law: name -> padded hidden widths; and the hidden shapes the tests install for each shaped class
CLASSES = {"128x128": (128, 128), "512x256": (512, 256), "512x512": (512, 512), "256x256x256": (256, 256, 256)}
SHIPPED = tuple(CLASSES)


def lib():
    global _LIB
    if _LIB is None:
        d = tempfile.mkdtemp(prefix="nig_shape_ref_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        so = os.path.join(d, "libmlp_shape_ref.so")
        subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-mfma", "-shared", "-fPIC", "-o", so,
                        os.path.join(_HERE, "mlp_shape_ref.c"), "-lm"], check=True)
        _LIB = C.CDLL(so)
    return _LIB


def _layers(weights):
    ws = [(np.ascontiguousarray(W, dtype=f32), np.ascontiguousarray(np.asarray(b, dtype=f32).reshape(-1))) for W, b in weights]
    ws[-1] = (np.ascontiguousarray(ws[-1][0].reshape(ws[-2][0].shape[1], -1)), ws[-1][1])
    return ws


def pre(weights, obs):
    """The head's pre-activations [n, A] (float32) of the actor `weights` on obs [n, S], in the law's order."""
    ws = _layers(weights)
    obs = np.ascontiguousarray(obs, dtype=f32)
    n, S = obs.shape
    A, nh = ws[-1][0].shape[1], len(ws) - 1
    assert ws[0][0].shape[0] == S
    dims = (C.c_int32 * nh)(*[W.shape[1] for W, _ in ws[:-1]])
    Wp = (C.c_void_p * len(ws))(*[W.ctypes.data for W, _ in ws])
    bp = (C.c_void_p * len(ws))(*[b.ctypes.data for _, b in ws])
    out = np.zeros((n, A), dtype=f32)
    rc = lib().shape_pre(C.c_int64(n), S, A, nh, dims, Wp, bp, obs.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    assert rc == 0
    return out


def act(oracle, weights, obs):
    """The law's actions [n, A]: the oracle's det_tanhf of pre()."""
    return oracle.detmath_unary("tanhf", pre(weights, obs))


def pre64(weights, x):
    """The network's head pre-activations in NumPy float64 for any number of hidden layers (closed_loop_matrix.mlp64 is this
    for two): no tiles, no chunks, no lanes."""
    z = np.asarray(x, dtype=np.float64)
    for i, (W, b) in enumerate(weights):
        z = z @ np.asarray(W, dtype=np.float64).reshape(z.shape[-1], -1) + np.asarray(b, dtype=np.float64).reshape(-1)
        if i + 1 < len(weights):
            z = np.maximum(z, 0)
    return z


def random_actor(S, A, dims, seed):
    """closed_loop_matrix.random_actor's construction for any hidden widths: W1 ~ 0.05 N(0, 1 / sqrt(S)), a hidden layer with K
    inputs ~ N(0, 1 / sqrt(K)), the head ~ N(0, sqrt(2 / K)), biases N(0, 0.05) (the head's N(0, 0.1)) -- which at (256, 256) are that
    function's 1 / 16 and 1 / 8."""
    rng = np.random.default_rng(seed)
    ws = [(rng.normal(0, 1.0 / np.sqrt(S), (S, dims[0])).astype(f32) * f32(0.05), rng.normal(0, 0.05, dims[0]).astype(f32))]
    for K, H in zip(dims[:-1], dims[1:]):
        ws.append((rng.normal(0, 1.0 / np.sqrt(K), (K, H)).astype(f32), rng.normal(0, 0.05, H).astype(f32)))
    K = dims[-1]
    ws.append((rng.normal(0, np.sqrt(2.0 / K), (K, A)).astype(f32), rng.normal(0, 0.1, A).astype(f32)))
    return ws
