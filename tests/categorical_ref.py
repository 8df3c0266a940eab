"""The law "nig-categorical-v1" (include/nig.h) restated in NumPy, and what the categorical-critic tests share: a plain helper
module (no fixtures, no collection hooks).

violation_prob(): float32 operations in the law's stated order -- the max, det_expf of the float32 difference (the oracle's
restatement of the device's det_expf), the four groups' left-to-right sums in row order, (t0 + t1) + (t2 + t3), one division.
mass64(): the reference's lines (agents/safety_critical.py:151-171: softmax, then the sum of the masked atoms) in float64.
radius(): the bound of the first against the second on the same logits, derived below and not tuned."""
import numpy as np

f32 = np.float32


def default_mask(atoms, v_min=-1.0, v_max=1.0, safety_threshold=0.0):
    below = np.linspace(v_min, v_max, atoms, dtype=f32) < f32(safety_threshold)
    return sum(1 << j for j in range(atoms) if below[j])


def violation_prob(oracle, z, below_mask):
    """p [n] float32 of logits z [N, n] float32 (row j: atom j), bit for bit what the law states."""
    z = np.ascontiguousarray(z, dtype=f32)
    N, n = z.shape
    assert 2 <= N <= 64 and below_mask >> N == 0
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        m = np.full(n, -np.inf, dtype=f32)
        for j in range(N):
            m = np.fmax(m, z[j])                                   # fmaxf: a NaN takes no part
        e = oracle.detmath_unary("expf", (z - m[None, :]).astype(f32)).reshape(N, n)
        t, v = np.zeros((4, n), dtype=f32), np.zeros((4, n), dtype=f32)
        for q in range(4):
            for P in range(4):
                for i in range(4):
                    j = 16 * P + 4 * q + i
                    if j < N:
                        t[q] = t[q] + e[j]
                        if (below_mask >> j) & 1:
                            v[q] = v[q] + e[j]
        T = (t[0] + t[1]) + (t[2] + t[3])
        V = (v[0] + v[1]) + (v[2] + v[3])
        p = V / T
    assert p.dtype == f32
    return p


def mass64(z, below_mask):
    """The reference's formula in float64 on logits z [N, n]: softmax over the atoms, then the sum over the masked atoms."""
    z = np.asarray(z, dtype=np.float64)
    N = z.shape[0]
    e = np.exp(z - z.max(axis=0, keepdims=True))
    dist = e / e.sum(axis=0, keepdims=True)                        # nn.softmax(logits, axis=-1)
    mask = np.array([(below_mask >> j) & 1 for j in range(N)], dtype=np.float64)
    return (dist * mask[:, None]).sum(axis=0)                      # jnp.sum(safety_dist * violation_mask, axis=-1)


def radius(N):
    """|p - mass64| <= radius(N) for finite logits, with u = 2^-24:
      e_j    the argument z_j - m is one float32 subtraction: relative error u in d = m - z_j >= 0, which changes e^-d by at most
             u d e^-d <= u / e absolutely (x e^-x <= 1 / e); det_expf is within 1.5 ulp = 3 u relative where its result is a normal
             float (tests/test_detmath.py "expf.normal" 1.5) and within one subnormal step, or below 2^-148 where it returns 0,
             elsewhere (< 2^-126: nothing beside u).  So |e_j' - e_j| <= 3 u e_j + u / e.
      sums   N non-negative terms, each passing through at most N - 1 inexact float32 additions (an addition of +0 is exact):
             |fl(sum) - sum| <= (N - 1) u sum.  With the terms' own errors: |T' - T| <= (3 + N - 1) u T + N u / e, V likewise (V <= T).
      p      T >= 1 (the max term is 1), p = V / T <= 1, one division (u): |p' - p| <= (|dV| + p |dT|) / T + u
             <= 2 ((N + 2) u + N u / e) + u, and 1 % on top for the second-order terms."""
    u = 2.0 ** -24
    return 1.01 * (2.0 * ((N + 2) * u + N * u / np.e) + u)


def same_bits(a, b):
    """Equal as bit patterns, a NaN equal to any NaN (the law fixes that p is NaN, not which)."""
    a, b = np.ascontiguousarray(a, dtype=f32), np.ascontiguousarray(b, dtype=f32)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])


def random_categorical_critic(S, A, atoms, seed):
    """closed_loop_matrix.random_critic with a head of `atoms` columns whose weights are small enough that the softmax does not
    saturate on one atom (the one-column critic's N(0, 1/2) head gives logits of order 10: p would be 0 or 1 in most lanes; with
    N(0, 1/8) and hidden activations of order 1 the logits have a spread of order 1, so two atoms stay inside (0.001, 0.999))."""
    rng, D = np.random.default_rng(seed), S + A
    return [(rng.normal(0, 1.0 / np.sqrt(D), (D, 256)).astype(f32) * f32(0.05), rng.normal(0, 0.05, 256).astype(f32)),
            (rng.normal(0, 1.0 / 16, (256, 256)).astype(f32), rng.normal(0, 0.05, 256).astype(f32)),
            (rng.normal(0, 1.0 / 8, (256, atoms)).astype(f32), rng.normal(0, 0.1, atoms).astype(f32))]
