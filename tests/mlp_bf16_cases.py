"""The exact-integer cases of "nig-mlp-bf16-v1" (include/nig.h), shared by tests/test_mlp_bf16_host.py and
tests/test_gpu_mlp_bf16.py.  A plain helper module (no fixtures, no collection hooks).

Every weight, bias and state is a small integer times a power of two, so that every term of every sum is a multiple of one
quantum and every partial sum, in ANY order, is below 2^24 quanta: float32 accumulation is then exact, the summation order and
the matrix unit's internal order cannot matter, and the law fixes every word.  What is left to go wrong is the layout: which
weight meets which activation in which lane.  The weights are dense, random and asymmetric with a seed per env.

Set A   states integers in [-4, 4]; W1 in {-1, 0, 1}, b1 integers in [-2, 2]; W2 in {-1, 0, 1} 2^-6, b2 integers 2^-6;
        W3 in {-1, 0, 1} 2^-10, b3 = 0.
Set B   the lo half of the input split and round-to-nearest-even ties: states integers in (-2^15, 2^15), W1 in {-1, 0, 1} 2^-8,
        b1 as set A.  z1 then has up to 23 significant bits, h1 = bf(relu(z1)) keeps a quantum of 2^-8 on its small values, and
        sum |h1| stays below 2^16 = 2^24 quanta.  Behind a dense layer 2 of set A's kind sum |h2| would be ~2^12 at a quantum
        of 2^-14: 2^26 quanta, not exact in every order.  So b2 = (-2 sigma + integers in [-2, 2]) 2^-6, sigma = the standard
        deviation of sum_k +-h1_k: about one unit in forty survives the ReLU, sum |h2| is ~2^7, and W3 in {-1, 0, 1} 2^-4 keeps
        z3 of order 1.  Hidden unit 0 of layer 1 reads state 0 alone (W1[0][0] = 2^-8, b1[0] = 0), and lanes 0 and 1 hold
        s_0 = 257 and 259: hi = 256 / 260 (ties to even, down and up), lo = +1 / -1, z1 = 257/256 and 259/256, h1 = 1 and
        1 + 2^-6 (ties again, down and up).
quanta_ok() is the host assertion that the data is what this says."""
import numpy as np

f32 = np.float32
SEEDS = {"cr": 11, "pg": 12, "ra": 13, "acr": 14, "apg": 15, "hvac": 16, "steel": 17, "supply": 18}


def _tri(rng, shape, scale):
    return (rng.integers(-1, 2, shape).astype(f32) * f32(scale)).astype(f32)


def set_a(key, S, A, B):
    rng = np.random.default_rng(1000 + SEEDS[key])
    ws = [(_tri(rng, (S, 256), 1.0), rng.integers(-2, 3, 256).astype(f32)),
          (_tri(rng, (256, 256), 2.0 ** -6), (rng.integers(-8, 9, 256).astype(f32) * f32(2.0 ** -6)).astype(f32)),
          (_tri(rng, (256, A), 2.0 ** -10), np.zeros(A, f32))]
    states = rng.integers(-4, 5, (B, S)).astype(f32)
    return ws, states


def set_b(key, S, A, B):
    rng = np.random.default_rng(2000 + SEEDS[key])
    W1 = _tri(rng, (S, 256), 2.0 ** -8)
    b1 = rng.integers(-2, 3, 256).astype(f32)
    W1[:, 0] = 0
    W1[0, 0] = f32(2.0 ** -8)
    b1[0] = 0
    # sigma of sum_k +-h1_k over 256 units, two in three of them connected: z1 ~ N(0, s1^2), s1^2 = S (2/3) (2^30 / 3) 2^-16,
    # E[h1^2] = s1^2 / 2
    s1 = np.sqrt(S * (2.0 / 3.0) * (2.0 ** 30 / 3.0)) * 2.0 ** -8
    sigma = np.sqrt(256 * (2.0 / 3.0) * s1 * s1 / 2.0)
    b2 = ((rng.integers(-2, 3, 256) - int(round(2.0 * sigma))).astype(f32) * f32(2.0 ** -6)).astype(f32)
    ws = [(W1, b1), (_tri(rng, (256, 256), 2.0 ** -6), b2), (_tri(rng, (256, A), 2.0 ** -4), np.zeros(A, f32))]
    states = rng.integers(-2 ** 15 + 1, 2 ** 15, (B, S)).astype(f32)
    states[0, 0], states[1, 0] = 257, 259
    return ws, states


def _lowbit(x):
    """The largest power of two dividing every nonzero entry of the float array x (float64)."""
    x = np.abs(np.asarray(x, dtype=np.float64))
    x = x[x > 0]
    if x.size == 0:
        return 1.0
    m, e = np.frexp(x)
    mant = np.round(m * 2.0 ** 53).astype(np.int64)          # exact: 53-bit mantissas
    tz = np.log2((mant & -mant).astype(np.float64))
    return float(2.0 ** np.min(e - 53 + tz))


def quanta_ok(ref, ws, states):
    """Host assertion: in every layer, every term (and the bias) is a multiple of one quantum and sum |term| < 2^24 quanta, so
    float32 accumulation in any order is exact.  ref = policies.mlp_bf16_reference(ws, states).  Returns the three spans in
    quanta (for printing)."""
    from neorl_industrial_gym_amd.policies import bf16_round, bf16_split
    hi, lo = bf16_split(states)
    xs = [np.concatenate([hi, lo], axis=1), ref["h1"], ref["h2"]]
    spans = []
    for k, (x, (W, b)) in enumerate(zip(xs, ws), start=1):
        q = _lowbit(x) * _lowbit(bf16_round(W))
        if np.any(b != 0):
            q = min(q, _lowbit(b))
        span = float(np.max(ref[f"abs{k}"])) / q
        assert span < 2.0 ** 24, (k, span, q)
        spans.append(span)
    return spans


def ties_and_lo(ref, states):
    """(number of exact round-to-nearest-even ties among the h1 and h2 roundings, number of nonzero lo parts)."""
    from neorl_industrial_gym_amd.policies import bf16_split
    ties = 0
    for k in (1, 2):
        z = np.maximum(ref[f"z{k}"], 0).astype(f32)
        assert np.array_equal(z.astype(np.float64), np.maximum(ref[f"z{k}"], 0)), "z is exact in float32"
        ties += int(((z.view(np.uint32) & np.uint32(0xFFFF)) == np.uint32(0x8000)).sum())
    _, lo = bf16_split(states)
    return ties, int((lo != 0).sum())


def int_reference(ws, states):
    """Set A in plain integer arithmetic (no floating point until the last line): h1, h2 as float32 holding bf16 values, z3 as
    float64.  Layer 1 in units of 1, layer 2 in units of 2^-6, layer 3 in units of 2^-16; bf of a non-negative integer n of
    quanta is done on integers (keep the top 8 bits, round half to even)."""
    def bf_int(n):
        n = np.asarray(n, dtype=np.int64)
        bits = np.where(n > 0, np.floor(np.log2(np.maximum(n, 1))).astype(np.int64) + 1, 0)
        sh = np.maximum(bits - 8, 0)
        low = n & ((np.int64(1) << sh) - 1)
        half = np.where(sh > 0, np.int64(1) << np.maximum(sh - 1, 0), 0)
        up = (low > half) | ((low == half) & (sh > 0) & (((n >> sh) & 1) == 1))
        return ((n >> sh) + up.astype(np.int64)) << sh
    (W1, b1), (W2, b2), (W3, b3) = ws
    I = lambda x, scale: np.round(np.asarray(x, dtype=np.float64) * scale).astype(np.int64)
    s = I(states, 1)
    z1 = s @ I(W1, 1) + I(b1, 1)
    h1 = bf_int(np.maximum(z1, 0))
    z2 = h1 @ I(W2, 64) + I(b2, 64)                      # units of 2^-6
    h2 = bf_int(np.maximum(z2, 0))
    z3 = h2 @ I(W3, 1024) + I(b3, 65536)                 # units of 2^-16
    return h1.astype(f32), (h2.astype(np.float64) / 64).astype(f32), z3.astype(np.float64) / 65536
