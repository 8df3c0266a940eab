"""The exact-integer cases of "nig-mlp-bf16-v1" (include/nig.h), shared by tests/test_mlp_bf16_host.py and
tests/test_gpu_mlp_bf16.py.  A plain helper module (no fixtures, no collection hooks).

Every weight, bias and state is a small integer times a power of two, so that every term of every sum is a multiple of one
quantum and every partial sum, in ANY order, is below 2^24 quanta: float32 accumulation is then exact, the summation order and
the matrix unit's internal order cannot matter, and the law fixes every word.  What is left to go wrong is the layout: which
weight meets which activation in which lane.  The weights are dense, random and asymmetric with a seed per env.

Set A   states integers in [-4, 4]; W1 in {-1, 0, 1}, b1 integers in [-2, 2]; W2 in {-1, 0, 1} 2^-6, b2 integers 2^-6;
        W3 in {-1, 0, 1} 2^-10, b3 = pairwise distinct integers in [-8, 8] times 2^-10 (W3's quantum): a head bias row read from
        the wrong place of the image's bias record changes a word of the action.
Set B   the lo half of the input split and round-to-nearest-even ties: states integers in (-2^15, 2^15), W1 in {-1, 0, 1} 2^-8,
        b1 as set A.  z1 then has up to 23 significant bits, h1 = bf(relu(z1)) keeps a quantum of 2^-8 on its small values, and
        sum |h1| stays below 2^16 = 2^24 quanta.  Behind a dense layer 2 of set A's kind sum |h2| would be ~2^12 at a quantum
        of 2^-14: 2^26 quanta, not exact in every order.  So b2 = (-2 sigma + integers in [-2, 2]) 2^-6, sigma = the standard
        deviation of sum_k +-h1_k: about one unit in forty survives the ReLU, sum |h2| is ~2^7, and W3 in {-1, 0, 1} 2^-4 keeps
        z3 of order 1; b3 = pairwise distinct integers in [-8, 8] times 2^-4 (|b3| <= 1/2).  Hidden unit 0 of layer 1 reads state 0 alone (W1[0][0] = 2^-8, b1[0] = 0), and lanes 0 and 1 hold
        s_0 = 257 and 259: hi = 256 / 260 (ties to even, down and up), lo = +1 / -1, z1 = 257/256 and 259/256, h1 = 1 and
        1 + 2^-6 (ties again, down and up).
Set C   bf16-subnormal operands, on set A's data: state columns 0 and 1 are zero on every lane but the first three, which hold
        small integers times 2^-130 in column 0 (subnormal as float32 and as bf16, and exact in bf16: the lo part is zero) and
        2^-126, the smallest normal value, in column 1.  Only four hidden units of their own read these two columns, one
        weight each, +-2^100, bias 0: every product is exact and normal (k 2^-30 and 2^-26), every sum has one term.  Those
        units feed nothing (their rows of W2 are zero), so layers 2 and 3 are set A's kind and every other unit's sums are
        set A's integers.  set_c_ok() is its host assertion.
quanta_ok() is the host assertion that the data is what this says."""
import numpy as np

f32 = np.float32
SEEDS = {"cr": 11, "pg": 12, "ra": 13, "acr": 14, "apg": 15, "hvac": 16, "steel": 17, "supply": 18}


def _tri(rng, shape, scale):
    return (rng.integers(-1, 2, shape).astype(f32) * f32(scale)).astype(f32)


def _head_bias(rng, A, quantum):
    """A pairwise distinct integers of [-8, 8] times the head's weight quantum."""
    assert A <= 17
    return (rng.permutation(np.arange(-8, 9))[:A].astype(f32) * f32(quantum)).astype(f32)


def set_a(key, S, A, B):
    rng = np.random.default_rng(1000 + SEEDS[key])
    ws = [(_tri(rng, (S, 256), 1.0), rng.integers(-2, 3, 256).astype(f32)),
          (_tri(rng, (256, 256), 2.0 ** -6), (rng.integers(-8, 9, 256).astype(f32) * f32(2.0 ** -6)).astype(f32)),
          (_tri(rng, (256, A), 2.0 ** -10), np.zeros(A, f32))]
    states = rng.integers(-4, 5, (B, S)).astype(f32)
    ws[2] = (ws[2][0], _head_bias(rng, A, 2.0 ** -10))          # (drawn last: the weights and states are the ones b3 = 0 had)
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
    ws[2] = (ws[2][0], _head_bias(rng, A, 2.0 ** -4))
    return ws, states


C_UNITS = (0, 1, 2, 3)                     # hidden units of layer 1: +2^100 s_0, +2^100 s_1, -2^100 s_0, -2^100 s_1
C_COL0 = (5, -3, 7)                        # lanes 0, 1, 2: state column 0 in units of 2^-130


def set_c(key, S, A, B):
    """(weights, states, the dedicated hidden units)."""
    assert B >= len(C_COL0)
    ws, states = set_a(key, S, A, B)
    (W1, b1), (W2, b2), l3 = ws
    W1, b1, W2, states = W1.copy(), b1.copy(), W2.copy(), states.copy()
    W1[:2, :] = 0                              # no other unit reads state columns 0 and 1
    W1[:, list(C_UNITS)] = 0
    big = f32(2.0 ** 100)
    W1[0, 0], W1[1, 1], W1[0, 2], W1[1, 3] = big, big, -big, -big
    b1[list(C_UNITS)] = 0
    W2[list(C_UNITS), :] = 0                   # the dedicated units feed nothing
    states[:, :2] = 0
    for lane, k in enumerate(C_COL0):
        states[lane, 0] = f32(k) * f32(2.0 ** -130)
        states[lane, 1] = f32(2.0 ** -126)
    assert np.all(np.abs(states[:len(C_COL0), 0]) < f32(2.0 ** -126)) and np.all(states[:len(C_COL0), 0] != 0), "subnormal, not flushed on the host"
    return [(W1, b1), (W2, b2), l3], states, list(C_UNITS)


def set_c_ok(ref, ws, states, units):
    """Host assertion of set C: the dedicated units' h1 is the one exact, normal product (or zero behind the ReLU) and a bf16
    value; without columns 0 and 1 the data passes quanta_ok, and the dedicated units change nothing behind layer 1."""
    from neorl_industrial_gym_amd.policies import bf16_round, bf16_split, mlp_bf16_reference
    hi, lo = bf16_split(states)
    assert np.array_equal(hi[:, :2], states[:, :2]) and not lo[:, :2].any(), "columns 0 and 1 are bf16 values: no lo part"
    n = len(C_COL0)
    want = np.zeros((states.shape[0], 4))
    want[:n, 0] = np.maximum(np.array(C_COL0, dtype=np.float64), 0) * 2.0 ** -30
    want[:n, 2] = np.maximum(-np.array(C_COL0, dtype=np.float64), 0) * 2.0 ** -30
    want[:n, 1] = 2.0 ** -26
    assert np.array_equal(ref["h1"][:, units].astype(np.float64), want)
    assert np.array_equal(bf16_round(want.astype(f32)).astype(np.float64), want) and np.all((want == 0) | (want >= 2.0 ** -126))
    rest = states.copy()
    rest[:, :2] = 0
    ref0 = mlp_bf16_reference(ws, rest)
    spans = quanta_ok(ref0, ws, rest)
    others = [u for u in range(ref["h1"].shape[1]) if u not in units]
    assert np.array_equal(ref0["h1"][:, others], ref["h1"][:, others]) and not ref0["h1"][:, units].any()
    assert np.array_equal(ref0["h2"], ref["h2"]) and np.array_equal(ref0["z3"], ref["z3"])
    return spans


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
