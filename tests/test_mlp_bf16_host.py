"""not-gpu: the host side of "nig-mlp-bf16-v1" (include/nig.h) -- the library's rounding against the NumPy restatement word for
word, the input split, the float64 reference against plain integer arithmetic on the exact-integer case, and the routing of
a Bf16MLPPolicy in utils._install_agent."""
import ctypes as C

import numpy as np
import pytest

import closed_loop_matrix as M
import mlp_bf16_cases as K

f32 = np.float32


def _words(x):
    return (np.ascontiguousarray(x, dtype=f32).view(np.uint32) >> np.uint32(16)).astype(np.uint16)


def _lib_round(x):
    import neorl_industrial_gym_amd as ni
    x = np.ascontiguousarray(x, dtype=f32)
    out = np.full(x.size, 0xDEAD, dtype=np.uint16)
    assert ni._lib.lib().nig_bf16_from_f32(x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), x.size) == 0
    return out.reshape(x.shape)


def test_library_rounding_is_the_numpy_rounding_word_for_word():
    from neorl_industrial_gym_amd.policies import bf16_round
    bits = lambda *w: np.array(w, dtype=np.uint32).view(f32)
    # ties: an even kept mantissa rounds down, an odd one up, on both signs; just below and just above a tie
    ties = bits(0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F807FFF, 0x3F808001, 0x3F81FFFF)
    want = np.array([0x3F80, 0x3F82, 0xBF80, 0xBF82, 0x3F80, 0x3F81, 0x3F82], dtype=np.uint16)
    assert np.array_equal(_lib_round(ties), want) and np.array_equal(_words(bf16_round(ties)), want)
    # the largest finite float rounds to inf; subnormals (float32's, and those of bf16's own range); zeros; infinities
    edge = bits(0x7F7FFFFF, 0xFF7FFFFF, 0x00000001, 0x00008000, 0x00008001, 0x00018000, 0x007FFFFF, 0x80000001, 0x00000000, 0x80000000,
                0x7F800000, 0xFF800000)
    want = np.array([0x7F80, 0xFF80, 0x0000, 0x0000, 0x0001, 0x0002, 0x0080, 0x8000, 0x0000, 0x8000, 0x7F80, 0xFF80], dtype=np.uint16)
    assert np.array_equal(_lib_round(edge), want) and np.array_equal(_words(bf16_round(edge)), want)
    # a NaN stays a NaN (quiet or signalling, either sign, payload in the low half alone)
    nans = bits(0x7FC00000, 0xFFC00000, 0x7F800001, 0x7F80FFFF, 0xFFA00000)
    for got in (_lib_round(nans), _words(bf16_round(nans))):
        assert np.all((got & 0x7F80) == 0x7F80) and np.all((got & 0x007F) != 0), got
    assert np.array_equal(_lib_round(nans), _words(bf16_round(nans)))
    assert np.all(np.isnan(bf16_round(nans)))
    # 10^5 random words
    w = np.random.default_rng(5).integers(0, 2 ** 32, 100000, dtype=np.uint64).astype(np.uint32).view(f32)
    with np.errstate(all="ignore"):
        assert np.array_equal(_lib_round(w), _words(bf16_round(w)))
    # the rounded value is a bfloat16: its low half is zero
    with np.errstate(all="ignore"):
        assert np.all((bf16_round(w).view(np.uint32) & np.uint32(0xFFFF)) == 0)


def test_the_input_split_keeps_sixteen_bits():
    from neorl_industrial_gym_amd.policies import bf16_round, bf16_split
    ints = np.arange(-2 ** 16 + 1, 2 ** 16, dtype=np.int64).astype(f32)
    hi, lo = bf16_split(ints)
    assert np.array_equal(hi.astype(np.float64) + lo.astype(np.float64), ints.astype(np.float64))
    assert np.array_equal(hi, bf16_round(hi)) and np.array_equal(lo, bf16_round(lo)) and int((lo != 0).sum()) > 2 ** 16
    rng = np.random.default_rng(6)
    x = (rng.standard_normal(200000) * np.exp(rng.uniform(-20, 20, 200000))).astype(f32)
    hi, lo = bf16_split(x)
    err = np.abs(x.astype(np.float64) - hi.astype(np.float64) - lo.astype(np.float64))
    assert np.all(err <= 2.0 ** -16 * np.abs(x.astype(np.float64)))
    big = np.array([3.4e38, -3.4e38, np.inf, -np.inf, 1.0], dtype=f32)
    hi, lo = bf16_split(big)
    assert np.all(np.isinf(hi[:4])) and np.all(lo[:4] == 0) and hi[4] == 1 and lo[4] == 0


@pytest.mark.parametrize("key,name", M.MFMA_ENVS)
def test_the_reference_is_integer_arithmetic_on_the_integer_case(key, name):
    """mlp_bf16_reference on set A equals a restatement with no floating point in it, and the data of both sets is what
    mlp_bf16_cases says: exact in float32 in any order, with ties and nonzero lo parts in set B."""
    import neorl_industrial_gym_amd as ni
    from neorl_industrial_gym_amd.policies import mlp_bf16_reference
    sp = ni._lib.env_spec(ni.batched.ENV_IDS[name])
    S, A = sp.state_dim, sp.action_dim
    for B in (M.B_BIG, M.B_SMALL):
        ws, st = K.set_a(key, S, A, B)
        ref = mlp_bf16_reference(ws, st)
        K.quanta_ok(ref, ws, st)
        h1, h2, z3 = K.int_reference(ws, st)
        assert np.array_equal(_words(ref["h1"]), _words(h1)) and np.array_equal(_words(ref["h2"]), _words(h2))
        assert np.array_equal(ref["z3"], z3) and np.array_equal(ref["action"], np.tanh(z3))
        assert ref["z1"].shape == ref["abs1"].shape == (B, 256) and ref["abs3"].shape == (B, A)
        assert int((h2 > 0).sum()) > 50 * B and len(np.unique(z3, axis=0)) == B
        ws, st = K.set_b(key, S, A, B)
        ref = mlp_bf16_reference(ws, st)
        K.quanta_ok(ref, ws, st)
        ties, lo = K.ties_and_lo(ref, st)
        assert ties >= 1 and lo >= 1
        assert _words(ref["h1"][0, :1])[0] == 0x3F80 and _words(ref["h1"][1, :1])[0] == 0x3F82, "the crafted ties, down and up"
        assert int((ref["h2"] > 0).sum()) >= B and np.max(np.abs(ref["z3"])) < 64
        # the head bias of both sets: nonzero somewhere in every pair of rows, pairwise distinct, integers in [-8, 8] of W3's
        # quantum; and z3 stays of order 1, so that a bias row moved to another row shows in the action (tanh is not saturated)
        for (wsx, q3), z3x in (((K.set_a(key, S, A, B)[0], 2.0 ** -10), z3), ((ws, 2.0 ** -4), ref["z3"])):
            b3 = wsx[2][1].astype(np.float64) / q3
            assert len(set(b3.tolist())) == A and np.array_equal(b3, np.round(b3)) and np.max(np.abs(b3)) <= 8 and np.count_nonzero(b3) >= A - 1
            assert np.median(np.abs(z3x)) < 4
            if B == M.B_BIG:
                assert np.all((np.abs(z3x) < 4).mean(axis=0) > 0.5), "every head row is unsaturated on most lanes"
    # h1 / h2 given: the layers behind them start from the given activations
    ref2 = mlp_bf16_reference(ws, st, h1=np.zeros_like(ref["h1"]))
    assert np.array_equal(ref2["z1"], ref["z1"]) and np.array_equal(ref2["z2"], np.broadcast_to(ws[1][1].astype(np.float64), ref["z2"].shape))


class _Env:
    """What utils._install_agent reads of an env, recording what it installs."""
    def __init__(self, S, A, has_limits=False):
        self.state_dim, self.action_dim, self.has_limits, self.device, self.installed = S, A, has_limits, "cpu", []

    def set_mlp_policy(self, w):
        self.installed.append("f32")

    def set_mlp_policy_bf16(self, w):
        self.installed.append("bf16")

    def rollout_mlp(self, *a, **k):
        return "rollout_mlp"

    def rollout_mlp_bf16(self, *a, **k):
        return "rollout_mlp_bf16"

    def rollout_mlp_limited(self, *a, **k):
        return "rollout_mlp_limited"


def test_install_agent_routes_a_bf16_policy_to_the_bf16_kernel():
    import torch
    import neorl_industrial_gym_amd as ni
    from neorl_industrial_gym_amd.utils import _install_agent
    S, A = 12, 3
    parent = ni.MLPPolicy(M.random_actor(S, A, 3), device="cpu")
    pol = parent.bf16()
    assert isinstance(pol, ni.Bf16MLPPolicy) and pol.is_trained and pol.precision == "bf16" and pol.fusable == parent.fusable is True
    assert pol.weights is parent.weights
    env = _Env(S, A)
    agent, rollout, disturbed = _install_agent(pol, env)
    assert agent is pol and disturbed is None and env.installed == ["bf16"] and rollout() == "rollout_mlp_bf16"
    # the float32 parent still takes the float32 kernel
    env = _Env(S, A)
    _, rollout, _ = _install_agent(parent, env)
    assert env.installed == ["f32"] and rollout() == "rollout_mlp"
    # an odd state dim (no MFMA actor), added constraints, injected draws: the host loop through predict_device, nothing installed
    for env, plain in ((_Env(15, A), True), (_Env(S, A, has_limits=True), True), (_Env(S, A), False)):
        p = ni.MLPPolicy(M.random_actor(env.state_dim, A, 3), device="cpu").bf16()
        _, rollout, disturbed = _install_agent(p, env, plain)
        assert rollout is None and disturbed is None and env.installed == []
    # a policy of another hidden width is not fusable: the host loop
    rng = np.random.default_rng(0)
    odd = ni.MLPPolicy([(rng.normal(size=(S, 64)).astype(f32), np.zeros(64, f32)), (rng.normal(size=(64, 64)).astype(f32), np.zeros(64, f32)),
                        (rng.normal(size=(64, A)).astype(f32), np.zeros(A, f32))], device="cpu").bf16()
    env = _Env(S, A)
    assert not odd.fusable and _install_agent(odd, env)[1] is None and env.installed == []
    # the torch emulation is the law up to accumulation order: against the float64 reference on real weights
    from neorl_industrial_gym_amd.policies import mlp_bf16_reference
    obs = (rng.normal(size=(64, S)) * 300).astype(f32)
    ref = mlp_bf16_reference(pol.weights, obs)
    got = pol.predict_device(torch.from_numpy(obs)).numpy()
    assert got.shape == (64, A) and np.max(np.abs(got - ref["action"])) < 1e-2
    assert np.array_equal(pol.predict(obs[0]), got[0])
