"""not-gpu: the host side of the fused safe-action search ("nig-search-v1", include/nig.h): policies.search_candidates against
the oracle's Philox and the [-1, 1) word rule, the critic padding helper, MLPPolicy.from_agent(critic="risk"), and
get_safe_action on the CPU device."""
import types

import numpy as np
import pytest
import torch

f32 = np.float32
STREAM_POLICY, SEARCH_BLOCK0 = 0xC0000000, 0x100


@pytest.fixture(scope="module")
def pol():
    from neorl_industrial_gym_amd import policies
    return policies


def _oracle_candidates(oracle, seed, env_index, t, N, A):
    """The law as include/nig.h states it: word j & 3 of block 0x100 + 4 c + (j >> 2) of the policy stream."""
    out = np.zeros((N, A), dtype=f32)
    for c in range(N):
        for j in range(A):
            ctr = [env_index & 0xFFFFFFFF, env_index >> 32, t, STREAM_POLICY + SEARCH_BLOCK0 + 4 * c + (j >> 2)]
            w = oracle.philox([ctr], [[seed & 0xFFFFFFFF, seed >> 32]])[0, j & 3]
            out[c, j] = f32((int(w) >> 8) * 2.0 ** -23 - 1.0)            # (exact in float64, and a float32: see the test's docstring)
    return out


@pytest.mark.parametrize("A", [3, 7, 8])
@pytest.mark.parametrize("N", [1, 5, 128])
def test_search_candidates_are_the_oracles_philox_words(pol, oracle, A, N):
    """(m * 2^-23 - 1 with m < 2^24 is a multiple of 2^-23 below 1 in magnitude: exact in float32 and float64 alike, so the
    float64 form above is the kernel's fmaf.)"""
    for seed, gi, t in [(0x5EED, 0, 1), (0x5EED, 699, 8), (0xDEADBEEF12345678, (1 << 32) + 5, 0xFFFFFFF0), (1, (7 << 32) | 0xFFFFFFFF, 77)]:
        got = pol.search_candidates(seed, gi, t, N, A)
        assert got.dtype == f32 and got.shape == (N, A)
        want = _oracle_candidates(oracle, seed, gi, t, N, A)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (seed, gi, t)
        assert (got >= -1).all() and (got < 1).all()
    # the key matters in every part: env_hi, t and the seed's high word each change the draws
    base = pol.search_candidates(5, 9, 3, 4, A)
    for other in [pol.search_candidates(5, 9 + (1 << 32), 3, 4, A), pol.search_candidates(5, 9, 4, 4, A), pol.search_candidates(5 + (1 << 32), 9, 3, 4, A)]:
        assert not np.array_equal(base, other)
    # a longer search extends a shorter one
    assert np.array_equal(pol.search_candidates(5, 9, 3, 9, A)[:4], base)


def test_philox_known_answer(pol, oracle):
    rng = np.random.default_rng(0)
    ctr = rng.integers(0, 1 << 32, (257, 4), dtype=np.uint64).astype(np.uint32)
    key = rng.integers(0, 1 << 32, (257, 2), dtype=np.uint64).astype(np.uint32)
    ctr[0], key[0] = 0xFFFFFFFF, 0xFFFFFFFF
    assert np.array_equal(pol.philox4x32_7(ctr, key), oracle.philox(ctr, key))


def _critic(D, h, seed):
    rng = np.random.default_rng(seed)
    return [(rng.normal(0, 1.0 / np.sqrt(D), (D, h)).astype(f32), rng.normal(0, 0.05, h).astype(f32)),
            (rng.normal(0, 1.0 / np.sqrt(h), (h, h)).astype(f32), rng.normal(0, 0.05, h).astype(f32)),
            (rng.normal(0, 1.0 / 2, (h, 1)).astype(f32), rng.normal(0, 0.1, 1).astype(f32))]


def _actor(S, A, h, seed):
    rng = np.random.default_rng(seed)
    return [(rng.normal(0, 1.0 / np.sqrt(S), (S, h)).astype(f32), rng.normal(0, 0.05, h).astype(f32)),
            (rng.normal(0, 1.0 / np.sqrt(h), (h, h)).astype(f32), rng.normal(0, 0.05, h).astype(f32)),
            (rng.normal(0, 1.0 / 8, (h, A)).astype(f32), rng.normal(0, 0.1, A).astype(f32))]


def _net64(layers, x):
    z = np.asarray(x, dtype=np.float64)
    for i, (W, b) in enumerate(layers):
        z = z @ np.asarray(W, dtype=np.float64) + np.asarray(b, dtype=np.float64).reshape(-1)
        if i + 1 < len(layers):
            z = np.maximum(z, 0)
    return 1.0 / (1.0 + np.exp(-z[..., 0]))


def test_pad_critic_shapes_zeros_and_value(pol):
    D, h = 15, 128
    cw = _critic(D, h, 3)
    pw = pol.pad_critic(cw)
    assert [(W.shape, b.shape) for W, b in pw] == [((D, 256), (256,)), ((256, 256), (256,)), ((256, 1), (1,))]
    assert all(W.dtype == f32 and b.dtype == f32 for W, b in pw)
    (P1, p1), (P2, p2), (P3, p3) = pw
    assert np.array_equal(P1[:, :h], cw[0][0]) and not P1[:, h:].any() and np.array_equal(p1[:h], cw[0][1]) and not p1[h:].any()
    assert np.array_equal(P2[:h, :h], cw[1][0]) and not P2[h:].any() and not P2[:, h:].any()
    assert np.array_equal(p2[:h], cw[1][1]) and not p2[h:].any()
    assert np.array_equal(P3[:h], cw[2][0]) and not P3[h:].any() and np.array_equal(p3, cw[2][1])
    x = np.random.default_rng(4).normal(0, 1, (64, D))
    assert np.abs(_net64(pw, x) - _net64(cw, x)).max() <= 1e-6
    # the float32 torch form of the padded network against the float64 unpadded one
    m = pol.MLPPolicy(_actor(12, 3, 256, 1), device="cpu", safety_weights=pw)
    xt = torch.as_tensor(x.astype(f32))
    p = m.safety_probs_device(xt[:, :12], xt[:, 12:]).numpy()
    assert np.abs(p - _net64(cw, x.astype(f32))).max() <= 1e-6
    # a 256-wide critic passes through; a head given as a vector is reshaped; a wider or ragged one is refused
    same = pol.pad_critic(_critic(D, 256, 5))
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(same, _critic(D, 256, 5)))
    vec = [cw[0], cw[1], (cw[2][0][:, 0], cw[2][1])]
    assert np.array_equal(pol.pad_critic(vec)[2][0], P3)
    with pytest.raises(ValueError):
        pol.pad_critic(_critic(D, 257, 6))
    with pytest.raises(ValueError):
        pol.pad_critic([cw[0], (cw[1][0][:, :100], cw[1][1]), cw[2]])


def _flax_dense(layers):
    return {"params": {"MLP_0": {f"Dense_{i}": {"kernel": W, "bias": b} for i, (W, b) in enumerate(layers)}}}


def _flax_risk(layers):
    return {"params": {n: {"kernel": W, "bias": b} for n, (W, b) in zip(("layers_0", "layers_1", "risk_head"), layers)}}


def test_from_agent_reads_the_risk_estimator(pol):
    S, A = 12, 3
    ws, safety, risk = _actor(S, A, 256, 1), _critic(S + A, 256, 2), _critic(S + A, 128, 3)
    agent = types.SimpleNamespace(state={"actor": types.SimpleNamespace(params=_flax_dense(ws)),
                                         "safety": types.SimpleNamespace(params=_flax_dense(safety))},
                                  risk_state=types.SimpleNamespace(params=_flax_risk(risk)),
                                  constraint_threshold=0.3, uncertainty_threshold=0.07, is_trained=True)
    r = pol.MLPPolicy.from_agent(agent, device="cpu", critic="risk")
    assert r.constraint_threshold == 0.07
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(r.safety_weights, risk))
    assert all(np.array_equal(a[0], b[0]) for a, b in zip(r.weights, ws))
    # the default is unchanged on an agent that has both
    d = pol.MLPPolicy.from_agent(agent, device="cpu")
    assert d.constraint_threshold == 0.3
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(d.safety_weights, safety))
    d2 = pol.MLPPolicy.from_agent(agent, device="cpu", critic="safety")
    assert d2.constraint_threshold == 0.3 and np.array_equal(d2.safety_weights[0][0], safety[0][0])
    # the searching policy of a 128-wide risk estimator is fusable and hands the kernel the padded critic
    sp = r.searching(7)
    assert sp.fusable and sp.n_candidates == 7 and sp.threshold == 0.07
    assert [W.shape for W, _ in sp.safety_weights] == [(S + A, 256), (256, 256), (256, 1)]
    assert r.searching(7, 0.0).threshold == 0.0                       # 0.0 is a threshold here, not "the default"
    with pytest.raises(ValueError):
        r.searching(0)
    with pytest.raises(ValueError):
        r.searching(129)
    del agent.risk_state
    with pytest.raises(ValueError):
        pol.MLPPolicy.from_agent(agent, device="cpu", critic="risk")
    with pytest.raises(ValueError):
        pol.MLPPolicy.from_agent(agent, device="cpu", critic="nope")


def test_get_safe_action_on_the_cpu_device(pol):
    S, A, n, N = 12, 3, 40, 9
    m = pol.MLPPolicy(_actor(S, A, 256, 1), device="cpu", safety_weights=_critic(S + A, 128, 2))
    obs = np.random.default_rng(5).normal(0, 1, (n, S)).astype(f32)
    # a threshold above every p: the preferred action (default: the actor's) comes back untouched
    a, info = m.get_safe_action(obs, n_candidates=N, safety_threshold=2.0)
    assert np.array_equal(a, m.predict(obs)) and not info["corrected"].any() and (info["choice"] == -1).all()
    assert np.array_equal(info["risk"], m.safety_probs_device(torch.as_tensor(obs), torch.as_tensor(a)).numpy())
    pref = np.random.default_rng(6).uniform(-1, 1, (n, A)).astype(f32)
    a, info = m.get_safe_action(obs, pref, n_candidates=N, safety_threshold=2.0)
    assert np.array_equal(a, pref) and not info["corrected"].any()
    # threshold 0: every row is corrected to the first of least risk among its own candidates (recomputed from the same seed)
    g = torch.Generator().manual_seed(123)
    a, info = m.get_safe_action(obs, n_candidates=N, safety_threshold=0.0, generator=g)
    u = torch.rand((n, N, A), generator=torch.Generator().manual_seed(123), dtype=torch.float32) * 2.0 - 1.0
    ot = torch.as_tensor(obs)
    pc = torch.stack([m.safety_probs_device(ot, u[:, c]) for c in range(N)], dim=1).numpy()
    best = pc.argmin(axis=1)                                         # NumPy: the first minimum
    assert info["corrected"].all() and np.array_equal(info["choice"], best)
    assert np.array_equal(info["risk"], pc[np.arange(n), best]) and np.array_equal(info["risk"], pc.min(axis=1))
    assert np.array_equal(a, u.numpy()[np.arange(n), best])
    # a single observation: the reference's scalars
    a1, i1 = m.get_safe_action(obs[0], n_candidates=N, safety_threshold=0.0, generator=torch.Generator().manual_seed(123))
    assert a1.shape == (A,) and isinstance(i1["risk"], float) and i1["corrected"] is True and isinstance(i1["choice"], int)
    # the searching policy acts with it
    sp = m.searching(N, 2.0)
    assert np.array_equal(sp.predict(obs), m.predict(obs))
