"""not-gpu: the host side of the fused safety-ensemble gate ("nig-gate-v1", include/nig.h): policies.pad_safety_member,
SafetyEnsemblePolicy.from_agent on Flax-shaped trees, the host get_safe_action on the CPU device against a literal NumPy
transcription of the reference's SafeEnsembleAgent (agents/safety_critical.py:460-532), the Python-side refusals, and the
gfx950 build of the new translation units."""
import ctypes as C
import glob
import os
import types

import numpy as np
import pytest
import torch

f32 = np.float32


@pytest.fixture(scope="module")
def pol():
    from neorl_industrial_gym_amd import policies
    return policies


def _member(D, h, n_out, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    return [(rng.normal(0, 1.0 / np.sqrt(D), (D, h)).astype(f32), rng.normal(0, 0.05, h).astype(f32)),
            (rng.normal(0, 1.0 / np.sqrt(h), (h, h)).astype(f32), rng.normal(0, 0.05, h).astype(f32)),
            (rng.normal(0, scale / 2, (h, n_out)).astype(f32), rng.normal(0, 0.1, n_out).astype(f32))]


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
    return z


@pytest.mark.parametrize("n_out", [1, 3, 4])
def test_pad_safety_member_shapes_zeros_and_value(pol, n_out):
    D, h = 15, 128
    mw = _member(D, h, n_out, 3)
    pw = pol.pad_safety_member(mw)
    assert [(W.shape, b.shape) for W, b in pw] == [((D, 256), (256,)), ((256, 256), (256,)), ((256, n_out), (n_out,))]
    assert all(W.dtype == f32 and b.dtype == f32 for W, b in pw)
    (P1, p1), (P2, p2), (P3, p3) = pw
    assert np.array_equal(P1[:, :h], mw[0][0]) and not P1[:, h:].any() and np.array_equal(p1[:h], mw[0][1]) and not p1[h:].any()
    assert np.array_equal(P2[:h, :h], mw[1][0]) and not P2[h:].any() and not P2[:, h:].any()
    assert np.array_equal(p2[:h], mw[1][1]) and not p2[h:].any()
    assert np.array_equal(P3[:h], mw[2][0]) and not P3[h:].any() and np.array_equal(p3, mw[2][1])
    x = np.random.default_rng(4).normal(0, 1, (64, D))
    assert np.abs(_net64(pw, x) - _net64(mw, x)).max() <= 1e-12      # (added terms are exact zeros; float64 sums of the same terms)
    # the float32 torch form of the padded member against the float64 unpadded one
    sp = pol.SafetyEnsemblePolicy(_actor(12, 3, 256, 1), [pw], device="cpu")
    xt = torch.as_tensor(x.astype(f32))
    z = sp.member_logits_device(xt[:, :12], xt[:, 12:]).numpy()
    assert z.shape == (1, 64, n_out)
    z64 = _net64(mw, x.astype(f32))
    assert np.abs(z[0] - z64).max() <= 1e-5 * max(1.0, np.abs(z64).max())
    # a 256-wide member passes through; pad_critic stays a one-column helper
    same = pol.pad_safety_member(_member(D, 256, n_out, 5))
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(same, _member(D, 256, n_out, 5)))
    if n_out > 1:
        with pytest.raises(ValueError):
            pol.pad_critic(mw)


def test_pad_safety_member_refusals(pol):
    D = 15
    with pytest.raises(ValueError):
        pol.pad_safety_member(_member(D, 257, 2, 6))
    with pytest.raises(ValueError):
        pol.pad_safety_member(_member(D, 128, 5, 6))                  # heads of more than four rows
    mw = _member(D, 128, 2, 6)
    with pytest.raises(ValueError):
        pol.pad_safety_member([mw[0], (mw[1][0][:, :100], mw[1][1]), mw[2]])
    with pytest.raises(ValueError):
        pol.pad_safety_member(mw[:2])
    vec = _member(D, 128, 1, 7)
    assert pol.pad_safety_member([vec[0], vec[1], (vec[2][0][:, 0], vec[2][1])])[2][0].shape == (256, 1)


def _flax_dense(layers):
    return {"params": {"MLP_0": {f"Dense_{i}": {"kernel": W, "bias": b} for i, (W, b) in enumerate(layers)}}}


def _flax_member(layers):
    return {"params": {n: {"kernel": W, "bias": b} for n, (W, b) in zip(("layers_0", "layers_1", "safety_head"), layers)}}


def test_from_agent_reads_the_ensemble_states(pol):
    S, A, K, n_out = 12, 3, 5, 3
    ws = _actor(S, A, 256, 1)
    ms = [_member(S + A, 128, n_out, 10 + i) for i in range(K)]
    actor_agent = types.SimpleNamespace(state={"actor": types.SimpleNamespace(params=_flax_dense(ws))}, is_trained=True)
    safe_agent = types.SimpleNamespace(ensemble_states=[types.SimpleNamespace(params=_flax_member(m)) for m in ms],
                                       temperature=1.5, uncertainty_threshold=0.07)
    sp = pol.SafetyEnsemblePolicy.from_agent(actor_agent, safe_agent, device="cpu")
    assert sp.temperature == 1.5 and sp.threshold == 0.07 and sp.max_uncertainty == 0.2 and sp.n_outputs == n_out
    assert len(sp.members) == K
    for got, want in zip(sp.members, ms):
        assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(got, want))
    assert all(np.array_equal(a[0], b[0]) for a, b in zip(sp.weights, ws))
    assert sp.fusable and hasattr(sp, "install")
    # what install() hands the env: the actor as it is, the members padded to 256
    calls = {}
    env = types.SimpleNamespace(set_mlp_policy=lambda w: calls.setdefault("actor", w),
                                set_mlp_safety_ensemble=lambda m, T, thr, umax: calls.setdefault("gate", (m, T, thr, umax)))
    sp.install(env)
    assert calls["actor"] is sp.weights
    m, T, thr, umax = calls["gate"]
    assert (T, thr, umax) == (1.5, 0.07, 0.2) and len(m) == K
    assert all([W.shape for W, _ in x] == [(S + A, 256), (256, 256), (256, n_out)] for x in m)
    # a tree without the named layers is refused
    bad = types.SimpleNamespace(ensemble_states=[types.SimpleNamespace(params=_flax_dense(ms[0]))], temperature=1.0, uncertainty_threshold=0.1)
    with pytest.raises(ValueError):
        pol.SafetyEnsemblePolicy.from_agent(actor_agent, bad, device="cpu")


def _reference_get_safe_action(members, T, thr, state, action):
    """agents/safety_critical.py:460-532 transcribed literally for ONE state (NumPy float32 for jnp's default dtype):
    compute_safety_violation_probability, then get_safe_action with max_acceptable_uncertainty = 0.2."""
    def apply_fn(m, s, a):
        x = np.concatenate([s, a], axis=-1)
        for W, b in m[:-1]:
            x = np.maximum(x @ W + b, f32(0))
        return x @ m[-1][0] + m[-1][1]
    with np.errstate(invalid="ignore", over="ignore"):
        predictions = np.array([apply_fn(m, state, action) for m in members])
        mean_pred = np.mean(predictions, axis=0)
        std_pred = np.std(predictions, axis=0)
        calibrated_pred = mean_pred / f32(T)
        base_prob = (1.0 / (1.0 + np.exp(-calibrated_pred.astype(np.float64)))).astype(f32)
        uncertainty_penalty = np.minimum(std_pred, f32(1.0))
        final_prob = base_prob + f32(0.5) * uncertainty_penalty
        violation_prob = np.clip(final_prob, f32(0.0), f32(1.0))
        uncertainty = np.std(predictions, axis=0)
        is_safe = np.all(violation_prob < thr)
        is_certain = np.all(uncertainty < 0.2)
    if is_safe and is_certain:
        return action, {"violation_prob": violation_prob, "uncertainty": uncertainty, "decision": "accept"}
    return np.zeros_like(action), {"violation_prob": violation_prob, "uncertainty": uncertainty, "decision": "reject_conservative"}


def _close(got, want):
    """the project's parity bar: 1e-5 relative with an absolute floor of 1e-6; NaN matches NaN"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and (np.abs(got - want)[~nan] <= np.maximum(1e-6, 1e-5 * np.abs(want[~nan]))).all()


def test_get_safe_action_on_the_cpu_device_against_the_reference(pol):
    """Accept, reject for probability, reject for spread, and the NaN case, each asserted to occur.  Rows whose p or sd lies
    within the parity bar of its limit may decide either way between two arithmetics; they are counted and must be few."""
    S, A, n, K, n_out = 12, 3, 300, 5, 3
    ws = _actor(S, A, 256, 1)
    base = _member(S + A, 128, n_out, 20, scale=0.4)
    rng = np.random.default_rng(21)
    # members = a common network with perturbed heads: spreads of the order of the limit, on both sides of it
    ms = [[base[0], base[1], ((base[2][0] + rng.normal(0, 0.035, base[2][0].shape)).astype(f32), (base[2][1] - f32(2.5)).astype(f32))] for _ in range(K)]
    obs = rng.normal(0, 1, (n, S)).astype(f32)
    seen = set()
    for T, thr in [(1.0, 0.25), (1.5, 0.3)]:
        sp = pol.SafetyEnsemblePolicy(ws, ms, temperature=T, threshold=thr, max_uncertainty=0.2, device="cpu")
        raw = sp.actor.predict(obs)
        a, info = sp.get_safe_action(obs)
        assert a.shape == (n, A) and info["violation_prob"].shape == (n, n_out) and info["uncertainty"].shape == (n, n_out)
        near = 0
        for i in range(n):
            ra, ri = _reference_get_safe_action(ms, T, thr, obs[i], raw[i])
            assert _close(info["violation_prob"][i], ri["violation_prob"]) and _close(info["uncertainty"][i], ri["uncertainty"]), i
            edge = (np.abs(ri["violation_prob"] - thr) <= 1e-5).any() or (np.abs(ri["uncertainty"] - 0.2) <= 1e-5).any()
            near += int(edge)
            if not edge:
                assert info["decision"][i] == ri["decision"] and np.array_equal(a[i], ra), i
                safe, certain = (ri["violation_prob"] < thr).all(), (ri["uncertainty"] < 0.2).all()
                seen.add("accept" if safe and certain else "probability" if certain else "spread" if safe else "both")
        assert near <= n // 50
        assert np.array_equal(sp.predict(obs), a)
    assert {"accept", "probability", "spread"} <= seen, seen
    # a preferred action is judged instead of the actor's; a single observation gives the reference's form
    pref = rng.uniform(-1, 1, (n, A)).astype(f32)
    sp = pol.SafetyEnsemblePolicy(ws, ms, threshold=2.0, max_uncertainty=10.0, device="cpu")
    a, info = sp.get_safe_action(obs, pref)
    assert np.array_equal(a, pref) and (info["decision"] == "accept").all()
    a1, i1 = sp.get_safe_action(obs[0], pref[0])
    assert a1.shape == (A,) and i1["decision"] == "accept" and i1["violation_prob"].shape == (n_out,)
    p, sd = sp.violation_probs(obs, pref)
    assert np.array_equal(p, info["violation_prob"]) and np.array_equal(sd, info["uncertainty"])
    # the NaN case: one member's head bias -inf -> std NaN, NaN < 0.2 false: rejected, as the reference
    inf = [m if j else [m[0], m[1], (m[2][0], np.array([-np.inf] + [0.0] * (n_out - 1), dtype=f32))] for j, m in enumerate(ms)]
    sp = pol.SafetyEnsemblePolicy(ws, inf, threshold=2.0, max_uncertainty=10.0, device="cpu")
    a, info = sp.get_safe_action(obs[:20])
    assert not a.any() and (info["decision"] == "reject_conservative").all() and np.isnan(info["uncertainty"][:, 0]).all()
    for i in range(20):
        ra, ri = _reference_get_safe_action(inf, 1.0, 2.0, obs[i], sp.actor.predict(obs[i]))
        assert ri["decision"] == "reject_conservative" and not ra.any() and np.isnan(ri["uncertainty"][0])
        assert _close(info["uncertainty"][i], ri["uncertainty"]) and _close(info["violation_prob"][i], ri["violation_prob"])
    # identical members and one member: the spread is exactly 0
    for members in ([ms[0]] * 5, [ms[0]]):
        sp = pol.SafetyEnsemblePolicy(ws, members, device="cpu")
        assert not sp.violation_probs(obs, pref)[1].any()


def test_python_side_refusals(pol):
    S, A = 12, 3
    ws, m3, m2 = _actor(S, A, 256, 1), _member(S + A, 128, 3, 2), _member(S + A, 128, 2, 3)
    with pytest.raises(RuntimeError):
        pol.SafetyEnsemblePolicy(ws, [], device="cpu")
    with pytest.raises(ValueError):
        pol.SafetyEnsemblePolicy(ws, [m3, m2], device="cpu")              # heads of different widths
    with pytest.raises(ValueError):
        pol.SafetyEnsemblePolicy(ws, [_member(S + A + 1, 128, 3, 4)], device="cpu")
    for T in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError):
            pol.SafetyEnsemblePolicy(ws, [m3], temperature=T, device="cpu")
    with pytest.raises(ValueError):
        pol.SafetyEnsemblePolicy(ws, [m3], threshold=np.nan, device="cpu")
    with pytest.raises(ValueError):
        pol.SafetyEnsemblePolicy(ws, [m3], max_uncertainty=np.nan, device="cpu")
    # not fusable (the host loop keeps it): too many members, a head of five rows, a wide member, a narrow actor
    assert pol.SafetyEnsemblePolicy(ws, [m3] * 8, device="cpu").fusable
    assert not pol.SafetyEnsemblePolicy(ws, [m3] * 9, device="cpu").fusable
    assert not pol.SafetyEnsemblePolicy(ws, [_member(S + A, 128, 5, 5)], device="cpu").fusable
    assert not pol.SafetyEnsemblePolicy(ws, [_member(S + A, 300, 3, 5)], device="cpu").fusable
    assert not pol.SafetyEnsemblePolicy(_actor(S, A, 128, 1), [m3], device="cpu").fusable
    import neorl_industrial_gym_amd as ni
    assert ni.SafetyEnsemblePolicy is pol.SafetyEnsemblePolicy and "SafetyEnsemblePolicy" in ni.__all__


def test_the_library_links_the_gated_translation_units():
    """One gated_<key>.hip per environment, built for gfx950 into libnig.so with the two entry points exported and bound."""
    from neorl_industrial_gym_amd import _build, _lib
    tus = sorted(os.path.basename(p) for p in glob.glob(os.path.join(_build.CSRC, "gated_*.hip")))
    assert tus == sorted(os.path.basename(p).replace("search_", "gated_") for p in glob.glob(os.path.join(_build.CSRC, "search_*.hip")))
    assert len(tus) == 9 and all(os.path.join(_build.CSRC, t) in _build.sources() for t in tus)
    assert not _build.stale()
    L = C.CDLL(_build.LIB)
    for sym in ("nig_set_mlp_safety_ensemble", "nig_rollout_mlp_gated"):
        assert hasattr(L, sym) and sym in _lib.PROTOTYPES
    assert len(_lib.PROTOTYPES["nig_rollout_mlp_gated"][1]) == 16 and len(_lib.PROTOTYPES["nig_set_mlp_safety_ensemble"][1]) == 14
    with open(_build.LIB, "rb") as f:
        blob = f.read()
    for key in ("15ChemicalReactor", "9PowerGrid", "13RobotAssembly"):
        assert b"rollout_mlp_gated_kernelINS_" + key.encode() in blob, key
