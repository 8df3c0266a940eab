"""not-gpu: EnsemblePolicy on the host against what the reference's EnsembleAgent computed (tests/golden/ensemble_laws.npz,
recorded by tests/gen_ensemble_golden.py from agents/ensemble.py executed in place): the action bit for bit with its dtype, the
uncertainty to the parity bar, the high-uncertainty mask, and EnsemblePolicy.from_agent on a reference-shaped stand-in.

Bounds.  Action: bit equality (the library's sequential order IS np.average's / np.mean's for these shapes).  Uncertainty: 1e-5
relative with a 1e-6 absolute floor -- the project's parity bar; the library documents the member-0-shifted single-pass variance
(include/nig.h), not NumPy's two-pass one, so no bit equality is claimed for it.  Mask: exact on every row whose recorded
uncertainty lies further than 1e-5 relative from the threshold, and at least 90 % of every case's rows must be such rows."""
import os
import types

import numpy as np
import pytest

from conftest import ROOT

DIMS, MEMBERS, METHODS = (3, 7, 8, 10, 16), (1, 2, 3, 5, 8), ("mean", "weighted", "voting")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "ensemble_laws.npz"))


def _policy(gold, A, K, method):
    """EnsemblePolicy.from_agent over stand-in members that answer with the recorded member actions (the law under test is the
    ensemble's, not the members'): the agent list has the recorded untrained members in it, the weight vector is the agent's."""
    import neorl_industrial_gym_amd as ni
    tag = f"A{A}_K{K}"
    preds, trained = gold[tag + "_preds"], gold[tag + "_trained"]
    it = iter(range(K))
    members = [types.SimpleNamespace(is_trained=bool(t), state_dim=4, action_dim=A, fusable=False, device="cpu",
                                     predict=(lambda o, deterministic=True, k=(next(it) if t else -1): preds[k])) for t in trained]
    pol = ni.EnsemblePolicy([m for m in members if m.is_trained], weights=gold[tag + "_weights"], method=method,
                            uncertainty_threshold=0.2, device="cpu")
    return pol, np.zeros((preds.shape[1], 4), dtype=np.float32), tag


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("K", MEMBERS)
@pytest.mark.parametrize("A", DIMS)
def test_action_is_the_references_bit_for_bit(gold, A, K, method):
    pol, obs, tag = _policy(gold, A, K, method)
    want = gold[f"{tag}_{method}_action"]
    got = pol.predict(obs)
    assert got.dtype == want.dtype == (np.float32 if method == "voting" else np.float64)
    assert got.shape == want.shape and np.array_equal(got, want), (tag, method, np.abs(got - want).max())


@pytest.mark.parametrize("K", MEMBERS)
@pytest.mark.parametrize("A", DIMS)
def test_uncertainty_and_mask(gold, A, K):
    pol, obs, tag = _policy(gold, A, K, "weighted")            # (predict_with_uncertainty's action is the "mean" law whatever the method)
    act, unc, indiv = pol.predict_with_uncertainty(obs, return_individual=True)
    want_act, want_unc, thr = gold[tag + "_unc_action"], gold[tag + "_unc"], float(gold[tag + "_threshold"])
    assert act.dtype == want_act.dtype and np.array_equal(act, want_act)
    assert np.array_equal(np.asarray(indiv).reshape(K, *want_act.shape), gold[tag + "_preds"])
    unc = np.asarray(unc)
    err = np.abs(unc.astype(np.float64) - want_unc.astype(np.float64))
    bound = np.maximum(1e-5 * np.abs(want_unc.astype(np.float64)), 1e-6)
    print(f"{tag}: uncertainty max abs error {err.max():.3g}, max error / bound {np.max(err / bound):.3g}")
    assert np.all(err <= bound), (tag, float(np.max(err / bound)))
    if K >= 2:
        assert unc.dtype == np.float32
        assert np.all(unc[40:44] == 0.0), "identical members: exactly 0"
    # near-agreeing members (rows 44-55, spread 1e-6 .. 1e-3) are inside the bound above; say how close
    if K >= 2:
        print(f"{tag}: near-agreeing rows, max error / bound {np.max((err / bound)[44:56]):.3g}")
    mask = pol.get_high_uncertainty_mask(obs, thr)
    eff = thr or 0.2
    clear = np.abs(want_unc - eff) > 1e-5 * abs(eff)
    assert clear.mean() >= 0.9
    assert np.array_equal(np.asarray(mask)[clear], gold[tag + "_mask"][clear])
    assert np.array_equal(pol.get_high_uncertainty_mask(obs), unc > 0.2)       # threshold None: the policy's own, strict >


def test_documented_order_restated():
    """ensemble_uncertainty is the order include/nig.h documents, restated here scalar by scalar; exactly 0 for identical members;
    the shifted variance keeps the bar where the members agree to 1e-6 .. 1e-3 but member 0 is the outlier."""
    from neorl_industrial_gym_amd.policies import ensemble_uncertainty
    f = np.float32
    rng = np.random.default_rng(5)
    for K, A in ((2, 3), (5, 7), (8, 16)):
        p = np.tanh(rng.normal(0, 1, (K, 6, A))).astype(f)
        got = ensemble_uncertainty(p)
        for r in range(6):
            usum = f(0)
            for j in range(A):
                s1 = s2 = f(0)
                for k in range(1, K):
                    d = f(p[k, r, j] - p[0, r, j])
                    s1 = f(s1 + d)
                    s2 = f(s2 + f(d * d))
                v = f(s2 - f(f(s1 * s1) / f(K)))
                v = v if v > 0 else f(0)
                usum = f(usum + np.sqrt(f(v / f(K))))
            assert got[r] == f(usum / f(A))
        assert np.all(ensemble_uncertainty(np.repeat(p[:1], K, axis=0)) == 0)
        for eps in (1e-6, 1e-4, 1e-3):                     # members 1 .. K-1 agree to eps, member 0 stands 0.3 apart
            q = np.clip(0.4 + eps * rng.uniform(-1, 1, (K, 6, A)), -1, 1).astype(f)
            q[0] = f(0.1)
            want = np.std(q.astype(np.float64), axis=0).mean(axis=-1)
            assert np.all(np.abs(ensemble_uncertainty(q) - want) <= np.maximum(1e-5 * want, 1e-6))


def _nets(S, A, seed):
    rng = np.random.default_rng(seed)
    return [(rng.normal(0, 0.3, (S, 256)).astype(np.float32), rng.normal(0, 0.05, 256).astype(np.float32)),
            (rng.normal(0, 1 / 16, (256, 256)).astype(np.float32), rng.normal(0, 0.05, 256).astype(np.float32)),
            (rng.normal(0, 1 / 8, (256, A)).astype(np.float32), rng.normal(0, 0.1, A).astype(np.float32))]


def _flax(layers, norm=False):
    mlp = {f"Dense_{i}": {"kernel": W, "bias": b} for i, (W, b) in enumerate(layers)}
    if norm:
        mlp["LayerNorm_0"] = {"scale": np.ones(256, np.float32), "bias": np.zeros(256, np.float32)}
    return {"params": {"MLP_0": mlp}}


def _member(layers, trained=True, norm=False):
    return types.SimpleNamespace(state={"actor": types.SimpleNamespace(params=_flax(layers, norm)), "safety": None},
                                 is_trained=trained, constraint_threshold=0.1)


def test_from_agent_recovers_members_weights_method_threshold():
    import neorl_industrial_gym_amd as ni
    S, A = 12, 3
    nets = [_nets(S, A, 10 + k) for k in range(4)]
    w = np.array([0.5, 0.2, 0.2, 0.1])
    agent = types.SimpleNamespace(agents=[_member(nets[0]), _member(nets[1], trained=False), _member(nets[2]), _member(nets[3])],
                                  weights=w, ensemble_method="weighted", uncertainty_threshold=0.35, is_trained=True,
                                  state={"ensemble": "initialized"})
    pol = ni.EnsemblePolicy.from_agent(agent, device="cpu")
    assert len(pol.members) == 3 and pol.fusable and pol.ensemble_method == "weighted" and pol.uncertainty_threshold == 0.35
    for m, k in zip(pol.members, (0, 2, 3)):               # trained members only, list order
        for (W, b), (w_, b_) in zip(nets[k], m.weights):
            assert np.array_equal(W, w_) and np.array_equal(b, b_)
    assert np.array_equal(pol.weights, w)
    # the active weights are the FIRST three entries, whichever members were trained (ensemble.py:238)
    obs = np.random.default_rng(0).normal(0, 1, (5, S)).astype(np.float32)
    preds = np.array([m.predict(obs) for m in pol.members])
    want = np.average(preds, axis=0, weights=w[:3])
    got = pol.predict(obs)
    assert got.dtype == np.float64 and np.array_equal(got, want)
    a1, u1 = pol.predict_with_uncertainty(obs[0])
    assert a1.shape == (A,) and np.ndim(u1) == 0
    assert abs(float(u1) - np.std(preds[:, 0], axis=0).mean()) <= 1e-5 * float(u1) + 1e-6
    d = pol.evaluate_diversity(obs)
    assert d["n_agents"] == 3 and abs(d["disagreement"] - np.std(preds, axis=0).mean()) < 1e-6 and d["diversity_score"] > 0
    # a LayerNorm member is refused; so are an ensemble without trained members and an unknown method
    agent.agents[2] = _member(nets[2], norm=True)
    with pytest.raises(ValueError, match="LayerNorm"):
        ni.EnsemblePolicy.from_agent(agent, device="cpu")
    agent.agents = [_member(nets[0], trained=False)]
    with pytest.raises(RuntimeError):
        ni.EnsemblePolicy.from_agent(agent, device="cpu")
    with pytest.raises(ValueError):
        ni.EnsemblePolicy([nets[0]], method="median", device="cpu")
    # a member of another hidden size is accepted by the policy but not fusable
    small = [(np.zeros((S, 64), np.float32), np.zeros(64, np.float32)), (np.zeros((64, 64), np.float32), np.zeros(64, np.float32)),
             (np.zeros((64, A), np.float32), np.zeros(A, np.float32))]
    assert not ni.EnsemblePolicy([nets[0], small], device="cpu").fusable


def test_abi_lists_and_constants():
    import re
    import neorl_industrial_gym_amd as ni
    txt = open(os.path.join(ROOT, "include", "nig.h")).read()
    assert re.search(r"#define NIG_FLAG_UNCERTAIN 0x8000u", txt) and ni._lib.FLAG_UNCERTAIN == 0x8000
    assert re.search(r"#define NIG_MAX_ENSEMBLE 8\b", txt) and ni._lib.MAX_ENSEMBLE == 8
    assert (ni._lib.ENSEMBLE_AVERAGE, ni._lib.ENSEMBLE_VOTING) == (0, 1)
    L = ni._lib.lib()
    for name, n in (("nig_set_mlp_ensemble", 14), ("nig_rollout_mlp_ensemble", 13)):
        assert name in ni._lib.SYMBOLS and hasattr(L, name) and len(getattr(L, name).argtypes) == n
    # a NULL handle is refused before anything touches a device
    assert L.nig_rollout_mlp_ensemble(None, 4, None, None, 0, None, 0, None, 0, 0, None, None, None) == 1
    assert b"nig_rollout_mlp_ensemble" in L.nig_last_error()
    assert L.nig_set_mlp_ensemble(None, 2, 256, None, None, None, None, None, None, 0, None, 1.0, 0.2, None) == 1
    assert b"nig_set_mlp_ensemble" in L.nig_last_error()
    assert hasattr(ni.batched.BatchedIndustrialEnv, "rollout_mlp_ensemble") and hasattr(ni.batched.BatchedIndustrialEnv, "set_mlp_ensemble")
