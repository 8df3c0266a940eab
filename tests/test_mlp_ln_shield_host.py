"""not-gpu: the fused shield of LayerNorm agents ("nig-mlp-ln-shield-v1", csrc/nig_mlp_ln_shield.hpp) on the host -- the critic
arguments of LayerNormMLPPolicy and its shape refusals, from_agent with and without a safety tree, the predict_with_safety contract,
where utils._install_agent sends the shielded policy, the ABI's declaration, and the restated p (tests/mlp_ln_shield_ref.py: the
restatement of "nig-mlp-ln-v1" on [obs, raw action] and the oracle's det_sigmoidf) against the float64 model under a derived bound."""
import os

import numpy as np
import pytest

import mlp_ln_ref as ref
import mlp_ln_shield_ref as sref
from conftest import ROOT

f32 = np.float32


@pytest.fixture(scope="module")
def ni():
    import neorl_industrial_gym_amd as ni
    return ni


def _networks(S, A, seed=5):
    ws, norms = ref.random_ln_actor(S, A, seed)
    cw, cn = sref.random_ln_critic(S, A, seed + 1, head=0.25)
    return ws, norms, cw, cn


# ---- 1. the constructor ------------------------------------------------------------------------------------------------------------------
def test_the_constructor_takes_a_critic_and_refuses_every_other_shape(ni):
    S, A = 12, 3
    ws, norms, cw, cn = _networks(S, A)
    plain = ni.LayerNormMLPPolicy(ws, norms, device="cpu")                               # as before: no critic, the default threshold
    assert plain.safety_weights is None and plain.safety_norms is None and plain.constraint_threshold == 0.1 and plain.fusable is True
    with pytest.raises(RuntimeError):
        plain.shielded()
    with pytest.raises(RuntimeError):
        plain.predict_with_safety(np.zeros((2, S), f32))
    pol = ni.LayerNormMLPPolicy(ws, norms, device="cpu", safety_weights=cw, safety_norms=cn, constraint_threshold=0.3)
    assert pol.constraint_threshold == 0.3 and pol.safety_eps == pol.eps == 1e-6
    assert all(np.array_equal(W, V) and np.array_equal(b, c) for (W, b), (V, c) in zip(pol.safety_weights, cw))
    assert all(np.array_equal(g, G) and np.array_equal(b, c) for (g, b), (G, c) in zip(pol.safety_norms, cn))
    assert ni.LayerNormMLPPolicy(ws, norms, device="cpu", safety_weights=cw, safety_norms=cn, safety_eps=1e-3).safety_eps == 1e-3
    head_as_vector = [cw[0], cw[1], (cw[2][0].reshape(-1), cw[2][1])]
    assert ni.LayerNormMLPPolicy(ws, norms, device="cpu", safety_weights=head_as_vector, safety_norms=cn).safety_weights[2][0].shape == (256, 1)
    bad = {
        "weights without norms": dict(safety_weights=cw),
        "norms without weights": dict(safety_norms=cn),
        "two layers": dict(safety_weights=cw[:2], safety_norms=cn),
        "one norm": dict(safety_weights=cw, safety_norms=cn[:1]),
        "input width S": dict(safety_weights=[(cw[0][0][:S], cw[0][1]), cw[1], cw[2]], safety_norms=cn),
        "hidden 128": dict(safety_weights=[(cw[0][0][:, :128], cw[0][1][:128]), (cw[1][0][:128, :128], cw[1][1][:128]), (cw[2][0][:128], cw[2][1])],
                           safety_norms=[(g[:128], b[:128]) for g, b in cn]),
        "two head rows": dict(safety_weights=[cw[0], cw[1], (np.zeros((256, 2), f32), np.zeros(2, f32))], safety_norms=cn),
        "short gamma": dict(safety_weights=cw, safety_norms=[(cn[0][0][:255], cn[0][1]), cn[1]]),
    }
    for eps in (0.0, -1e-6, float("nan"), float("inf")):
        bad[f"safety_eps {eps}"] = dict(safety_weights=cw, safety_norms=cn, safety_eps=eps)
    for what, kw in bad.items():
        with pytest.raises(ValueError):
            ni.LayerNormMLPPolicy(ws, norms, device="cpu", **kw)
            pytest.fail(what)


# ---- 2. from_agent -----------------------------------------------------------------------------------------------------------------------
class _State:
    def __init__(self, params):
        self.params = params


def _tree(ws, norms):
    mlp = {f"Dense_{i}": {"kernel": W, "bias": b} for i, (W, b) in enumerate(ws)}
    if norms is not None:
        mlp.update({f"LayerNorm_{i}": {"scale": g, "bias": b} for i, (g, b) in enumerate(norms)})
    return _State({"params": {"MLP_0": mlp}})


class _Agent:
    def __init__(self, actor, safety="absent", threshold=None):
        self.state = {"actor": actor}
        if safety != "absent":
            self.state["safety"] = safety
        if threshold is not None:
            self.constraint_threshold = threshold


def test_from_agent_reads_the_safety_tree_when_there_is_one(ni):
    S, A = 12, 3
    ws, norms, cw, cn = _networks(S, A)
    pol = ni.LayerNormMLPPolicy.from_agent(_Agent(_tree(ws, norms), _tree(cw, cn), threshold=0.25), device="cpu")
    assert pol.constraint_threshold == 0.25 and pol.fusable is True
    assert all(np.array_equal(W, V) and np.array_equal(b, c) for (W, b), (V, c) in zip(pol.safety_weights, cw))
    assert all(np.array_equal(g, G) and np.array_equal(b, c) for (g, b), (G, c) in zip(pol.safety_norms, cn))
    assert ni.LayerNormMLPPolicy.from_agent(_Agent(_tree(ws, norms), _tree(cw, cn)), device="cpu").constraint_threshold == 0.1
    for agent in (_Agent(_tree(ws, norms)), _Agent(_tree(ws, norms), None, threshold=0.25)):     # without a safety entry: as before
        bare = ni.LayerNormMLPPolicy.from_agent(agent, device="cpu")
        assert bare.safety_weights is None and bare.constraint_threshold == 0.1
        assert all(np.array_equal(W, V) for (W, _), (V, _) in zip(bare.weights, ws))
        with pytest.raises(RuntimeError):
            bare.shielded()
    with pytest.raises(ValueError, match="safety"):                                     # a plain safety tree
        ni.LayerNormMLPPolicy.from_agent(_Agent(_tree(ws, norms), _tree(cw, None)), device="cpu")
    with pytest.raises(ValueError, match="safety"):
        ni.LayerNormMLPPolicy.from_agent(_Agent(_tree(ws, norms), _tree(cw, cn[:1])), device="cpu")


# ---- 3. predict_with_safety --------------------------------------------------------------------------------------------------------------
def test_predict_with_safety_halves_where_p_is_not_below_the_threshold(ni):
    S, A = 28, 10
    ws, norms, cw, cn = _networks(S, A, seed=9)
    obs = np.random.default_rng(3).normal(0, 1, (256, S)).astype(f32)
    pol = ni.LayerNormMLPPolicy(ws, norms, device="cpu", safety_weights=cw, safety_norms=cn, constraint_threshold=0.0)
    raw = pol.predict(obs)
    m = sref.model64(cw, cn, obs, raw)
    p64 = 1.0 / (1.0 + np.exp(-m["pre"][:, 0]))
    a, p = pol.predict_with_safety(obs, safety_threshold=float(np.median(p64)))
    assert a.shape == (256, A) and p.shape == (256,) and a.dtype == f32 and p.dtype == f32
    assert np.abs(p - p64).max() <= 2e-5, "torch's form of the critic against the float64 model"
    thr = float(np.median(p64))
    clear = np.abs(p64 - thr) > 1e-4                                                     # (lanes within the forms' distance of the threshold say nothing)
    halved = ~(p64 < thr)
    assert 64 < halved.sum() < 192 and clear.sum() > 200
    assert np.array_equal(a[clear], np.where(halved[:, None], raw * f32(0.5), raw)[clear])
    pol.constraint_threshold = thr                                                       # the fallback: None and 0.0 take constraint_threshold
    for st in (None, 0.0):
        a2, p2 = pol.predict_with_safety(obs, safety_threshold=st)
        assert np.array_equal(a2, a) and np.array_equal(p2, p)
    a3, _ = pol.predict_with_safety(obs, safety_threshold=2.0)
    assert np.array_equal(a3, raw)
    a1, p1 = pol.predict_with_safety(obs[0], safety_threshold=2.0)
    assert a1.shape == (A,) and np.ndim(p1) == 0
    sh = pol.shielded()
    assert type(sh).__name__ == "ShieldedLayerNormPolicy" and sh.base is pol and sh.threshold == thr and sh.normalization == "layer_norm" and sh.fusable is True
    assert np.array_equal(sh.predict(obs), a) and pol.shielded(0.75).threshold == 0.75
    import torch
    assert np.array_equal(sh.predict_device(torch.as_tensor(obs)).numpy(), a)


# ---- 4. the routing ----------------------------------------------------------------------------------------------------------------------
def test_install_agent_sends_the_shielded_policy_to_rollout_mlp_safe(ni):
    from test_limits_families_host import _route
    S, A = 12, 3
    ws, norms, cw, cn = _networks(S, A)
    pol = ni.LayerNormMLPPolicy(ws, norms, device="cpu", safety_weights=cw, safety_norms=cn, constraint_threshold=0.4)
    sh = pol.shielded()

    def names(route):
        return route[0], [c[0] for c in route[2]]
    name, args, calls, _ = _route(ni, sh, False)
    assert (name, [c[0] for c in calls]) == ("rollout_mlp_safe", ["set_mlp_policy_ln", "set_mlp_safety_ln"]) and args == (7,)
    assert calls[0][1] == (pol,) and calls[1][1] == (pol, 0.4)
    assert names(_route(ni, pol, False)) == ("rollout_mlp", ["set_mlp_policy_ln"])      # the bare policy keeps its route
    assert names(_route(ni, sh, True)) == (None, [])                                    # added constraints: the host loop
    assert names(_route(ni, sh, False, plain=False)) == (None, [])                      # recorded draws
    assert names(_route(ni, ni.Disturbed(sh, ni.Disturbance(action_noise=0.1), seed=1), False)) == (None, [])
    ows, onorms, ocw, ocn = _networks(15, 4)
    odd = ni.LayerNormMLPPolicy(ows, onorms, device="cpu", safety_weights=ocw, safety_norms=ocn).shielded()
    assert names(_route(ni, odd, False, state_dim=15, action_dim=4)) == (None, [])      # WaterTreatment's shape: no MFMA actor
    raw_agent = _Agent(_tree(ws, norms), _tree(cw, cn))                                 # a raw reference agent: the host loop, as before
    assert names(_route(ni, raw_agent, False)) == (None, [])


def test_the_abi_is_declared_bound_and_exported(ni):
    L = ni._lib.lib()
    hdr = open(os.path.join(ROOT, "include", "nig.h")).read()
    assert "int nig_set_mlp_safety_ln(" in hdr and "#define NIG_SAFETY_SIGMOID_LN  3" in hdr and '"nig-mlp-ln-shield-v1"' in hdr
    assert len(ni._lib.PROTOTYPES["nig_set_mlp_safety_ln"][1]) == 15 and hasattr(L, "nig_set_mlp_safety_ln")
    assert ni._lib.SAFETY_SIGMOID_LN == 3 and hasattr(ni.BatchedIndustrialEnv, "set_mlp_safety_ln")
    assert ni.__version__ == "0.8.0" and L.nig_version().decode().startswith("nig 0.8.0")       # the version string stays


# ---- 5. the restated p against the formula in float64 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,A", [(12, 3), (32, 8), (28, 10)])
def test_the_restated_p_is_the_formula_within_the_derived_bound(oracle, S, A):
    """|p - p64| <= pre_bound / 4 + 3 ulp(p) + a float64 rounding: the sigmoid's slope is at most 1/4, so the pre-activation's forward
    error (ref.pre_bound with the critic's input width S + A: its layer-1 chain has that many steps and the bias and pad steps) enters
    p with at most that factor; det_sigmoidf is within 3 ulp of the sigmoid on normal results (tests/detmath_check.c), and p <= 1
    puts an ulp at 2^-23 at most."""
    ws, norms, cw, cn = _networks(S, A, seed=40 + S)
    obs = np.random.default_rng(S).normal(0, 1, (4096, S)).astype(f32)
    raw = ref.act(oracle, ws, norms, obs)
    m = sref.model64(cw, cn, obs, raw)
    pre = sref.critic_pre(cw, cn, obs, raw)
    bound = ref.pre_bound(m, S + A + (S + A) % 2)[:, 0]
    err = np.abs(pre.astype(np.float64) - m["pre"][:, 0])
    assert np.all(err <= bound), float(np.max(err / bound))
    p = sref.prob(oracle, cw, cn, obs, raw)
    p64 = 1.0 / (1.0 + np.exp(-m["pre"][:, 0]))
    perr = np.abs(p.astype(np.float64) - p64)
    pbound = 0.25 * bound + 3.0 * 2.0 ** -23 + 2.0 ** -50
    print(f"S={S} A={A}: pre error {err.max():.3g} (bound up to {bound.max():.3g}); p error {perr.max():.3g}, largest error / bound {np.max(perr / pbound):.3g}")
    assert np.all(perr <= pbound), float(np.max(perr / pbound))
    assert len(np.unique(p)) > 2048 and 0.02 < p.min() and p.max() < 0.98, "p says something about its pre-activation"
