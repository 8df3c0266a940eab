"""not-gpu: the host side of the disturbance model ("nig-disturb-v1", include/nig.h) -- Disturbance validation and struct
packing, the robustness score arithmetic on hand numbers, Disturbed.predict on a stub agent (held / fresh draws, their
moments) and MLPPolicy.exploring()."""
import ctypes as C

import numpy as np
import pytest

f32 = np.float32


@pytest.fixture(scope="module")
def ni():
    import neorl_industrial_gym_amd as ni
    return ni


def test_exports(ni):
    L = ni._lib.lib()
    for name, n in (("nig_set_disturbance", 3), ("nig_rollout_policy_disturbed", 13), ("nig_rollout_mlp_disturbed", 13)):
        assert name in ni._lib.SYMBOLS and hasattr(L, name) and len(getattr(L, name).argtypes) == n
    for name in ("Disturbance", "Disturbed", "evaluate_robustness", "robustness_scores"):
        assert name in ni.__all__ and hasattr(ni, name)
    assert L.nig_set_disturbance(None, None, None) == 1 and b"NULL handle" in L.nig_last_error()
    assert L.nig_rollout_policy_disturbed(None, 1, None, None, 0, None, 0, None, 0, 0, None, 0, None) == 1
    assert L.nig_rollout_mlp_disturbed(None, 1, None, None, 0, None, 0, None, 0, 0, None, 0, None) == 1
    # the struct the binding packs is the header's: 32 + 10 floats, two bounds, one int32
    assert C.sizeof(ni._lib.DisturbanceStruct) == 4 * (32 + 10 + 2 + 1)
    assert (ni._lib.HOLD_STEP, ni._lib.HOLD_EPISODE) == (0, 1)


def test_disturbance_packing(ni):
    d = ni.Disturbance(obs_noise=0.25, action_noise=[0.1, 0.0, 0.5], clip=(-1, 1), hold="episode")
    D = d.to_struct(12, 3)
    assert list(D.sigma_obs)[:12] == [0.25] * 12 and list(D.sigma_obs)[12:] == [0.0] * 20       # scalar broadcast, pad zero
    assert [f32(x) for x in list(D.sigma_act)[:3]] == [f32(0.1), f32(0.0), f32(0.5)] and list(D.sigma_act)[3:] == [0.0] * 7
    assert (D.clip_lo, D.clip_hi, D.hold) == (-1.0, 1.0, 1)
    D0 = ni.Disturbance().to_struct(32, 10)
    assert not any(D0.sigma_obs) and not any(D0.sigma_act) and D0.hold == 0
    assert D0.clip_lo == -np.inf and D0.clip_hi == np.inf
    so, sa = ni.Disturbance(obs_noise=np.arange(4) * 0.5).sigmas(4, 2)
    assert so.dtype == f32 and so.tolist() == [0.0, 0.5, 1.0, 1.5] and sa.tolist() == [0.0, 0.0]
    s2 = ni.Disturbance(obs_noise=1.0, action_noise=1.0, hold="episode").scaled(0.3)
    assert s2.obs_noise == f32(0.3) and s2.action_noise == f32(0.3) and s2.hold == "episode"


@pytest.mark.parametrize("kw", [dict(obs_noise=-0.1), dict(obs_noise=np.nan), dict(obs_noise=np.inf), dict(action_noise=-1.0),
                                dict(action_noise=[0.1, np.nan]), dict(action_noise=[0.1, np.inf]), dict(clip=(1.0, -1.0)),
                                dict(clip=(np.nan, 1.0)), dict(clip=(0.0, np.nan)), dict(hold="forever"),
                                dict(obs_noise=np.zeros((2, 2)))])
def test_disturbance_refusals(ni, kw):
    with pytest.raises(ValueError):
        ni.Disturbance(**kw)


def test_disturbance_dimension_mismatch(ni):
    with pytest.raises(ValueError):
        ni.Disturbance(obs_noise=[0.1, 0.2]).to_struct(12, 3)
    with pytest.raises(ValueError):
        ni.Disturbance(action_noise=[0.1] * 4).to_struct(12, 3)
    with pytest.raises(ValueError):
        ni.Disturbance().to_struct(33, 3)


def test_robustness_scores_hand_numbers(ni):
    levels, kinds = [0.0, 0.1, 0.2], ["observation_noise", "action_noise"]
    res = {"observation_noise": {0.0: {"mean_return": 8.0}, 0.1: {"mean_return": 6.0}, 0.2: {"mean_return": 2.0}},
           "action_noise": {0.0: {"mean_return": 8.0}, 0.1: {"mean_return": 8.0}, 0.2: {"mean_return": 4.0}}}
    scores, overall = ni.robustness_scores(res, levels, kinds)          # (dyadic numbers: every quotient and mean is exact)
    assert scores == {"observation_noise": 0.5, "action_noise": 0.75} and overall == 0.625
    # the baseline is level 0 of the FIRST type, whatever the others hold there
    res["action_noise"][0.0]["mean_return"] = 99.0
    assert ni.robustness_scores(res, levels, kinds)[0]["action_noise"] == 0.75
    # negative returns: plain ratios, as upstream
    neg = {"observation_noise": {0.0: {"mean_return": -2.0}, 0.1: {"mean_return": -4.0}}}
    assert ni.robustness_scores(neg, [0.0, 0.1], ["observation_noise"]) == ({"observation_noise": 2.0}, 2.0)
    # zero baseline: every score is 0.0
    res["observation_noise"][0.0]["mean_return"] = 0.0
    assert ni.robustness_scores(res, levels, kinds) == ({"observation_noise": 0.0, "action_noise": 0.0}, 0.0)


class _Echo:
    """stub agent: action = the first A observation columns"""
    is_trained = True

    def __init__(self, S, A):
        self.state_dim, self.action_dim = S, A

    def predict(self, observations, deterministic=True):
        return np.asarray(observations, dtype=f32)[..., :self.action_dim]


def test_disturbed_surface(ni):
    w = ni.Disturbed(_Echo(4, 2), ni.Disturbance())
    assert w.is_trained and (w.state_dim, w.action_dim) == (4, 2)
    obs = np.arange(12, dtype=f32).reshape(3, 4)
    assert np.array_equal(w.predict(obs), obs[:, :2])                      # all-zero sigmas, no clip: the agent itself
    assert w.predict(obs[0]).shape == (2,)


@pytest.mark.parametrize("kind", ["obs", "act"])
def test_disturbed_hold(ni, kind):
    obs = np.zeros((5, 4), dtype=f32)
    kw = dict(obs_noise=0.5) if kind == "obs" else dict(action_noise=0.5)
    held = ni.Disturbed(_Echo(4, 2), ni.Disturbance(hold="episode", **kw), seed=3)
    a0, a1 = held.predict(obs), held.predict(obs)
    assert np.array_equal(a0, a1) and np.any(a0 != 0)                      # the same perturbation on every call ...
    assert not np.array_equal(a0[0], a0[1])                                # ... of each lane's own
    held.begin_episode(5)
    a2 = held.predict(obs)
    assert not np.array_equal(a2, a0) and np.array_equal(held.predict(obs), a2)   # ... until begin_episode
    fresh = ni.Disturbed(_Echo(4, 2), ni.Disturbance(hold="step", **kw), seed=3)
    assert not np.array_equal(fresh.predict(obs), fresh.predict(obs))


@pytest.mark.parametrize("kind,sigma", [("obs", 0.3), ("act", 0.1)])
def test_disturbed_moments(ni, kind, sigma):
    """10^5 draws: sample mean within 4 sigma / sqrt(n) of 0, sample standard deviation within 4 sigma / sqrt(2 n) of sigma."""
    n = 100_000
    kw = dict(obs_noise=sigma) if kind == "obs" else dict(action_noise=sigma)
    w = ni.Disturbed(_Echo(1, 1), ni.Disturbance(**kw), seed=11)
    x = w.predict(np.zeros((n, 1), dtype=f32)).astype(np.float64).ravel()
    assert abs(x.mean()) < 4 * sigma / np.sqrt(n)
    assert abs(x.std() - sigma) < 4 * sigma / np.sqrt(2 * n)


def test_exploring_clips(ni):
    rng = np.random.default_rng(0)
    S, A, H = 12, 3, 256
    W = [(rng.standard_normal((S, H)).astype(f32), np.zeros(H, f32)), (rng.standard_normal((H, H)).astype(f32), np.zeros(H, f32)),
         (rng.standard_normal((H, A)).astype(f32), np.zeros(A, f32))]
    pol = ni.MLPPolicy(W, device="cpu")                                     # (saturated tanh head: actions at +-1)
    ex = pol.exploring(sigma=0.5)
    assert isinstance(ex, ni.Disturbed) and ex.disturbance.clip == (f32(-1), f32(1)) and ex.disturbance.hold == "step"
    assert ex.disturbance.action_noise == f32(0.5) and not np.any(ex.disturbance.obs_noise)
    assert pol.exploring().disturbance.action_noise == f32(0.1)            # agents/cql.py:345-350
    obs = rng.standard_normal((2000, S)).astype(f32)
    base, a = pol.predict(obs), ex.predict(obs)
    assert a.shape == base.shape and a.min() >= -1.0 and a.max() <= 1.0
    assert np.any(np.abs(base) == 1.0) and np.any(a != base)
    assert np.all(np.abs(a - base) <= 0.5 * 5.5)                            # |z| <= 5.5 for any sane generator
    assert np.array_equal(pol.predict(obs, deterministic=False), base)     # predict itself stays as it is
