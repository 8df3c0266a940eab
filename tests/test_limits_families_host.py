"""not-gpu: the _limited twins of the closed-loop families (include/nig.h: nig_rollout_mlp_safe_limited, _search_limited,
_gated_limited, _projected_limited, _ensemble_limited, _disturbed_limited, nig_rollout_policy_disturbed_limited) -- the ABI's
declarations, and where utils._install_agent sends every agent kind on an env with and without added safety constraints.  The
device side is tests/test_gpu_limits_families.py."""
import os
import re

import numpy as np
import pytest

import closed_loop_matrix as M
from conftest import ROOT

TWINS = ("nig_rollout_mlp_safe_limited", "nig_rollout_mlp_search_limited", "nig_rollout_mlp_gated_limited",
         "nig_rollout_mlp_projected_limited", "nig_rollout_mlp_ensemble_limited", "nig_rollout_mlp_disturbed_limited",
         "nig_rollout_policy_disturbed_limited")
S, A = 12, 3


@pytest.fixture(scope="module")
def ni():
    import neorl_industrial_gym_amd as ni
    return ni


def test_the_abi_is_declared_bound_and_exported(ni):
    """Each twin is declared in the header with xflags_out before the stream, bound with one pointer more than its parent, and
    exported by the built library."""
    L = ni._lib.lib()
    hdr = open(os.path.join(ROOT, "include", "nig.h")).read()
    for name in TWINS:
        m = re.search(r"\bint %s\(([^;]*)\);" % name, hdr)
        assert m, name
        assert re.search(r"uint32_t \*xflags_out,\s*void \*stream$", m.group(1)), name
        assert name in ni._lib.PROTOTYPES and hasattr(L, name), name
        parent = name[:-len("_limited")]
        pr, pa = ni._lib.PROTOTYPES[parent]
        tr, ta = ni._lib.PROTOTYPES[name]
        assert tr is pr and ta == pa[:-1] + [ni._lib.vp, pa[-1]], name
        assert hasattr(ni.BatchedIndustrialEnv, name[len("nig_"):]), name
    assert hdr.count("a rollout equals nig_step_limited fed") >= 1 + 6      # the plain twins' sentence, in every new comment too


class StubEnv:
    """Records what _install_agent does to an env: every set_* / install call and the name of every rollout method asked for."""
    device = "cpu"

    def __init__(self, has_limits, state_dim=S, action_dim=A):
        self.has_limits, self.state_dim, self.action_dim = has_limits, state_dim, action_dim
        self.calls = []

    def __getattr__(self, name):
        if name.startswith("set_") or name.startswith("rollout_"):
            def method(*a, **k):
                self.calls.append((name, a))
                return name
            method.route = name
            return method
        raise AttributeError(name)


def _route(ni, agent, has_limits, plain=True, **dims):
    """(the name of the rollout method _install_agent picked or None, the arguments a call rollout(7) hands it, the env's calls)"""
    from neorl_industrial_gym_amd.utils import _install_agent
    env = StubEnv(has_limits, **dims)
    _, rollout, disturbed = _install_agent(agent, env, plain)
    if rollout is None:
        return None, None, env.calls, disturbed
    n = len(env.calls)
    rollout(7)
    (name, args), = env.calls[n:]
    return name, args, env.calls[:n], disturbed


def _agents(ni):
    from neorl_industrial_gym_amd.policies import ConstraintProjectionPolicy, EnsemblePolicy, MLPPolicy, SafetyEnsemblePolicy
    ws = M.random_actor(S, A, 1)
    mlp = MLPPolicy(ws, device="cpu", safety_weights=M.random_critic(S, A, 2), constraint_threshold=0.3)
    dist = ni.Disturbance(obs_noise=0.1, action_noise=0.1, hold="step")
    return {
        "policy": (ni.random_agent(S, A), "rollout_policy", (7,)),
        "mlp": (MLPPolicy(ws, device="cpu"), "rollout_mlp", (7,)),
        "shielded": (mlp.shielded(), "rollout_mlp_safe", (7,)),
        "searching": (mlp.searching(n_candidates=3), "rollout_mlp_search", (7, 3)),
        "gated": (SafetyEnsemblePolicy(ws, [M.random_critic(S, A, 3, n_out=2), M.random_critic(S, A, 4, n_out=2)], device="cpu"),
                  "rollout_mlp_gated", (7,)),
        "projecting": (ConstraintProjectionPolicy(ws, M.random_critic(S, A, 5, n_out=2), max_iters=3, step=0.25, device="cpu"),
                       "rollout_mlp_projected", (7, 3, 0.25)),
        "ensemble": (EnsemblePolicy([ws, M.random_actor(S, A, 6), M.random_actor(S, A, 7)], method="voting", device="cpu"),
                     "rollout_mlp_ensemble", (7,)),
        "disturbed policy": (ni.Disturbed(ni.random_agent(S, A), dist, seed=1), "rollout_policy_disturbed", (7,)),
        "disturbed mlp": (ni.Disturbed(MLPPolicy(ws, device="cpu"), dist, seed=1), "rollout_mlp_disturbed", (7,)),
    }


def test_install_agent_picks_the_limited_method_of_every_family(ni):
    """With added constraints every agent kind goes to the _limited method of the family it takes without them, with the same
    arguments and the same installation calls; without them the routes are the ones they were."""
    for kind, (agent, parent, args) in _agents(ni).items():
        name0, args0, calls0, dist0 = _route(ni, agent, False)
        name1, args1, calls1, dist1 = _route(ni, agent, True)
        assert name0 == parent and args0 == args, (kind, name0, args0)
        assert name1 == parent + "_limited" and args1 == args, (kind, name1, args1)
        assert [c[0] for c in calls0] == [c[0] for c in calls1] and dist0 == dist1, kind
        assert dist0 == ({"disturbed policy": "fused-policy", "disturbed mlp": "fused-mlp"}.get(kind)), kind


def test_a_reference_ensemble_agent_is_upgraded_both_ways(ni):
    """A reference EnsembleAgent (agents, weights, ensemble_method; no install) whose members MLPPolicy.from_agent can read."""
    class Params:
        def __init__(self, ws):
            self.params = {"params": {"MLP_0": {f"Dense_{i}": {"kernel": W, "bias": b} for i, (W, b) in enumerate(ws)}}}

    class Member:
        is_trained = True

        def __init__(self, ws):
            self.state = {"actor": Params(ws)}

    class Ensemble:
        is_trained = True
        ensemble_method = "voting"
        uncertainty_threshold = 0.2

        def __init__(self):
            self.agents = [Member(M.random_actor(S, A, k)) for k in (1, 2, 3)]
            self.weights = np.ones(3) / 3

    from neorl_industrial_gym_amd.policies import EnsemblePolicy
    try:
        EnsemblePolicy.from_agent(Ensemble(), device="cpu")
    except Exception as e:                              # (what _install_agent would swallow: say it here instead)
        pytest.fail(f"the stand-in is not what EnsemblePolicy.from_agent reads: {e!r}")
    assert _route(ni, Ensemble(), False)[0] == "rollout_mlp_ensemble"
    assert _route(ni, Ensemble(), True)[0] == "rollout_mlp_ensemble_limited"


def test_agents_of_the_host_loop_stay_there(ni):
    """A non-fusable agent, recorded draws (plain = False) and an MFMA family on an env without the MFMA actor under limits."""
    from neorl_industrial_gym_amd.policies import MLPPolicy

    class Host:
        is_trained = True

        def predict(self, obs, deterministic=True):
            return np.zeros((len(obs), A), np.float32)

    narrow = [(np.zeros((S, 64), np.float32), np.zeros(64, np.float32)), (np.zeros((64, 64), np.float32), np.zeros(64, np.float32)),
              (np.zeros((64, A), np.float32), np.zeros(A, np.float32))]
    for limits in (False, True):
        assert _route(ni, Host(), limits)[0] is None
        assert _route(ni, MLPPolicy(narrow, device="cpu"), limits)[0] is None
        assert _route(ni, ni.Disturbed(Host(), ni.Disturbance(obs_noise=0.1), seed=1), limits)[0] is None
        for kind, (agent, _, _) in _agents(ni).items():
            assert _route(ni, agent, limits, plain=False)[0] is None, kind
    odd = _agents(ni)
    assert _route(ni, MLPPolicy(M.random_actor(15, 4, 1), device="cpu"), True, state_dim=15, action_dim=4)[0] is None
    assert _route(ni, odd["policy"][0], True, state_dim=15, action_dim=4)[0] == "rollout_policy_limited"
