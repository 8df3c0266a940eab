"""FIXTURE GENERATION ONLY (never collected, never imported by a test): records what the reference's EnsembleAgent computes,
for tests/test_ensemble_host.py, into tests/golden/ensemble_laws.npz.

    python tests/gen_ensemble_golden.py

Runs where the reference sources are present (oracle/ref_import.py, imported unchanged).  The reference's
agents/ensemble.py is executed IN PLACE: a shell package `neorl_industrial.agents` whose __path__ is the reference directory,
stub modules agents.base / .cql / .iql / .td3bc that only provide the four class names ensemble.py imports (the real ones need
jax / flax / optax), and EnsembleAgent._predict_impl / .predict_with_uncertainty / .get_high_uncertainty_mask called on a
stand-in object (agents, weights, ensemble_method, is_trained, logger, uncertainty_threshold) whose members have `is_trained`
and `predict`.  Data only is written: member actions, weights, trained flags, and the reference's outputs.

Cases: A in {3, 7, 8, 10, 16} x K trained members in {1, 2, 3, 5, 8} (one set of member actions each, ROWS rows) x the three
ensemble methods.  Untrained members sit in the middle of the agent list ((A + K) % 3 of them), so the active weights -- the FIRST
K entries of the weight vector -- are not the trained members' own; the weight vectors rotate through normalised, unnormalised
and partly negative.  Rows: tanh-of-normal member actions about a common centre; identical members; members that agree to within
1e-6 .. 1e-3 (where a careless variance cancels); member actions at +-1.  The mask is recorded at the median of the reference's own
uncertainties; the generator fails unless at least 90 % of every case's rows lie further than 1e-5 relative from that threshold
(the rows a test may hold the mask to exactly).
"""
import importlib
import logging
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_import  # noqa: E402

ROWS = 64
DIMS, MEMBERS, METHODS = (3, 7, 8, 10, 16), (1, 2, 3, 5, 8), ("mean", "weighted", "voting")


def load_ensemble_class():
    ref_import.load_reference()
    agents = types.ModuleType("neorl_industrial.agents")
    agents.__path__ = [os.path.join(ref_import.REF_SRC, "agents")]
    sys.modules["neorl_industrial.agents"] = agents
    for mod, cls in (("base", "OfflineAgent"), ("cql", "CQLAgent"), ("iql", "IQLAgent"), ("td3bc", "TD3BCAgent")):
        m = types.ModuleType("neorl_industrial.agents." + mod)
        setattr(m, cls, type(cls, (), {}))
        sys.modules[m.__name__] = m
    return importlib.import_module("neorl_industrial.agents.ensemble").EnsembleAgent


def member_actions(rng, K, A):
    """float32 [K, ROWS, A] in [-1, 1]"""
    f32 = np.float32
    p = np.empty((K, ROWS, A), dtype=f32)
    centre = rng.normal(0, 0.8, (ROWS, A))
    p[:, :40] = np.tanh(centre[None, :40] + 0.3 * rng.normal(0, 1, (K, 40, A))).astype(f32)
    base = np.tanh(centre[40:56]).astype(f32)
    p[:, 40:44] = base[None, :4]                                            # identical members
    for i, eps in enumerate((1e-6, 1e-5, 1e-4, 1e-3)):                      # near-agreeing members
        r = slice(44 + 3 * i, 47 + 3 * i)
        p[:, r] = np.clip(base[None, 4 + 3 * i:7 + 3 * i].astype(np.float64) + eps * rng.uniform(-1, 1, (K, 3, A)), -1, 1).astype(f32)
    tail = np.tanh(centre[None, 56:] + 0.3 * rng.normal(0, 1, (K, 8, A))).astype(f32)
    at_one = rng.uniform(0, 1, tail.shape) < 0.4
    p[:, 56:] = np.where(at_one, np.sign(tail).astype(f32), tail)           # member actions at +-1
    return p


def main():
    Ens = load_ensemble_class()

    class StandIn:
        _predict_impl = Ens._predict_impl
        predict_with_uncertainty = Ens.predict_with_uncertainty
        get_high_uncertainty_mask = Ens.get_high_uncertainty_mask
        is_trained = True
        logger = logging.getLogger("gen_ensemble_golden")

    logging.disable(logging.WARNING)                        # (K = 1 warns "need at least 2 trained agents")
    rng = np.random.default_rng(20240607)
    out, case = {}, 0
    for A in DIMS:
        for K in MEMBERS:
            preds = member_actions(rng, K, A)
            n_un = (A + K) % 3
            trained = np.ones(K + n_un, dtype=bool)
            trained[1 + np.arange(n_un) * 2 if K > 1 else 1 + np.arange(n_un)] = False   # untrained members inside the list
            assert trained.sum() == K and trained[0]
            obs = np.zeros((ROWS, 4), dtype=np.float32)     # the stand-in members ignore it
            it = iter(range(K))
            agents = [types.SimpleNamespace(is_trained=bool(t), predict=(lambda o, deterministic=True, k=(next(it) if t else -1): preds[k]))
                      for t in trained]
            kind = case % 3
            w = rng.uniform(0.2, 1.0, K + n_un)
            if kind == 0:
                w = w / w.sum()
            elif kind == 1:
                w = w * 3.7
            else:
                w[1 % len(w)] = -0.35 * w[1 % len(w)]
            assert abs(np.sum(w[:K])) > 0.1
            s = StandIn()
            s.agents, s.weights, s.uncertainty_threshold = agents, w, 0.2
            tag = f"A{A}_K{K}"
            out[tag + "_preds"], out[tag + "_weights"], out[tag + "_trained"] = preds, w, trained
            for method in METHODS:
                s.ensemble_method = method
                act = s._predict_impl(obs)
                out[f"{tag}_{method}_action"] = act
                assert act.dtype == (np.float32 if method == "voting" else np.float64)
            s.ensemble_method = "mean"
            act_u, unc = s.predict_with_uncertainty(obs)
            unc = np.asarray(unc)
            thr = float(np.median(unc))
            mask = np.asarray(s.get_high_uncertainty_mask(obs, thr))
            eff = thr or s.uncertainty_threshold
            clear = np.abs(unc - eff) > 1e-5 * abs(eff)
            share = clear.mean()
            assert share >= 0.9, (tag, share)
            out[tag + "_unc_action"], out[tag + "_unc"], out[tag + "_threshold"], out[tag + "_mask"] = act_u, unc, np.float64(thr), mask
            print(f"{tag}: untrained {n_un}, weights kind {kind}, median uncertainty {thr:.6g}, rows clear of the threshold {share:.3f}, "
                  f"flagged {int(mask.sum())}/{ROWS}")
            case += 1
    path = os.path.join(ROOT, "tests", "golden", "ensemble_laws.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
