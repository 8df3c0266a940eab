"""-m gpu: the closed-loop families under added box constraints -- the _limited twins of rollout_mlp_safe, _search, _gated,
_projected, _ensemble ("voting" and "mean"), _disturbed and rollout_policy_disturbed (include/nig.h).
  1. inert limits (infinite bounds) are off: every output and the handle equal the parent's bit for bit;
  2. non-critical limits leave the trajectory alone, and every xflags word is BoxConstraint.check_fn in NumPy on that step's
     obs_out row and clipped act_out row (the float64 action for the "mean" ensemble where the env steps on it);
  3. the limited loop is the limited step kernel fed with the loop's own actions;
  4. the family's correction still happens under real limits;
  5. refusals and the memory footprint of xflags_out;
  6. evaluate_with_safety / evaluate_robustness end to end.
Shapes are the closed-loop matrix's (tests/closed_loop_matrix.py): B = 700 and 5, T = 7, episodes of at most 5 steps, seed 0x5EED,
auto-reset and tally on.  Thresholds are medians of a first parent run at B = 700, so about half the lanes take the correction."""
import ctypes as C

import numpy as np
import pytest
import torch

import closed_loop_matrix as M
from footprint import Arena, Layout
from test_gpu_limits import (LIMIT_ENVS, LIMIT_MFMA, MAXS, SEED, T, _bits, _code, _handle, _inert, _make, _quantile_boxes,
                             _same_tally)

pytestmark = pytest.mark.gpu

MFMA_FAMILIES = ("safe", "search", "gated", "projected", "ens_voting", "ens_mean", "disturbed")
CASES = [(f, k) for f in MFMA_FAMILIES for k, _ in LIMIT_MFMA] + [("policy_disturbed", k) for k, _ in LIMIT_ENVS]
ACT64 = ("cr", "pg", "ra")                     # the envs whose step follows a float64 action's type (nig_step64)
N_CAND, GATE_K, GATE_C, PROJ_ITERS, PROJ_STEP, ENS_K = 3, 2, 2, 3, 0.5, 3
MEAN_W = [0.9, 0.4, 1.7]
PARENT = {"safe": "rollout_mlp_safe", "search": "rollout_mlp_search", "gated": "rollout_mlp_gated", "projected": "rollout_mlp_projected",
          "ens_voting": "rollout_mlp_ensemble", "ens_mean": "rollout_mlp_ensemble", "disturbed": "rollout_mlp_disturbed",
          "policy_disturbed": "rollout_policy_disturbed"}
CORRECTS = {"safe": "FLAG_SHIELDED", "search": "FLAG_SHIELDED", "gated": "FLAG_SHIELDED", "projected": "FLAG_SHIELDED",
            "ens_voting": "FLAG_UNCERTAIN", "ens_mean": "FLAG_UNCERTAIN"}


@pytest.fixture(scope="module")
def ni():
    import neorl_industrial_gym_amd as ni
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return ni


# ---- the families' networks and settings ----------------------------------------------------------------------------------------
def _actor(ni, key, S, A, seed):
    """test_gpu_limits._agent's actor: ChemicalReactor's first layer scaled per state column, M.matrix_actor for the rest."""
    ws = M.random_actor(S, A, seed)
    if key == "cr":
        sc = M.state_scale(ni, key, SEED)
        ws = [((ws[0][0] * np.float32(20.0) * sc[:, None]).astype(np.float32), ws[0][1]), ws[1], ws[2]]
    return M.matrix_actor(ni, key, ws, SEED)


def _critic(ni, key, S, A, seed, n_out=1):
    """M.random_critic with its first layer's state rows scaled by M.state_scale (1 / (1 + mean |s_i|) per state column), so that
    p spreads over the lanes.  (Not test_gpu_safety_shield._matrix_nets' 20 / (1 + mean |s_i|): with M.random_critic's head of
    standard deviation 1/2 that saturates the sigmoid -- measured on the device: p is exactly 0 on more than half of
    SteelAnnealing's lanes and the gate's clipped p exactly 1 on four of the six envs, so a threshold at the median put every
    lane on one side.  With inputs of order one the logits are of order one and the probabilities are distinct floats.)"""
    cw, sc = M.random_critic(S, A, seed, n_out), M.state_scale(ni, key, SEED)
    return [(np.concatenate([cw[0][0][:S] * sc[:, None], cw[0][0][S:]]).astype(np.float32), cw[0][1]), cw[1], cw[2]]


NEUTRAL = dict(thr=2.0, umax=np.inf, tol=0.0)          # limits nothing reaches: the first run whose medians give the settings


def _install(ni, env, fam, key, cfg):
    from neorl_industrial_gym_amd.policies import ensemble_active_weights
    S, A = env.state_dim, env.action_dim
    if fam == "policy_disturbed":
        env.set_policy(ni.random_agent(S, A))
    elif fam.startswith("ens_"):
        members = [_actor(ni, key, S, A, 200 + 7 * k) for k in range(ENS_K)]
        thr = 0.2 if cfg is NEUTRAL else cfg["thr"]
        if fam == "ens_voting":
            env.set_mlp_ensemble(members, None, None, "voting", thr)
        else:
            aw, wsum = ensemble_active_weights(MEAN_W, ENS_K, "mean")
            env.set_mlp_ensemble(members, aw, wsum, "mean", thr)
    else:
        env.set_mlp_policy(_actor(ni, key, S, A, 5))
    if fam in ("safe", "search"):
        env.set_mlp_safety(_critic(ni, key, S, A, 6), cfg["thr"])
    elif fam == "gated":
        env.set_mlp_safety_ensemble([_critic(ni, key, S, A, 8 + m, n_out=GATE_C) for m in range(GATE_K)], 1.0, cfg["thr"], cfg["umax"])
    elif fam == "projected":
        env.set_mlp_constraint(_critic(ni, key, S, A, 10, n_out=GATE_C), cfg["thr"], cfg["tol"])
    elif fam.endswith("disturbed"):
        env.set_disturbance(ni.Disturbance(obs_noise=0.1, action_noise=0.1, hold="step"))


def _run(env, fam, limited, n=T):
    """One closed-loop launch of n steps of the family (its _limited twin) with every output: numpy arrays over the batch's
    lanes, the family's own rows under their names.  (obs_out / seen_out need B * S to be a multiple of 4: None otherwise.)"""
    B, S, A, ld, dev = env.batch, env.state_dim, env.action_dim, env.ld, env.device
    z = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device=dev)
    rew, fl, act = z(n, ld), z(n, ld, dtype=torch.int32), z(n, A, ld)
    xf = torch.full((n, ld), -1, dtype=torch.int32, device=dev)
    obs = z(n, B, S) if (B * S) % 4 == 0 else None
    if fam == "safe":
        rows, head = dict(prob=z(n, ld)), ()
    elif fam == "search":
        rows, head = dict(prob=z(n, ld), risk=z(n, ld), choice=z(n, ld, dtype=torch.int32)), (N_CAND,)
    elif fam == "gated":
        rows, head = dict(prob=z(n, GATE_C, ld), unc=z(n, GATE_C, ld), logit=z(n, GATE_K, GATE_C, ld)), ()
    elif fam == "projected":
        rows, head = dict(prob=z(n, GATE_C, ld), viol=z(n, GATE_C, ld), iters=z(n, ld, dtype=torch.int32), grad=z(n, A, ld)), (PROJ_ITERS, PROJ_STEP)
    elif fam.startswith("ens_"):
        rows, head = dict(unc=z(n, ld), mem=z(n, ENS_K, A, ld)), ()
    else:
        rows, head = dict(seen=obs if obs is None else z(n, B, S)), ()
    method = getattr(env, PARENT[fam] + ("_limited" if limited else ""))
    method(n, *head, rew, fl, obs, act, *rows.values(), *((xf,) if limited else ()))
    torch.cuda.synchronize()
    assert bool((xf[:, B:] == -1).all()), "xflags pad columns"
    out = dict(rew=rew[:, :B].cpu().numpy(), fl=fl[:, :B].cpu().numpy(), xf=xf[:, :B].cpu().numpy(), obs=None if obs is None else obs.cpu().numpy(),
               act=act[:, :, :B].cpu().numpy(), act_dev=act, rows={})
    for name, t in rows.items():
        out["rows"][name] = None if t is None else (t.cpu().numpy() if name == "seen" else t[..., :B].cpu().numpy())
    return out


def _the_action_the_env_stepped_on(fam, key, out):
    """[T, B, A]: act_out's rows; for the "mean" ensemble on an env that steps on the float64 action, that action rebuilt from
    the members' rows by the documented law (tests/test_gpu_ensemble.py::_the_step_took_that_action)."""
    if fam == "ens_mean" and key in ACT64:
        from neorl_industrial_gym_amd.policies import ensemble_action
        preds = np.ascontiguousarray(out["rows"]["mem"].transpose(1, 0, 3, 2))          # [K, T, B, A]
        a64 = ensemble_action(preds, MEAN_W, "mean")
        assert a64.dtype == np.float64 and np.array_equal(_bits(a64.astype(np.float32)), _bits(out["act"].transpose(0, 2, 1)))
        return a64
    return out["act"].transpose(0, 2, 1)


_CFG, _PARENT = {}, {}


def _medians(L, fam, o):
    """The family's settings from the rows of one parent launch: medians over the live lane-steps."""
    live = (o["fl"] & L.FLAG_INACTIVE) == 0
    r, cfg = o["rows"], dict(NEUTRAL)
    if fam in ("safe", "search"):
        cfg["thr"] = float(np.median(r["prob"][live]))
    elif fam == "gated":
        cfg["thr"] = float(np.median(r["prob"].max(axis=1)[live]))
        cfg["umax"] = float(np.quantile(r["unc"].max(axis=1)[live], 0.75))
    elif fam == "projected":
        pm = r["prob"].max(axis=1)[live].astype(np.float64)
        cfg["thr"] = float(np.median(pm))
        q = np.quantile(pm, 0.75)              # the tolerance: the upper quartile's logit -- about half of the projected
        cfg["tol"] = float(np.log(q / (1.0 - q)))      # lanes meet it without a step, the others walk
    else:
        cfg["thr"] = float(np.median(r["unc"][live]))
    assert np.isfinite(cfg["thr"]) and not np.isnan(cfg["umax"]) and np.isfinite(cfg["tol"]), cfg
    return cfg


def _cfg(ni, fam, key):
    """The family's settings for `key`: the medians of the PARENT's own rows over the live lane-steps of its B = 700 launch.
    A correction changes the trajectory it is decided on (a searched lane steps on a uniform candidate), so the parent's rows
    depend on the settings: the first launch runs with limits nothing reaches, the second with the first's medians, and the
    second's medians are the settings.  (Measured with the first launch's medians alone: SteelAnnealing's search corrected 0.909
    of the live steps under real limits -- its candidates drive the states to where the critic's p0 is higher.)
    The ensemble's threshold only sets a flag bit: both launches give the same median."""
    ck = (fam, key)
    if ck not in _CFG:
        cfg = NEUTRAL
        if fam in CORRECTS:
            for _ in range(2):
                env = _make(ni, key, M.B_BIG)
                _install(ni, env, fam, key, cfg)
                env.reset()
                cfg = _medians(ni._lib, fam, _run(env, fam, False))
                env.close()
        _CFG[ck] = dict(cfg)
    return _CFG[ck]


def _env(ni, fam, key, B, cons=(), autoreset=True):
    env = _make(ni, key, B, autoreset=autoreset, cons=cons)
    _install(ni, env, fam, key, _cfg(ni, fam, key))
    env.reset()
    return env


def _parent(ni, fam, key, B):
    """The parent family's launch at the family's settings on a fresh same-seed handle: computed once, left unchanged."""
    ck = (fam, key, B)
    if ck not in _PARENT:
        env = _env(ni, fam, key, B)
        out = _run(env, fam, False)
        out.pop("act_dev")
        out["handle"] = _handle(env)
        env.close()
        for v in list(out.values()) + list(out["rows"].values()):
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _PARENT[ck] = out
    return _PARENT[ck]


def _boxes(ni, fam, key, critical):
    par = _parent(ni, fam, key, M.B_BIG)
    S, A = par["obs"].shape[2], par["act"].shape[1]
    return _quantile_boxes(ni, par["obs"].reshape(-1, S), par["act"].transpose(0, 2, 1).reshape(-1, A), critical=critical)


def _same_outputs(got, par, keys):
    for k in keys:
        assert (got[k] is None and par[k] is None) or np.array_equal(_bits(got[k]), _bits(par[k])), k
    assert set(got["rows"]) == set(par["rows"])
    for k, v in got["rows"].items():
        assert (v is None and par["rows"][k] is None) or np.array_equal(v.view(np.uint32), par["rows"][k].view(np.uint32)), k


# ---- 1. inert limits are off -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [M.B_BIG, M.B_SMALL])
@pytest.mark.parametrize("fam,key", CASES)
def test_inert_limits_are_off(ni, fam, key, B):
    L = ni._lib
    par = _parent(ni, fam, key, B)
    probe = _make(ni, key, 1)
    cons = _inert(ni, probe.state_dim, probe.action_dim)
    probe.close()
    env = _env(ni, fam, key, B, cons=cons)
    got = _run(env, fam, True)
    h, ph = _handle(env), par["handle"]
    env.close()
    _same_outputs(got, par, ("rew", "fl", "obs", "act"))
    assert not got["xf"].any()
    for k in ("state", "ctr", "life", "ep_ret"):
        assert np.array_equal(h[k].view(np.uint8), ph[k].view(np.uint8)), k
    assert h["counter"] == ph["counter"]
    for r in range(L.T_ROWS):
        extra = 4 * ph["tally"][L.T_LEN_SUM] if r in (L.T_SATISFIED, L.T_CONSTRAINTS) else 0
        assert np.array_equal(h["tally"][r], ph["tally"][r] + extra), r
    assert ph["tally"][L.T_EPISODES].sum() > 0


# ---- 2. non-critical limits: the parent's trajectory, the Python law's bits ---------------------------------------------------------
@pytest.mark.parametrize("B", [M.B_BIG, M.B_SMALL])
@pytest.mark.parametrize("fam,key", CASES)
def test_noncritical_limits_keep_the_trajectory_and_match_the_python_law(ni, fam, key, B):
    L = ni._lib
    par = _parent(ni, fam, key, B)
    cons = _boxes(ni, fam, key, critical=False)
    env = _env(ni, fam, key, B, cons=cons)
    got = _run(env, fam, True)
    env.close()
    _same_outputs(got, par, ("fl", "obs", "act"))
    live = (got["fl"] & L.FLAG_INACTIVE) == 0
    assert live.all() and not ((got["xf"] >> 8) & 7).any()
    if got["obs"] is None:
        return
    act = _the_action_the_env_stepped_on(fam, key, got)
    one = act.dtype.type(1)
    clipped = np.clip(act, -one, one)
    assert clipped.dtype == act.dtype
    for k in range(T):
        xb = np.array([[0 if c.check_fn(s, a) else 1 for c in cons] for s, a in zip(got["obs"][k], clipped[k])], dtype=np.int64)
        want = (xb * (1 << np.arange(4))).sum(axis=1) | (xb.sum(axis=1) << 4)
        assert np.array_equal(got["xf"][k], want), (k, "xflags")
    if B == M.B_BIG:
        assert got["xf"].any()


# ---- 3. the limited loop is the limited step kernel ------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [M.B_BIG, M.B_SMALL])
@pytest.mark.parametrize("fam,key", CASES)
def test_the_limited_loop_is_the_limited_step_kernel(ni, fam, key, B):
    """A second same-seed handle with the same constraints takes the loop's actions step by step through env.step
    (nig_step_limited; nig_step64_limited on the float64 action where the env stepped on one)."""
    L = ni._lib
    cons = _boxes(ni, fam, key, critical=True)
    a, b = _env(ni, fam, key, B, cons=cons), _make(ni, key, B, cons=cons)
    b.reset()
    assert a.counter == b.counter
    out = _run(a, fam, True)
    act = _the_action_the_env_stepped_on(fam, key, out)
    mask = ~np.int32(L.FLAG_SHIELDED | L.FLAG_UNCERTAIN)
    for k in range(T):
        if act.dtype == np.float64:
            b.step(torch.from_numpy(np.ascontiguousarray(act[k])).to(b.device), layout="aos")
        else:
            b.step(out["act_dev"][k, :, :B], layout="soa")
        torch.cuda.synchronize()
        assert np.array_equal(_bits(b.reward.cpu().numpy()), _bits(out["rew"][k])), (k, "reward")
        assert np.array_equal(b.flags.cpu().numpy(), out["fl"][k] & mask), (k, "flags")
        assert np.array_equal(b.xflags.cpu().numpy(), out["xf"][k]), (k, "xflags")
        if k + 1 < T and out["obs"] is not None:
            assert np.array_equal(_bits(b.get_state().cpu().numpy()), _bits(out["obs"][k + 1])), (k, "state")
    ha, hb = _handle(a), _handle(b)
    a.close(); b.close()
    for k in ("state", "ctr", "life", "ep_ret"):
        assert np.array_equal(ha[k].view(np.uint8), hb[k].view(np.uint8)), k
    assert ha["counter"] == hb["counter"] and ha["tally"][L.T_EPISODES].sum() > 0
    _same_tally(L, ha["tally"], hb["tally"], "tally")
    if B == M.B_BIG:
        assert out["xf"].any() and ((out["xf"] >> 8) & 7).any()


# ---- 4. the correction still happens ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,key", [c for c in CASES if c[0] in CORRECTS])
def test_the_correction_still_happens_under_real_limits(ni, fam, key):
    L = ni._lib
    env = _env(ni, fam, key, M.B_BIG, cons=_boxes(ni, fam, key, critical=True))
    out = _run(env, fam, True)
    env.close()
    live = (out["fl"] & L.FLAG_INACTIVE) == 0
    share = float(((out["fl"] & getattr(L, CORRECTS[fam])) != 0)[live].mean())
    print(f"{fam} {key}: {CORRECTS[fam]} on {share:.3f} of the live steps; settings {_cfg(ni, fam, key)}")
    assert 0.1 <= share <= 0.9, share
    assert out["xf"].any()


# ---- 5. refusals and footprint -----------------------------------------------------------------------------------------------
def _calls(env, n, rew, fl, act, xf):
    return {
        "safe": lambda: env.rollout_mlp_safe_limited(n, rew, fl, None, act, None, xf),
        "search": lambda: env.rollout_mlp_search_limited(n, N_CAND, rew, fl, None, act, None, None, None, xf),
        "gated": lambda: env.rollout_mlp_gated_limited(n, rew, fl, None, act, None, None, None, xf),
        "projected": lambda: env.rollout_mlp_projected_limited(n, PROJ_ITERS, PROJ_STEP, rew, fl, None, act, None, None, None, None, xf),
        "ensemble": lambda: env.rollout_mlp_ensemble_limited(n, rew, fl, None, act, None, None, xf),
        "disturbed": lambda: env.rollout_mlp_disturbed_limited(n, rew, fl, None, act, None, xf),
        "policy_disturbed": lambda: env.rollout_policy_disturbed_limited(n, rew, fl, None, act, None, xf),
    }


def _fills(env):
    ld, A, dev = env.ld, env.action_dim, env.device
    return (torch.full((1, ld), -7.0, dtype=torch.float32, device=dev), torch.full((1, ld), 0x5A5A5A5B, dtype=torch.int32, device=dev),
            torch.full((1, A, ld), -7.0, dtype=torch.float32, device=dev), torch.full((1, ld), 0x3C3C3C3C, dtype=torch.int32, device=dev))


def _untouched(env, before, rew, fl, act, xf):
    torch.cuda.synchronize()
    after = _handle(env)
    assert after["counter"] == before["counter"]
    for k in ("state", "ctr", "life", "ep_ret", "tally"):
        assert np.array_equal(after[k].view(np.uint8), before[k].view(np.uint8)), k
    assert bool((rew == -7.0).all()) and bool((fl == 0x5A5A5A5B).all()) and bool((act == -7.0).all()) and bool((xf == 0x3C3C3C3C).all())


def test_refusals_launch_and_write_nothing(ni):
    INV, UNS = 1, 4
    band = ni.BoxConstraint("band", {("action", 0): (-0.5, 0.5)}, -1.0)
    # no limits installed: NIG_ERR_INVALID, whatever else is installed
    env = _make(ni, "cr", M.B_SMALL)
    S, A = env.state_dim, env.action_dim
    env.set_policy(ni.random_agent(S, A)); env.set_mlp_policy(M.random_actor(S, A, 5)); env.set_mlp_safety(M.random_critic(S, A, 6), 0.5)
    env.set_mlp_ensemble([M.random_actor(S, A, 5), M.random_actor(S, A, 7)], None, None, "voting", 0.2)
    env.set_mlp_safety_ensemble([M.random_critic(S, A, 8, n_out=2), M.random_critic(S, A, 9, n_out=2)], 1.0, 0.5, 0.2)
    env.set_mlp_constraint(M.random_critic(S, A, 10, n_out=2), 0.1, 0.01)
    env.set_disturbance(ni.Disturbance(obs_noise=0.1, action_noise=0.1, hold="step"))
    env.reset()
    bufs = _fills(env)
    before = _handle(env)
    for name, call in _calls(env, 1, *bufs).items():
        assert _code(ni, call) == INV, name
        assert "no limits installed" in env._L.nig_last_error().decode(), name
    _untouched(env, before, *bufs)
    # ... and with them every twin runs
    env.add_safety_constraint(band)
    for name, call in _calls(env, 1, *bufs).items():
        assert _code(ni, call) == 0, name
    torch.cuda.synchronize()
    assert env.counter == before["counter"] + 7 and bool((bufs[3][0, :M.B_SMALL] != 0x3C3C3C3C).all())
    env.close()
    # limits installed, the parent's prerequisites missing: the parent's code
    env = _make(ni, "cr", M.B_SMALL, cons=[band])
    env.reset()
    bufs = _fills(env)
    before = _handle(env)
    for name, call in _calls(env, 1, *bufs).items():
        assert _code(ni, call) == INV, name              # no actor / policy / ensemble installed
    env.set_mlp_policy(M.random_actor(S, A, 5)); env.set_policy(ni.random_agent(S, A))
    want = {"safe": "no safety critic", "search": "no safety critic", "gated": "no safety ensemble", "projected": "no constraint predictor",
            "ensemble": "no ensemble", "disturbed": "no disturbance", "policy_disturbed": "no disturbance"}
    for name, call in _calls(env, 1, *bufs).items():
        assert _code(ni, call) == INV and want[name] in env._L.nig_last_error().decode(), name
    env.set_mlp_safety(M.random_critic(S, A, 6), 0.5); env.set_mlp_constraint(M.random_critic(S, A, 10, n_out=2), 0.1, 0.01)
    rew, fl, act, xf = bufs
    assert _code(ni, lambda: env.rollout_mlp_search_limited(1, 0, rew, fl, None, act, None, None, None, xf)) == INV
    assert _code(ni, lambda: env.rollout_mlp_projected_limited(1, 0, 0.1, rew, fl, None, act, None, None, None, None, xf)) == INV
    _untouched(env, before, *bufs)
    env.close()
    # WaterTreatment has no MFMA actor: the MFMA twins refuse as their parents do, the policy twin runs
    env = _make(ni, "water", M.B_SMALL, cons=[band])
    env.set_policy(ni.random_agent(env.state_dim, env.action_dim))
    env.set_disturbance(ni.Disturbance(obs_noise=0.1, action_noise=0.1, hold="step"))
    env.reset()
    bufs = _fills(env)
    before = _handle(env)
    calls = _calls(env, 1, *bufs)
    for name in ("safe", "search", "gated", "projected", "ensemble", "disturbed"):
        assert _code(ni, calls[name]) == UNS, name
    _untouched(env, before, *bufs)
    assert _code(ni, calls["policy_disturbed"]) == 0
    env.close()
    # the Advanced pair takes no limits (nig_set_limits refuses): every twin stops at "no limits installed"
    for name in ("AdvancedChemicalReactor-v0", "AdvancedPowerGrid-v0"):
        env = ni.make_batched(name, M.B_SMALL, seed=SEED, tally=True)
        env.set_policy(ni.random_agent(env.state_dim, env.action_dim)); env.set_mlp_policy(M.random_actor(env.state_dim, env.action_dim, 5))
        env.set_disturbance(ni.Disturbance(obs_noise=0.1, action_noise=0.1, hold="step"))
        env.reset()
        bufs = _fills(env)
        before = _handle(env)
        for fam, call in _calls(env, 1, *bufs).items():
            assert _code(ni, call) == INV, (name, fam)
        _untouched(env, before, *bufs)
        env.close()


@pytest.mark.parametrize("mode", ["odd", "tight"])
@pytest.mark.parametrize("entry", ["safe", "search", "gated", "projected", "ensemble", "disturbed", "policy_disturbed"])
def test_footprint_of_the_limited_twins(ni, entry, mode):
    """tests/footprint.py arenas around every caller buffer, on a handle without auto-reset with held lanes
    (test_gpu_limits.test_footprint_of_the_limited_entry_points' rig): pad columns, stride gaps, rows beyond n_steps and the rows
    of frozen lanes keep the canary, xflags included (a frozen lane's xflags word is written: 0)."""
    from test_gpu_footprint import Rig, ceil4, clean, gap, pitch
    key, B, n = "cr", 321, 3
    r = Rig(ni, key, B, autoreset=False, max_steps=2)
    S, A, ld, L, lib = r.S, r.A, r.ld, ni._lib, r.L
    r.env.add_safety_constraint(ni.BoxConstraint("trip", {("action", 0): (-0.6, 0.6), ("state", 0): (-np.inf, np.inf)}, -5.0, critical=True))
    e = r.env
    e.set_policy(ni.random_agent(S, A)); e.set_mlp_policy(M.random_actor(S, A, 11)); e.set_mlp_safety(M.random_critic(S, A, 12), 0.5)
    e.set_mlp_ensemble([M.random_actor(S, A, 11), M.random_actor(S, A, 13)], None, None, "voting", 0.2)
    e.set_mlp_safety_ensemble([M.random_critic(S, A, 14, n_out=2), M.random_critic(S, A, 15, n_out=2)], 1.0, 0.5, 0.2)
    e.set_mlp_constraint(M.random_critic(S, A, 16, n_out=2), 0.1, 0.01)
    e.set_disturbance(ni.Disturbance(obs_noise=0.1, action_noise=0.1, hold="step"))
    a = Arena("cuda")
    os_, lda = pitch(mode, B, ld, 1), pitch(mode, B, ld, 2)
    rew = a.add("reward_out", "f32", Layout(n, os_, 1, os_, B))
    fl = a.add("flags_out", "flags", Layout(n, os_, 1, os_, B))
    xf = a.add("xflags_out", "flags", Layout(n, os_, 1, os_, B))
    obs = a.add("obs_out", "f32", Layout(n, ceil4(B * S) + gap(mode, 1, mult4=True), 1, B * S, B * S, lane_width=S), align=16)
    act = a.add("act_out", "f32", Layout(n, A * lda + gap(mode, 2), A, lda, B))
    a.build()
    r.reset()
    hold = torch.arange(1, B, 5, device="cuda")
    r.hold(hold)
    p = lambda b: C.c_void_p(b.ptr)
    a.freeze_inputs()
    shared = (p(rew), p(fl), os_, p(obs), obs.layout.outer_stride, p(act), lda, act.layout.outer_stride)
    N = None
    rc = {"safe": lambda: lib.nig_rollout_mlp_safe_limited(r.h, n, *shared, N, p(xf), r.st()),
          "search": lambda: lib.nig_rollout_mlp_search_limited(r.h, n, N_CAND, *shared, N, N, N, p(xf), r.st()),
          "gated": lambda: lib.nig_rollout_mlp_gated_limited(r.h, n, *shared, N, N, N, 0, 0, p(xf), r.st()),
          "projected": lambda: lib.nig_rollout_mlp_projected_limited(r.h, n, PROJ_ITERS, PROJ_STEP, *shared, N, N, N, N, 0, 0, p(xf), r.st()),
          "ensemble": lambda: lib.nig_rollout_mlp_ensemble_limited(r.h, n, *shared, N, N, p(xf), r.st()),
          "disturbed": lambda: lib.nig_rollout_mlp_disturbed_limited(r.h, n, *shared, N, 0, p(xf), r.st()),
          "policy_disturbed": lambda: lib.nig_rollout_policy_disturbed_limited(r.h, n, *shared, N, 0, p(xf), r.st())}[entry]()
    assert rc == 0, lib.nig_last_error()
    torch.cuda.synchronize()
    f = fl.rows(n)[:, 0]
    live = (f & L.FLAG_INACTIVE) == 0
    assert not bool(live[0][hold].any()) and bool(live[0].sum() == B - len(hold)) and not bool(live[-1].any())
    assert bool((xf.rows(n)[:, 0][~live] == 0).all())
    written = {b.name: dict(n_outer=n) for b in (rew, fl, xf)}
    written.update({b.name: dict(n_outer=n, live=live) for b in (obs, act)})
    clean([str(x) for x in a.check(written)] + r.workspace_findings(), f"{entry} {mode}")
    r.close()


# ---- 6. end to end -----------------------------------------------------------------------------------------------------------
def _sums_of_the_rows(L, out):
    """evaluate_with_safety's integer aggregates and the per-episode returns from the flags + xflags + reward rows of a launch
    without auto-reset (ChemicalReactor: the episode return is the float32 sum of the float32 rewards, nig_episode.hpp)."""
    fl, xf = out["fl"], out["xf"]
    live = (fl & L.FLAG_INACTIVE) == 0
    viol = ((((fl >> L.FLAG_NVIOL_SHIFT) & 3) + ((xf >> 4) & 7)) * live).sum()
    crit = ((((fl >> L.FLAG_NCRIT_SHIFT) & 3) + ((xf >> 8) & 7)) * live).sum()
    shut = (((fl & L.FLAG_SHUTDOWN) != 0) & live).sum()
    ret = np.zeros(fl.shape[1], np.float32)
    for k in range(fl.shape[0]):
        ret = np.where(live[k], ret + out["rew"][k], ret).astype(np.float32)
    assert (((fl & (L.FLAG_TERMINATED | L.FLAG_TRUNCATED)) != 0) & live).sum(axis=0).min() == 1, "every episode ends inside the launch"
    return dict(safety_violations=int(viol), critical_violations=int(crit), emergency_shutdowns=int(shut),
                successful_episodes=int((ret > 0).sum())), ret.astype(np.float64)


def test_evaluate_with_safety_runs_the_shielded_agent_on_the_device_under_added_constraints(ni, monkeypatch):
    from neorl_industrial_gym_amd.policies import MLPPolicy, pad_critic
    L, key, B = ni._lib, "cr", M.B_BIG
    cons = _boxes(ni, "safe", key, critical=True)
    thr = _cfg(ni, "safe", key)["thr"]
    probe = _make(ni, key, 1)
    S, A = probe.state_dim, probe.action_dim
    probe.close()
    ws, cw = _actor(ni, key, S, A, 5), _critic(ni, key, S, A, 6)
    agent = MLPPolicy(ws, safety_weights=cw, constraint_threshold=thr).shielded()
    env = _make(ni, key, B, autoreset=False, cons=cons)
    taken = []
    real = env.rollout_mlp_safe_limited
    monkeypatch.setattr(env, "rollout_mlp_safe_limited", lambda *a, **k: (taken.append(a[0]), real(*a, **k))[1])
    got = ni.evaluate_with_safety(agent, env, n_episodes=B)
    env.close()
    assert taken == [MAXS], "one fused launch of the shield's limited twin"
    man = _make(ni, key, B, autoreset=False, cons=cons)
    man.set_mlp_policy(ws); man.set_mlp_safety(pad_critic(cw), thr)
    man.reset()
    want, ret = _sums_of_the_rows(L, _run(man, "safe", True, n=MAXS))
    man.close()
    for k, v in want.items():
        assert got[k] == v, (k, got[k], v)
    assert want["safety_violations"] > 0 and want["critical_violations"] > 0
    assert abs(got["return_mean"] - ret.mean()) <= 1e-12 * abs(ret.mean())


def test_evaluate_robustness_keeps_the_added_constraints_and_stays_fused(ni):
    from neorl_industrial_gym_amd.policies import MLPPolicy
    L, key, B = ni._lib, "cr", M.B_BIG
    cons = _boxes(ni, "disturbed", key, critical=True)
    probe = _make(ni, key, 1)
    S, A = probe.state_dim, probe.action_dim
    probe.close()
    ws = _actor(ni, key, S, A, 5)
    env = _make(ni, key, B, autoreset=False, cons=cons)
    got = ni.evaluate_robustness(MLPPolicy(ws), env, n_episodes=B, noise_levels=(0.1,), disturbance_types=("observation_noise",), hold="step")
    env.close()
    assert got["path"] == "fused-mlp"
    cell = got["robustness_results"]["observation_noise"][0.1]
    # the cell by hand: a fresh same-seed handle with the constraints, the wrapper's disturbance, one launch of the twin
    man = _make(ni, key, B, autoreset=False, cons=cons)
    man.set_mlp_policy(ws)
    man.set_disturbance(ni.Disturbance(obs_noise=0.1, hold="step"))
    man.reset()
    out = _run(man, "disturbed", True, n=MAXS)
    want, ret = _sums_of_the_rows(L, out)
    man.close()
    assert ((out["xf"] >> 4) & 7).any(), "the added constraints count"
    assert cell["safety_violations"] == want["safety_violations"] > 0
    assert abs(cell["mean_return"] - ret.mean()) <= 1e-12 * abs(ret.mean())
