"""-m gpu: the distributional safety critic on the device ("nig-categorical-v1", include/nig.h): nig_mlp_violation_prob, and
nig_rollout_mlp_safe / nig_rollout_mlp_search and their _limited twins with the categorical critic in the handle's critic slot.

The reference's DistributionalSafetyCritic cannot run here (jax / flax are absent), so there is no golden fixture from it.  The
logits are held to the CPU oracle's one-output critic column by column; p is held bit for bit to the law restated in NumPy
(tests/categorical_ref.py) on the device's own logits and, within the radius derived in categorical_ref.radius, to a float64
NumPy restatement of the reference's lines (agents/safety_critical.py:151-171); the closed loops are held to the evaluator.

Shapes: closed_loop_matrix's B = 700 (five full 128-env blocks and a partial one) and B = 5 (one partial wave), episodes of at
most 5 steps in launches of T = 6 (lanes freeze or reset inside a launch), 3 search candidates; 51 atoms (the reference's) on
all eight MFMA envs, and 2, 16, 17, 64 atoms -- the edges of the four 16-row head passes -- on ChemicalReactor (one-chunk critic
layer 1) and PowerGrid (two chunks).  The evaluator, the shield and the search run over that whole matrix; the _limited twins over
the six envs that accept added constraints at 51 atoms and over the eight edge cases; the non-finite biases on all eight envs at 51
atoms; the slot and the isolation tests, which hold the host's bookkeeping and not a kernel shape, on ChemicalReactor and PowerGrid."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import categorical_ref as R
import closed_loop_matrix as M
import handle_lifecycle as H

pytestmark = pytest.mark.gpu

T, MAXS, SEED, NC = 6, M.MAXS_NEW, 0x5EED, 3
f32 = np.float32
ALL51 = [(k, 51) for k, _ in M.MFMA_ENVS]
EDGES = [(k, n) for k in ("cr", "pg") for n in (2, 16, 17, 64)]
LIM51 = [(k, 51) for k, _ in M.MFMA_ENVS if k not in M.CLONED]      # (the Advanced pair takes no added constraints: no twin)
OUT = ("act", "obs", "reward", "flags", "prob", "risk", "choice")
FIDELITY = {}


@pytest.fixture(scope="module")
def ni():
    import neorl_industrial_gym_amd as ni
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return ni


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32) if x.dtype == np.float32 else x


@functools.lru_cache(maxsize=None)
def _nets(ni, key, atoms):
    """The lifecycle tests' actor; a categorical critic whose state rows are scaled by the observed magnitudes (their critic's
    construction), so that p spreads over the lanes; the default mask of `atoms` atoms on [-1, 1]."""
    probe = ni.make_batched(M.NAMES[key], 1)
    S, A = probe.state_dim, probe.action_dim
    probe.close()
    ws = H.actor(ni, key, S, A, 5)
    cw, sc = R.random_categorical_critic(S, A, atoms, 60 + atoms), M.state_scale(ni, key, SEED)
    # (gain 20 on both parts of the input, test_gpu_safe_action_search.py's construction: the lanes' states lie close together --
    # AdvancedChemicalReactor's p spanned 0.008 without it, half of the 700 colliding in float32 -- and the candidates must differ in p)
    cw = [(np.concatenate([cw[0][0][:S] * f32(20.0) * sc[:, None], cw[0][0][S:] * f32(20.0)]).astype(f32), cw[0][1]), cw[1], cw[2]]
    return ws, cw, R.default_mask(atoms), S, A


def _make(ni, key, B, autoreset=True, cons=()):
    env = ni.make_batched(M.NAMES[key], B, seed=SEED, autoreset=autoreset, tally=True, max_episode_steps=MAXS)
    for c in cons:
        env.add_safety_constraint(c)
    return env


def _start(ni, env, key, t0=0):
    env.counter = t0
    env.reset()
    M.install_start(ni, env, key, SEED)


def _launch(ni, env, entry, n=T, limited=False):
    """One launch of n steps of nig_rollout_mlp_safe / _search (its _limited twin) through the C entry points, with every output.
    (An observation step is a multiple of 4 floats: where B * S is none, the rows are padded.)"""
    B, S, A, ld, dev = env.batch, env.state_dim, env.action_dim, env.ld, env.device
    ostep = (B * S + 3) // 4 * 4
    z = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device=dev)
    act, obs, fl, rw, pr, rk = z(n, A, ld), z(n, ostep), z(n, ld, dtype=torch.int32), z(n, ld), z(n, ld), z(n, ld)
    ch = z(n, ld, dtype=torch.int32)
    xf = torch.full((n, ld), -1, dtype=torch.int32, device=dev)
    p = lambda x: C.c_void_p(x.data_ptr())
    L = ni._lib.lib()
    common = (p(rw), p(fl), ld, p(obs), ostep, p(act), ld, A * ld, p(pr))
    t_before = env.counter
    with torch.cuda.device(dev):
        if entry == "search":
            fn = L.nig_rollout_mlp_search_limited if limited else L.nig_rollout_mlp_search
            args = (env._h, n, NC) + common + (p(rk), p(ch)) + ((p(xf),) if limited else ()) + (env._stream(),)
        else:
            fn = L.nig_rollout_mlp_safe_limited if limited else L.nig_rollout_mlp_safe
            args = (env._h, n) + common + ((p(xf),) if limited else ()) + (env._stream(),)
        ni._lib.check(fn(*args))
    torch.cuda.synchronize()
    assert env.counter == t_before + n
    o = dict(act=act[:, :, :B].permute(0, 2, 1).cpu().numpy(), obs=obs[:, :B * S].reshape(n, B, S).cpu().numpy(), flags=fl[:, :B].cpu().numpy(),
             reward=rw[:, :B].cpu().numpy(), prob=pr[:, :B].cpu().numpy(), risk=rk[:, :B].cpu().numpy(), choice=ch[:, :B].cpu().numpy(),
             xf=xf[:, :B].cpu().numpy(), act_dev=act, t0=t_before)
    o["live"] = (o["flags"] & ni._lib.FLAG_INACTIVE) == 0
    o["shielded"] = (o["flags"] & ni._lib.FLAG_SHIELDED) != 0
    return o


def _handle(env):
    torch.cuda.synchronize()
    return dict(state=env.get_state().cpu().numpy(), ctr=env.ctr.cpu().numpy(), life=env.life_viol.cpu().numpy(),
                ep_ret=env.ep_return.cpu().numpy(), tally=env.tally.cpu().numpy(), counter=env.counter)


def _run(ni, key, atoms, B, entry, thr, limited=False, cons=(), cw=None, autoreset=True):
    """A fresh same-seed handle with the actor and the categorical critic, one launch of T steps.  Returns (env, outputs + handle)."""
    ws, cw0, mask, S, A = _nets(ni, key, atoms)
    env = _make(ni, key, B, autoreset=autoreset, cons=cons)
    env.set_mlp_policy(ws)
    env.set_mlp_safety_categorical(cw0 if cw is None else cw, thr, mask)
    assert env.mlp_safety_kind == ni._lib.SAFETY_CATEGORICAL
    _start(ni, env, key)
    o = _launch(ni, env, entry, limited=limited)
    o["handle"] = _handle(env)
    return env, o


def _same(a, b, what, lanes=slice(None), keys=OUT, handle=True):
    for k in keys:
        assert np.array_equal(_bits(a[k][:, lanes]), _bits(b[k][:, lanes])), (what, k)
    if handle:
        for k in ("state", "ctr", "life", "ep_ret"):
            assert np.array_equal(a["handle"][k][lanes].view(np.uint8), b["handle"][k][lanes].view(np.uint8)), (what, k)
        assert a["handle"]["counter"] == b["handle"]["counter"], what
        assert np.array_equal(a["handle"]["tally"][:, lanes].view(np.uint8), b["handle"]["tally"][:, lanes].view(np.uint8)), (what, "tally")


@functools.lru_cache(maxsize=None)
def _neutral(ni, key, atoms):
    """The shield launch at a threshold no p reaches (2.0) on B = 700: the start observations, the raw actions and the p the
    other tests take their inputs and thresholds from.  Computed once, left unchanged."""
    env, o = _run(ni, key, atoms, M.B_BIG, "safe", 2.0)
    env.close()
    o.pop("act_dev")
    assert o["live"][0].all() and not o["shielded"].any()
    for v in o.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return o


def _evaluate(ni, env, obs, act, atoms, pad=5):
    """env.violation_prob on n rows, with canary words behind the outputs: (p [n], logits [atoms, n])."""
    n = obs.shape[0]
    dev = env.device
    pr = torch.full((n + pad,), 7.5, dtype=torch.float32, device=dev)
    zz = torch.full((atoms + 1, n + pad), 7.5, dtype=torch.float32, device=dev)
    got = env.violation_prob(torch.from_numpy(np.array(obs, dtype=f32)).to(dev), torch.from_numpy(np.array(act, dtype=f32)).to(dev), pr, zz)
    torch.cuda.synchronize()
    assert got.data_ptr() == pr.data_ptr() and got.shape == (n,)
    assert bool((pr[n:] == 7.5).all()) and bool((zz[:, n:] == 7.5).all()) and bool((zz[atoms:] == 7.5).all()), "pad columns / rows keep their words"
    return pr[:n].cpu().numpy(), zz[:atoms, :n].cpu().numpy()


@functools.lru_cache(maxsize=None)
def _evaluated(ni, oracle, key, atoms):
    """The evaluator on step 0's 700 (observation, raw action) pairs, and the oracle's p of every head column as a one-output
    critic on the same pairs: computed once per case and shared."""
    ws, cw, mask, S, A = _nets(ni, key, atoms)
    o = _neutral(ni, key, atoms)
    obs = np.array(o["obs"][0])
    raw = oracle.mlp_actions(key, ws, obs)
    assert np.array_equal(_bits(raw), _bits(o["act"][0])), "the raw action is nig_rollout_mlp's (the oracle's)"
    env = _make(ni, key, 8)
    env.set_mlp_safety_categorical(cw, 0.5, mask)
    p, z = _evaluate(ni, env, obs, raw, atoms)
    small = {n: _evaluate(ni, env, obs[:n], raw[:n], atoms) for n in (M.B_SMALL, 1)}
    env.close()
    cols = np.stack([oracle.mlp_critic(key, [cw[0], cw[1], (cw[2][0][:, j:j + 1].copy(), cw[2][1][j:j + 1].copy())], obs, raw) for j in range(atoms)])
    for a in (p, z, cols, obs, raw):
        a.setflags(write=False)
    return dict(obs=obs, raw=raw, p=p, z=z, small=small, cols=cols)


# ---- 1, 2. the evaluator ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,atoms", ALL51 + EDGES)
def test_evaluator_logits_are_the_oracles_columns(ni, oracle, key, atoms):
    """det_sigmoidf(logit_out[j]) is bit for bit oracle.mlp_critic of the one-output critic (C3[:, j], c3[j]) for every j < N on
    700 columns; n = 5 and n = 1 give the first columns of that launch (a lane does not depend on its neighbours); the pad
    columns of both outputs and the row behind the last atom keep their words (_evaluate)."""
    e = _evaluated(ni, oracle, key, atoms)
    sig = oracle.detmath_unary("sigmoidf", e["z"].ravel()).reshape(e["z"].shape)
    assert np.array_equal(_bits(sig), _bits(e["cols"]))
    assert np.isfinite(e["z"]).all() and M.distinct_rows(e["z"].T) >= 600
    for n, (p, z) in e["small"].items():
        assert np.array_equal(_bits(p), _bits(e["p"][:n])) and np.array_equal(_bits(z), _bits(e["z"][:, :n])), n


@pytest.mark.parametrize("key,atoms", ALL51 + EDGES)
def test_evaluator_probability_is_the_law(ni, oracle, key, atoms):
    """prob_out is bit for bit categorical_ref.violation_prob on the device's own logit_out, and within categorical_ref.radius
    (derived there, not tuned) of the float64 softmax mass on those logits.  The seeds give at least 600 distinct, unsaturated p
    over the 700 start states, by the float64 network too (closed_loop_matrix.mlp64)."""
    ws, cw, mask, S, A = _nets(ni, key, atoms)
    e = _evaluated(ni, oracle, key, atoms)
    assert R.same_bits(e["p"], R.violation_prob(oracle, e["z"], mask))
    want = R.mass64(e["z"], mask)
    worst = float(np.abs(e["p"].astype(np.float64) - want).max() / R.radius(atoms))
    print(f"{key} atoms={atoms}: |p - float64 mass| / radius({atoms}) = {worst:.3g}")
    FIDELITY[(key, atoms)] = worst
    assert worst <= 1.0
    p64 = R.mass64(M.mlp64(cw, np.concatenate([e["obs"], e["raw"]], axis=1)).T, mask)
    assert len(np.unique(p64)) >= 600 and 1e-3 < p64.min() and p64.max() < 1 - 1e-3, (len(np.unique(p64)), p64.min(), p64.max())
    assert np.abs(e["p"] - p64).max() <= 1e-3, "the device's network is the float64 network's, to float32 accuracy"
    out = os.environ.get("NIG_CATEGORICAL_FIDELITY")           # profiles/bench_categorical.py's companion record (profiles/categorical/fidelity.txt)
    if out and len(FIDELITY) == len(ALL51 + EDGES):
        with open(out, "w") as f:
            f.write("worst |prob_out - float64 softmax mass on the device's logits| / categorical_ref.radius(atoms), 700 columns per case\n")
            for (k, n), w in FIDELITY.items():
                f.write(f"{k:7s} atoms {n:2d}  radius {R.radius(n):.3e}  worst / radius {w:.4f}\n")


# ---- 3. the shield ----------------------------------------------------------------------------------------------------------------
def _median(ni, key, atoms):
    p = _neutral(ni, key, atoms)["prob"][0]
    med = float(np.median(p))
    # (the float64 p of the 700 lanes are distinct -- test_evaluator_probability_is_the_law -- but half of AdvancedChemicalReactor's
    # lanes lie within a few float32 steps of each other, so the float32 p are asked only not to pile up on one side of the median)
    assert (p < med).mean() >= 0.25 and (p >= med).mean() >= 0.25 and len(np.unique(p)) >= 300
    return med


def _check_shield(ni, oracle, key, atoms, o, thr):
    """Every live step against the shield's law with p from the evaluator on the recorded observation and the oracle's raw action."""
    ws, cw, mask, S, A = _nets(ni, key, atoms)
    ev = _make(ni, key, 8)
    ev.set_mlp_safety_categorical(cw, 0.5, mask)
    for k in range(T):
        lv = o["live"][k]
        raw = oracle.mlp_actions(key, ws, o["obs"][k])
        p, _ = _evaluate(ni, ev, o["obs"][k], raw, atoms)
        assert R.same_bits(o["prob"][k][lv], p[lv]), (k, "prob")
        with np.errstate(invalid="ignore"):
            keep = p < f32(thr)
        want = np.where(keep[:, None], raw, raw * f32(0.5))
        assert np.array_equal(_bits(o["act"][k])[lv], _bits(want)[lv]), (k, "act")
        assert np.array_equal(o["shielded"][k], lv & ~keep), (k, "FLAG_SHIELDED")
    ev.close()


@pytest.mark.parametrize("B", [M.B_BIG, M.B_SMALL])
@pytest.mark.parametrize("key,atoms", ALL51 + EDGES)
def test_shield_acts_on_the_categorical_p(ni, oracle, key, atoms, B):
    """rollout_mlp_safe with the categorical critic at the median p of step 0: prob_out[k] is bit for bit violation_prob(obs_out[k],
    raw action), the raw action oracle.mlp_actions on obs_out[k]; the env received a where p < thr and a * 0.5 elsewhere, with
    FLAG_SHIELDED; each branch holds at least a quarter of the live lanes of step 0 (B = 700), so both share waves; and
    check_env_steps holds the plant to the oracle on the rollout's own actions."""
    thr = _median(ni, key, atoms)
    env, o = _run(ni, key, atoms, B, "safe", thr)
    env.close()
    _check_shield(ni, oracle, key, atoms, o, thr)
    if B == M.B_BIG:
        sh, lv = o["shielded"][0], o["live"][0]
        assert lv.all() and sh.mean() >= 0.25 and (~sh).mean() >= 0.25, sh.mean()
        assert any((sh[w:w + 64].any() and not sh[w:w + 64].all()) for w in range(0, 640, 64)), "both branches share a wave"
    assert M.check_env_steps(oracle, ni._lib, key, o["obs"], o["act"], o["flags"], SEED, MAXS) > 0 or key == "apg"
    assert not o["live"].all() or o["handle"]["tally"][ni._lib.T_EPISODES].sum() > 0      # (episodes end inside the launch)


# ---- 4. the search ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [M.B_BIG, M.B_SMALL])
@pytest.mark.parametrize("key,atoms", ALL51 + EDGES)
def test_search_above_one_is_the_categorical_shield(ni, key, atoms, B):
    """At a threshold above 1 no lane searches: act, obs, reward, flags, prob, the final state, counters and tallies are bit for
    bit rollout_mlp_safe's with the same critic; choice is -1 and risk is prob on live steps."""
    env, o = _run(ni, key, atoms, B, "search", 2.0)
    env.close()
    env, r = _run(ni, key, atoms, B, "safe", 2.0)
    env.close()
    live = o["live"]
    assert (o["choice"][live] == -1).all() and (o["choice"][~live] == 0).all() and not o["shielded"].any()
    assert np.array_equal(_bits(o["risk"]), _bits(o["prob"]))
    _same(o, r, "search at 2.0 vs shield at 2.0", keys=("act", "obs", "reward", "flags", "prob"))


@pytest.mark.parametrize("B", [M.B_BIG, M.B_SMALL])
@pytest.mark.parametrize("key,atoms", ALL51 + EDGES)
def test_search_at_zero_takes_the_first_least_p(ni, oracle, key, atoms, B):
    """At threshold 0 every live lane searches: choice / risk / action are the first least p among policies.search_candidates'
    draws, each p bit for bit violation_prob of that candidate on the recorded observation; prob is the raw action's p."""
    from neorl_industrial_gym_amd.policies import search_candidates
    from test_gpu_safe_action_search import _first_min
    ws, cw, mask, S, A = _nets(ni, key, atoms)
    env, o = _run(ni, key, atoms, B, "search", 0.0)
    env.close()
    ev = _make(ni, key, 8)
    ev.set_mlp_safety_categorical(cw, 0.5, mask)
    assert np.array_equal(o["shielded"], o["live"])
    for k in range(T):
        idx = np.nonzero(o["live"][k])[0]
        if idx.size == 0:
            continue
        obs = o["obs"][k][idx]
        p0, _ = _evaluate(ni, ev, obs, oracle.mlp_actions(key, ws, obs), atoms)
        assert R.same_bits(o["prob"][k][idx], p0), (k, "prob")
        cand = np.stack([search_candidates(SEED, int(i), k + 1, NC, A) for i in idx])                 # [n, NC, A]
        pc, _ = _evaluate(ni, ev, np.repeat(obs, NC, axis=0), cand.reshape(idx.size * NC, A), atoms)
        best, pb = _first_min(pc.reshape(idx.size, NC))
        assert np.array_equal(o["choice"][k][idx], best), (k, "choice")
        assert np.array_equal(_bits(o["risk"][k][idx]), _bits(pb.astype(f32))), (k, "risk")
        assert np.array_equal(_bits(o["act"][k][idx]), _bits(cand[np.arange(idx.size), best])), (k, "action")
    ev.close()
    if B == M.B_BIG:
        assert len(np.unique(o["choice"][o["live"]])) == NC, "every candidate wins somewhere"
    M.check_env_steps(oracle, ni._lib, key, o["obs"], o["act"], o["flags"], SEED, MAXS)


# ---- 5. the _limited twins --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [M.B_BIG, M.B_SMALL])
@pytest.mark.parametrize("entry", ["safe", "search"])
@pytest.mark.parametrize("key,atoms", LIM51 + EDGES)
def test_inert_limits_are_the_parents(ni, key, atoms, entry, B):
    from test_gpu_limits import _inert
    L = ni._lib
    ws, cw, mask, S, A = _nets(ni, key, atoms)
    thr = _median(ni, key, atoms)
    env, par = _run(ni, key, atoms, B, entry, thr)
    env.close()
    env, got = _run(ni, key, atoms, B, entry, thr, limited=True, cons=_inert(ni, S, A))
    env.close()
    _same(got, par, "inert limits", handle=False)
    assert not got["xf"].any() and (par["shielded"].any() or B == M.B_SMALL)
    for k in ("state", "ctr", "life", "ep_ret"):
        assert np.array_equal(got["handle"][k].view(np.uint8), par["handle"][k].view(np.uint8)), k
    for r in range(L.T_ROWS):
        extra = 4 * par["handle"]["tally"][L.T_LEN_SUM] if r in (L.T_SATISFIED, L.T_CONSTRAINTS) else 0
        assert np.array_equal(got["handle"]["tally"][r], par["handle"]["tally"][r] + extra), r


@pytest.mark.parametrize("entry", ["safe", "search"])
@pytest.mark.parametrize("key,atoms", LIM51 + EDGES)
def test_a_live_limit_is_the_limited_step_on_act_out(ni, key, atoms, entry):
    """One live critical constraint on the first action: a second same-seed handle with the same constraint takes the loop's
    act_out step by step through env.step (nig_step_limited) and gives the loop's rewards, flags, xflags and next states."""
    L = ni._lib
    ws, cw, mask, S, A = _nets(ni, key, atoms)
    a0 = _neutral(ni, key, atoms)["act"][..., 0].astype(np.float64)
    cons = [ni.BoxConstraint("band", {("action", 0): (f32(np.quantile(a0, 0.3)), f32(np.quantile(a0, 0.7)))}, -6.0, critical=True)]
    a, out = _run(ni, key, atoms, M.B_BIG, entry, _median(ni, key, atoms), limited=True, cons=cons)
    b = _make(ni, key, M.B_BIG, cons=cons)
    _start(ni, b, key)
    mask_bits = ~np.int32(L.FLAG_SHIELDED | L.FLAG_UNCERTAIN)
    for k in range(T):
        b.step(out["act_dev"][k, :, :M.B_BIG], layout="soa")
        torch.cuda.synchronize()
        assert np.array_equal(_bits(b.reward.cpu().numpy()), _bits(out["reward"][k])), (k, "reward")
        assert np.array_equal(b.flags.cpu().numpy(), out["flags"][k] & mask_bits), (k, "flags")
        assert np.array_equal(b.xflags.cpu().numpy(), out["xf"][k]), (k, "xflags")
        if k + 1 < T:
            assert np.array_equal(_bits(b.get_state().cpu().numpy()), _bits(out["obs"][k + 1])), (k, "state")
    hb = _handle(b)
    a.close(); b.close()
    for k in ("state", "ctr", "life"):
        assert np.array_equal(out["handle"][k].view(np.uint8), hb[k].view(np.uint8)), k
    assert out["xf"].any() and ((out["xf"] >> 8) & 7).any() and out["shielded"].any()


# ---- 6. the slot, and isolation ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["cr", "pg"])
def test_one_critic_slot_with_a_kind(ni, key):
    """Sigmoid -> categorical -> sigmoid on one handle gives the first sigmoid run bit for bit; the two kinds give different p;
    installing an actor keeps the categorical critic."""
    L = ni._lib
    ws, cw, mask, S, A = _nets(ni, key, 51)
    sw = H.critic(ni, key, S, A, 6)
    env = _make(ni, key, M.B_BIG)
    assert env.mlp_safety_kind == L.SAFETY_NONE
    env.set_mlp_policy(ws)
    runs = []
    for kind in ("sigmoid", "categorical", "sigmoid", "categorical", "actor"):
        if kind == "sigmoid":
            env.set_mlp_safety(sw, 0.5)
        elif kind == "categorical":
            env.set_mlp_safety_categorical(cw, 0.5, mask)
        else:
            env.set_mlp_policy(ws)                                   # installing an actor keeps the critic and its kind
        assert env.mlp_safety_kind == (L.SAFETY_SIGMOID if kind == "sigmoid" else L.SAFETY_CATEGORICAL)
        _start(ni, env, key)
        runs.append(_launch(ni, env, "safe"))
    env.close()
    keys = ("act", "obs", "reward", "flags", "prob")
    _same(runs[2], runs[0], "sigmoid again", keys=keys, handle=False)
    _same(runs[3], runs[1], "categorical again", keys=keys, handle=False)
    _same(runs[4], runs[1], "categorical after an actor install", keys=keys, handle=False)
    assert not np.array_equal(_bits(runs[0]["prob"]), _bits(runs[1]["prob"]))
    fresh_env, fresh = _run(ni, key, 51, M.B_BIG, "safe", 0.5)
    fresh_env.close()
    _same(runs[1], fresh, "the slot's categorical run vs a fresh handle's", keys=keys, handle=False)


@pytest.mark.parametrize("key", ["cr", "pg"])
def test_violation_prob_touches_no_handle_state(ni, oracle, key):
    """violation_prob between two launches changes no later output, counter or tally: 3 + 3 steps with a call in between equal
    3 + 3 steps without, in every output and in the handle."""
    ws, cw, mask, S, A = _nets(ni, key, 51)
    e = _evaluated(ni, oracle, key, 51)
    outs = []
    for call in (True, False):
        env = _make(ni, key, M.B_BIG)
        env.set_mlp_policy(ws)
        env.set_mlp_safety_categorical(cw, _median(ni, key, 51), mask)
        _start(ni, env, key)
        first = _launch(ni, env, "search", n=3)
        before = _handle(env)
        if call:
            p, _ = _evaluate(ni, env, e["obs"], e["raw"], 51)
            assert np.array_equal(_bits(p), _bits(e["p"]))
            after = _handle(env)
            for k in before:
                assert np.array_equal(np.asarray(before[k]), np.asarray(after[k])) or k == "tally" and np.array_equal(before[k].view(np.uint8), after[k].view(np.uint8)), k
        second = _launch(ni, env, "search", n=3)
        second["handle"] = _handle(env)
        first["handle"] = before
        outs.append((first, second))
        env.close()
    _same(outs[0][0], outs[1][0], "first launch")
    _same(outs[0][1], outs[1][1], "second launch")


@pytest.mark.parametrize("entry", ["safe", "search"])
@pytest.mark.parametrize("key", ["cr", "pg"])
def test_a_lane_does_not_depend_on_its_neighbours(ni, key, entry):
    """B = 5 equals the first five lanes of B = 700, bit for bit in every output and in the handle's per-lane arrays."""
    thr = _median(ni, key, 51)
    env, big = _run(ni, key, 51, M.B_BIG, entry, thr, autoreset=False)
    env.close()
    env, small = _run(ni, key, 51, M.B_SMALL, entry, thr, autoreset=False)
    env.close()
    _same(big, small, "B = 700 vs B = 5", lanes=slice(0, M.B_SMALL))


# ---- 7. non-finite ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["nan", "-inf", "-3e38"])
@pytest.mark.parametrize("key", [k for k, _ in M.MFMA_ENVS])
def test_non_finite_head_bias(ni, oracle, key, what):
    """c3[j] = NaN: z_j is NaN, p is NaN and every live lane shields.  c3[j] = -inf: the result is the law's, bit for bit -- which
    is NaN too, because the bias k-step multiplies the bias by 0 on the second lane half (include/nig.h says so; the oracle's
    one-row head restates it).  c3[j] = -3e38: a finite logit far below det_expf's domain, an atom of exactly no mass: p is the
    law's bit for bit and the float64 mass of the other atoms within the radius."""
    atoms, j = 51, 20
    ws, cw, mask, S, A = _nets(ni, key, atoms)
    c3 = cw[2][1].copy()
    c3[j] = {"nan": np.nan, "-inf": -np.inf, "-3e38": -3e38}[what]
    bad = [cw[0], cw[1], (cw[2][0], c3)]
    o0 = _neutral(ni, key, atoms)
    obs, raw = np.array(o0["obs"][0]), np.array(o0["act"][0])
    thr = 0.99
    env, o = _run(ni, key, atoms, M.B_BIG, "safe", thr, cw=bad)
    p, z = _evaluate(ni, env, obs, raw, atoms)
    env.close()
    with np.errstate(invalid="ignore", over="ignore"):
        col = oracle.mlp_critic(key, [bad[0], bad[1], (bad[2][0][:, j:j + 1].copy(), c3[j:j + 1].copy())], obs, raw)
        assert R.same_bits(oracle.detmath_unary("sigmoidf", z[j]), col), "the logit is the one-row head's, non-finite or not"
    assert R.same_bits(p, R.violation_prob(oracle, z, mask))
    assert R.same_bits(o["prob"][0], p)
    if what == "-3e38":
        assert np.isfinite(p).all() and (z[j] < -1e38).all()
        rest = np.delete(z, j, axis=0)
        rmask = sum(1 << (i if i < j else i - 1) for i in range(atoms) if i != j and (mask >> i) & 1)
        assert np.abs(p - R.mass64(rest, rmask)).max() <= R.radius(atoms)
        assert not o["shielded"][0].all()
    else:
        assert np.isnan(z[j]).all() and np.isnan(p).all() and np.isnan(o["prob"][o["live"]]).all()
        assert np.array_equal(o["shielded"], o["live"]), "a NaN p shields"
        assert np.array_equal(_bits(o["act"][0]), _bits(raw * f32(0.5)))


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(ni):
    L, lib = ni._lib, ni._lib.lib()
    ws, cw, mask, S, A = _nets(ni, "cr", 51)
    n = 200
    env = _make(ni, "cr", n)
    env.reset()
    dev = env.device
    obs, act = torch.zeros(S, n, device=dev), torch.zeros(A, n, device=dev)
    pr, zz = torch.full((n,), 7.5, device=dev), torch.full((51, n), 7.5, device=dev)
    p = lambda x: C.c_void_p(x.data_ptr())

    def attempt(what, n_=n, ld_obs=n, ld_act=n, ld_logit=n, code=1):
        h0 = _handle(env)
        rc = lib.nig_mlp_violation_prob(env._h, n_, p(obs), ld_obs, p(act), ld_act, p(pr), p(zz), ld_logit, env._stream())
        torch.cuda.synchronize()
        assert rc == code, (what, rc, lib.nig_last_error())
        assert bool((pr == 7.5).all()) and bool((zz == 7.5).all()), what
        h1 = _handle(env)
        assert all(np.array_equal(np.asarray(h0[k]).view(np.uint8) if isinstance(h0[k], np.ndarray) else h0[k],
                                  np.asarray(h1[k]).view(np.uint8) if isinstance(h1[k], np.ndarray) else h1[k]) for k in h0), what
    attempt("no critic installed")
    env.set_mlp_safety(H.critic(ni, "cr", S, A, 6), 0.5)
    attempt("a sigmoid critic installed")
    with pytest.raises(L.NigError):
        env.violation_prob(obs, act, layout="soa")
    env.set_mlp_safety_categorical(cw, 0.5, mask)
    attempt("n = 0", n_=0)
    attempt("ld_obs below n", ld_obs=n - 1)
    attempt("ld_act below n", ld_act=n - 1)
    attempt("ld_logit below n", ld_logit=n - 1)
    assert lib.nig_mlp_violation_prob(env._h, n, p(obs), n, p(act), n, p(pr), None, 0, env._stream()) == 0      # logit_out may be NULL
    torch.cuda.synchronize()
    assert bool((pr != 7.5).all()) and bool((zz == 7.5).all())
    # the setter's own refusals leave the slot as it was
    W = [np.ascontiguousarray(x) for pair in cw for x in pair]
    wp = [w.ctypes.data_as(C.c_void_p) for w in W]
    for atoms_, mask_, hidden in ((1, 0, 256), (65, 0, 256), (51, 1 << 51, 256)):
        assert lib.nig_set_mlp_safety_categorical(env._h, hidden, atoms_, *wp, mask_, 0.5, env._stream()) == 1
    assert lib.nig_set_mlp_safety_categorical(env._h, 128, 51, *wp, mask, 0.5, env._stream()) == 4
    assert env.mlp_safety_kind == L.SAFETY_CATEGORICAL and lib.nig_get_mlp_safety_atoms(env._h) == 51
    # the Python method refuses by ValueError what it can see: a short or misplaced output, a layout it does not know
    for bad in (dict(prob_out=torch.empty(n - 1, device=dev)), dict(logits_out=torch.empty(50, n, device=dev)),
                dict(logits_out=torch.empty(51, n - 1, device=dev)), dict(prob_out=torch.empty(n)), dict(logits_out=torch.empty(51, n)),
                dict(prob_out=torch.empty(n, dtype=torch.float64, device=dev)), dict(layout="cols")):
        with pytest.raises(ValueError):
            env.violation_prob(obs, act, **{"layout": "soa", **bad})
    with pytest.raises(ValueError):
        env.violation_prob(obs[:-1], act, layout="soa")
    env.set_mlp_safety(H.critic(ni, "cr", S, A, 6), 0.5)
    assert lib.nig_get_mlp_safety_atoms(env._h) == 0 and lib.nig_get_mlp_safety_atoms(None) == -1
    env.close()
    water = ni.make_batched("WaterTreatment-v0", 8)
    Sw, Aw = water.state_dim, water.action_dim
    cww = R.random_categorical_critic(Sw, Aw, 51, 3)
    Ww = [np.ascontiguousarray(x) for pair in cww for x in pair]
    rc = lib.nig_set_mlp_safety_categorical(water._h, 256, 51, *[w.ctypes.data_as(C.c_void_p) for w in Ww], mask, 0.5, water._stream())
    assert rc == 4 and water.mlp_safety_kind == L.SAFETY_NONE            # NIG_ERR_UNSUPPORTED: no MFMA actor for an odd state dim
    water.close()


# ---- the Python route -------------------------------------------------------------------------------------------------------------
def test_evaluate_with_safety_runs_the_categorical_agent_on_the_device(ni, monkeypatch):
    """MLPPolicy(safety_kind="categorical").shielded() / searching(3) are installed by _install_agent with
    set_mlp_safety_categorical and played by the fused kernels (under an added BoxConstraint by the _limited twins), never on the
    host; pol.compute_safety_violation_probability(state, action, env) is env.violation_prob."""
    ws, cw, mask, S, A = _nets(ni, "cr", 51)
    pol = ni.MLPPolicy(ws, safety_weights=cw, safety_kind="categorical", constraint_threshold=_median(ni, "cr", 51))
    for agent, name in ((pol.shielded(), "rollout_mlp_safe"), (pol.searching(NC), "rollout_mlp_search")):
        for limited in (False, True):
            env = ni.make_batched("ChemicalReactor-v0", 256, autoreset=False, tally=True, max_episode_steps=12)
            if limited:
                env.add_safety_constraint(ni.BoxConstraint("band", {("action", 0): (-0.5, 0.5)}, -1.0))
            assert agent.fusable

            def boom(*_a, **_k):
                raise AssertionError("the fused categorical agent must not step or predict on the host")
            monkeypatch.setattr(env, "step", boom)
            monkeypatch.setattr(agent, "predict", boom)
            monkeypatch.setattr(agent, "predict_device", boom)
            calls = []
            meth = name + ("_limited" if limited else "")
            real = getattr(env, meth)
            monkeypatch.setattr(env, meth, lambda *x, _r=real, **k: (calls.append(x), _r(*x, **k)))
            got = ni.evaluate_with_safety(agent, env, n_episodes=256)
            assert calls and env.mlp_safety_kind == ni._lib.SAFETY_CATEGORICAL and len(got) == 13, meth
            env.close()
    env = ni.make_batched("ChemicalReactor-v0", 16)
    o = _neutral(ni, "cr", 51)
    p = pol.compute_safety_violation_probability(o["obs"][0], o["act"][0], env)
    assert np.array_equal(_bits(p), _bits(np.array(o["prob"][0])))
    host = pol.compute_safety_violation_probability(o["obs"][0], o["act"][0])
    assert np.abs(host - p).max() <= 1e-4 and not np.array_equal(host, p)
    env.close()
