"""-m gpu: the fused ensemble actor (nig_set_mlp_ensemble / nig_rollout_mlp_ensemble, BatchedIndustrialEnv.rollout_mlp_ensemble)
-- the reference's EnsembleAgent.predict / predict_with_uncertainty in the MFMA actor kernel -- against the CPU oracle's actor,
the host restatement of the documented law (policies.ensemble_action / ensemble_uncertainty, held to the reference's recorded
values by tests/test_ensemble_host.py), nig_step64 / nig_step on a teacher-forced second handle, and evaluate_with_safety.

Bounds: bit equality everywhere except the uncertainty against NumPy's two-pass np.std (1e-5 relative, 1e-6 absolute: the
project's parity bar; the library documents the member-0-shifted order, which the same test holds to bit equality) and the
evaluate_with_safety dicts (1e-5: the members run as torch GEMMs on the comparison side, another float32 summation order)."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import closed_loop_matrix as M
from footprint import Arena, Layout
from test_gpu_footprint import Rig, ceil4, clean, gap, pitch

pytestmark = pytest.mark.gpu

# Which env brings which kernel shape: tests/closed_loop_matrix.py.  The cases at B = 3000 below run the five envs the module
# began with from reset(); the *_matrix tests run every env the family is compiled for (the average and the voting kernel of
# each) at the matrix's shapes, AdvancedChemicalReactor and AdvancedPowerGrid from per-lane distinct start states.

ENVS = [("cr", "ChemicalReactor-v0"), ("pg", "PowerGrid-v0"), ("ra", "RobotAssembly-v0"),
        ("acr", "AdvancedChemicalReactor-v0"), ("hvac", "HVACControl-v0")]
ACT64 = ("cr", "pg", "ra")                     # the envs whose step follows a float64 action's type (nig_step64)
B, T, MAXS, SEED = 3000, 14, 9, 0x5EED         # B not a multiple of 128: a partial last block; episodes end inside the run
# method, agent weight vector (the first K entries are the active ones)
LAWS = [("mean", [0.9, 0.4, 1.7, 0.3, 0.6, 1.1, 0.2, 0.8]), ("weighted", [0.5, -0.2, 0.4, 0.3, 0.1, 0.25, -0.05, 0.2]), ("voting", None)]


@pytest.fixture(scope="module")
def ni():
    import neorl_industrial_gym_amd as ni
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return ni


def _random_actor(S, A, seed):       # the style of test_gpu_safety_shield.py
    rng = np.random.default_rng(seed)
    return [(rng.normal(0, 1.0 / np.sqrt(S), (S, 256)).astype(np.float32) * np.float32(0.05), rng.normal(0, 0.05, 256).astype(np.float32)),
            (rng.normal(0, 1.0 / 16, (256, 256)).astype(np.float32), rng.normal(0, 0.05, 256).astype(np.float32)),
            (rng.normal(0, 1.0 / 8, (256, A)).astype(np.float32), rng.normal(0, 0.1, A).astype(np.float32))]


def _dims(ni, name):
    probe = ni.make_batched(name, 1)
    S, A = probe.state_dim, probe.action_dim
    probe.close()
    return S, A


def _raw_members(S, A, K, seed0):
    return [_random_actor(S, A, seed0 + 7 * k) for k in range(K)]


_SCALE = {}


def _members(ni, name, K, seed0):
    """K random actors whose first layer is scaled to the env's state magnitudes (20 / (1 + mean |s_i|) per state column, the
    states of a probe handle after three uniform-action steps).  Unscaled, ChemicalReactor's temperatures of ~350 drive every
    tanh head to exactly +-1: all lanes then share ONE uncertainty value and a threshold at the median flags nobody."""
    if name not in _SCALE:
        probe = ni.make_batched(name, 512, seed=SEED)
        probe.reset()
        for t in range(1, 4):
            probe.step(probe.fill_actions(t), layout="soa")
        torch.cuda.synchronize()
        _SCALE[name] = (probe.state_dim, probe.action_dim,
                        (1.0 / (1.0 + np.abs(probe.get_state().cpu().numpy()).mean(axis=0))).astype(np.float32))
        probe.close()
    S, A, sc = _SCALE[name]
    return [[((m[0][0] * np.float32(20.0) * sc[:, None]).astype(np.float32), m[0][1]), m[1], m[2]] for m in _raw_members(S, A, K, seed0)]


def _install(ni, env, members, method, w, thr):
    from neorl_industrial_gym_amd.policies import ensemble_active_weights
    if method == "voting":
        env.set_mlp_ensemble(members, None, None, method, thr)
        return None
    aw, wsum = ensemble_active_weights(w, len(members), method)
    env.set_mlp_ensemble(members, aw, wsum, method, thr)
    return aw


def _run(ni, name, members, method, w, thr, B=B, T=T, autoreset=True, env_index0=0, launches=None, fill=0.0, max_steps=MAXS, start=False):
    """start: give the lanes of an env whose reset is the same for every lane distinct start states (closed_loop_matrix)."""
    K = len(members)
    env = ni.make_batched(name, B, autoreset=autoreset, tally=True, max_episode_steps=max_steps, env_index0=env_index0, seed=SEED)
    _install(ni, env, members, method, w, thr)
    dev = env.device
    act = torch.full((T, env.action_dim, env.ld), fill, dtype=torch.float32, device=dev)
    mem = torch.full((T, K, env.action_dim, env.ld), fill, dtype=torch.float32, device=dev)
    # (an observation step is a multiple of 4 floats: where B * S is none, the rows are padded and the C entry point is called
    # directly -- the Python method takes a contiguous [n, B, S] tensor)
    S, ostep = env.state_dim, (B * env.state_dim + 3) // 4 * 4
    obs = torch.full((T, ostep), fill, dtype=torch.float32, device=dev)
    fl = torch.zeros(T, env.ld, dtype=torch.int32, device=dev)
    rw = torch.zeros(T, env.ld, dtype=torch.float32, device=dev)
    un = torch.full((T, env.ld), fill, dtype=torch.float32, device=dev)
    P = lambda t: C.c_void_p(t.data_ptr())
    env.reset()
    if start:
        M.install_start(ni, env, M.KEY_OF[name], SEED)
    t0 = env.counter
    k0 = 0
    for n in (launches or (T,)):
        if ostep != B * S:
            with torch.cuda.device(dev):
                ni._lib.check(ni._lib.lib().nig_rollout_mlp_ensemble(env._h, n, P(rw[k0:]), P(fl[k0:]), env.ld, P(obs[k0:]), ostep, P(act[k0:]), env.ld,
                                                                     env.action_dim * env.ld, P(un[k0:]), P(mem[k0:]), env._stream()))
        else:
            env.rollout_mlp_ensemble(n, rw[k0:], fl[k0:], obs[k0:].view(-1, B, S), act[k0:], un[k0:], mem[k0:])
        k0 += n
    assert k0 == T
    torch.cuda.synchronize()
    assert env.counter == t0 + T
    out = dict(act=act[:, :, :B].permute(0, 2, 1).cpu().numpy(), mem=mem[:, :, :, :B].permute(0, 1, 3, 2).cpu().numpy(),
               obs=obs[:, :B * S].reshape(T, B, S).cpu().numpy(), flags=fl[:, :B].cpu().numpy(), rew=rw[:, :B].cpu().numpy(), unc=un[:, :B].cpu().numpy(), t0=t0)
    out["live"] = (out["flags"] & ni._lib.FLAG_INACTIVE) == 0
    out["uncertain"] = (out["flags"] & ni._lib.FLAG_UNCERTAIN) != 0
    return env, out


def _law(o, method, w):
    """The documented law on the recorded member actions: (float64 or float32 action [T, B, A], uncertainty [T, B])."""
    from neorl_industrial_gym_amd.policies import ensemble_action, ensemble_uncertainty
    preds = np.ascontiguousarray(o["mem"].transpose(1, 0, 2, 3))           # [K, T, B, A]
    return ensemble_action(preds, w, method), ensemble_uncertainty(preds), preds


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32 if x.dtype == np.float32 else np.uint64)


@pytest.mark.parametrize("method,w", LAWS, ids=[m for m, _ in LAWS])
@pytest.mark.parametrize("autoreset", [False, True], ids=["frozen", "autoreset"])
@pytest.mark.parametrize("key,name", ENVS)
def test_members_action_and_uncertainty(ni, oracle, key, name, autoreset, method, w):
    """Every member's action is the oracle's single actor on the recorded observation; act_out is the documented law on the
    recorded member actions; unc_out is the documented order bit for bit and np.std(...).mean(-1) to the parity bar; the flag
    is unc_out > threshold with the threshold at the median of a first run's uncertainties (both branches taken)."""
    _members_action_and_uncertainty(ni, oracle, key, name, autoreset, method, w, dict(B=B, T=T, max_steps=MAXS))


# the matrix's cases: both batch sizes, both kernels (average, voting), lanes that freeze and lanes that reset
MATRIX_CASES = [(M.B_BIG, True, LAWS[0]), (M.B_BIG, False, LAWS[2]), (M.B_BIG, True, LAWS[1]), (M.B_SMALL, False, LAWS[0]), (M.B_SMALL, True, LAWS[2])]
MATRIX_IDS = [f"{b}-{'autoreset' if ar else 'frozen'}-{law[0]}" for b, ar, law in MATRIX_CASES]


def _matrix_members(ni, key, name, K, seed0):
    return [M.continuing(key, m) for m in _members(ni, name, K, seed0)]


@pytest.mark.parametrize("B,autoreset,law", MATRIX_CASES, ids=MATRIX_IDS)
@pytest.mark.parametrize("key,name", M.MFMA_ENVS)
def test_members_action_and_uncertainty_matrix(ni, oracle, key, name, B, autoreset, law):
    """test_members_action_and_uncertainty on every MFMA env at the closed-loop matrix's shapes; on step 0 the member actions of
    the envs only these cases reach are also held to the actor in NumPy float64."""
    _members_action_and_uncertainty(ni, oracle, key, name, autoreset, law[0], law[1], dict(B=B, T=M.T_NEW, max_steps=M.MAXS_NEW, start=True))


def _members_action_and_uncertainty(ni, oracle, key, name, autoreset, method, w, shape):
    S, A = _dims(ni, name)
    T, start = shape["T"], shape.get("start", False)
    K = 3 if method != "voting" else 5
    ms = _matrix_members(ni, key, name, K, 100) if start else _members(ni, name, K, 100)
    env0, o0 = _run(ni, name, ms, method, w, 0.2, autoreset=autoreset, **shape)
    env0.close()
    thr = float(np.median(o0["unc"][o0["live"]]))
    env, o = _run(ni, name, ms, method, w, thr, autoreset=autoreset, fill=-7.0, **shape)
    live = o["live"]
    assert live[0].all() and (autoreset or not live[-1].all()), "episodes must end inside the run"
    if start and key in M.FLOAT64_KEYS:
        for m in range(K):
            assert M.worst(f"{key} {method} B={shape['B']}: member {m}'s actions of step 0 against float64", o["mem"][0, m],
                           M.actor64(ms[m], o["obs"][0]), M.ACT_ATOL) <= 1.0
    if start and key in M.CLONED and shape["B"] == M.B_BIG:
        assert M.distinct_rows(o["mem"][0, 0]) >= 600 and M.distinct_rows(o["act"][0]) >= 600, "step 0: the lanes are no clones of each other"
    for k in range(T):
        for m in range(K):
            want = oracle.mlp_actions(key, ms[m], o["obs"][k])
            assert np.array_equal(_bits(o["mem"][k, m])[live[k]], _bits(want)[live[k]]), (k, m)
    act, unc, preds = _law(o, method, w)
    assert act.dtype == (np.float32 if method == "voting" else np.float64)
    assert np.array_equal(_bits(o["act"])[live], _bits(act.astype(np.float32))[live])
    assert np.array_equal(_bits(o["unc"])[live], _bits(unc)[live])
    ref = np.std(preds, axis=0).mean(axis=-1)
    err = np.abs(o["unc"].astype(np.float64) - ref.astype(np.float64))[live]
    bound = np.maximum(1e-5 * np.abs(ref.astype(np.float64)), 1e-6)[live]
    print(f"{key} {method}: uncertainty against np.std, max error / bound {np.max(err / bound):.3g}")
    assert np.all(err <= bound)
    assert np.array_equal(o["uncertain"][live], (o["unc"] > np.float32(thr))[live])
    assert not o["uncertain"][~live].any()
    frac = o["uncertain"][live].mean()
    assert 0.05 < frac < 0.95, frac
    # frozen lanes keep their words
    for name_ in ("act", "mem", "unc", "obs"):
        x = o[name_] if name_ != "mem" else o["mem"].transpose(0, 2, 1, 3)
        assert np.all(x[~live] == np.float32(-7.0)), name_
    env.close()


@pytest.mark.parametrize("method,w", LAWS, ids=[m for m, _ in LAWS])
@pytest.mark.parametrize("autoreset", [False, True], ids=["frozen", "autoreset"])
@pytest.mark.parametrize("key,name", ENVS)
def test_the_step_took_that_action(ni, key, name, autoreset, method, w):
    """A second handle (same seed and env_index0) is teacher-forced per step with obs_out[k], the step counters of the flag
    words and the launch counter, and stepped in fast mode on the recomputed action: nig_step64 on the float64 action for the
    average methods on ChemicalReactor / PowerGrid / RobotAssembly, nig_step on the float32 action otherwise.  Its new state is
    obs_out[k + 1] bit for bit on lanes that did not finish; reward and flag word (without NIG_FLAG_UNCERTAIN) are the rollout's
    on every live lane.  Where the float64 step applies, a third handle stepping on the float32-rounded action must differ
    from it in some state word -- otherwise this test could not tell the two instantiations apart."""
    _the_step_took_that_action(ni, key, name, autoreset, method, w, dict(B=B, T=T, max_steps=MAXS))


@pytest.mark.parametrize("B,autoreset,law", MATRIX_CASES, ids=MATRIX_IDS)
@pytest.mark.parametrize("key,name", M.MFMA_ENVS)
def test_the_step_took_that_action_matrix(ni, key, name, B, autoreset, law):
    """test_the_step_took_that_action on every MFMA env at the closed-loop matrix's shapes."""
    _the_step_took_that_action(ni, key, name, autoreset, law[0], law[1], dict(B=B, T=M.T_NEW, max_steps=M.MAXS_NEW, start=True))


def _the_step_took_that_action(ni, key, name, autoreset, method, w, shape):
    S, A = _dims(ni, name)
    B, T, MAXS, start = shape["B"], shape["T"], shape["max_steps"], shape.get("start", False)
    ms = _matrix_members(ni, key, name, 3, 200) if start else _members(ni, name, 3, 200)
    L = ni._lib
    env, o = _run(ni, name, ms, method, w, 0.2, autoreset=autoreset, **shape)
    env.close()
    act, _, _ = _law(o, method, w)
    f64 = method != "voting" and key in ACT64
    if not f64:
        act = act.astype(np.float32)
    e2 = ni.make_batched(name, B, autoreset=autoreset, tally=True, max_episode_steps=MAXS, seed=SEED)
    e3 = ni.make_batched(name, B, autoreset=autoreset, tally=True, max_episode_steps=MAXS, seed=SEED) if f64 else None
    live = o["live"]
    differ = checked = 0
    for k in range(T - 1):
        fl = o["flags"][k]
        step_after = (fl.astype(np.uint32) >> L.FLAG_STEP_SHIFT).astype(np.int64)
        ctr = np.where(live[k], step_after - 1, L.CTR_DONE).astype(np.int32)
        res = []
        for e, a in ((e2, act[k]), (e3, act[k].astype(np.float32))):
            if e is None:
                continue
            e.state_soa.copy_(torch.from_numpy(np.ascontiguousarray(o["obs"][k].T)).to(e.device))
            e.ctr.copy_(torch.from_numpy(ctr).to(e.device))
            e.counter = o["t0"] + k
            nxt, rew, _, _, _ = e.step(torch.from_numpy(np.ascontiguousarray(a)).to(e.device), layout="aos")
            torch.cuda.synchronize()
            res.append((nxt.cpu().numpy().copy(), rew.cpu().numpy().copy(), e.flags.cpu().numpy().copy()))
        nxt, rew, f2 = res[0]
        cont = live[k] & live[k + 1] & ((fl & (L.FLAG_TERMINATED | L.FLAG_TRUNCATED | L.FLAG_DID_RESET)) == 0)
        checked += int(cont.sum())
        assert np.array_equal(_bits(o["obs"][k + 1])[cont], _bits(nxt)[cont]), k
        assert np.array_equal(_bits(o["rew"][k])[live[k]], _bits(rew)[live[k]]), k
        assert np.array_equal((fl & ~L.FLAG_UNCERTAIN)[live[k]], f2[live[k]]), k
        if f64:
            differ += int((_bits(res[1][0])[cont] != _bits(nxt)[cont]).any(axis=1).sum())
    # (more than one compared step per lane on average; five lanes of a plant whose episodes may end on their first steps --
    # RobotAssembly leaves its workspace -- need not reach that: there the loop must have compared something)
    assert checked > (B if B > 100 else 0)
    if f64:
        print(f"{key} {method}: lane-steps on which the float32 and the float64 step differ: {differ} of {checked}")
        assert differ > 0, "no lane tells the float64 step from the float32 one"
    e2.close()
    if e3 is not None:
        e3.close()


@pytest.mark.parametrize("autoreset", [False, True], ids=["frozen", "autoreset"])
@pytest.mark.parametrize("key,name", ENVS)
def test_one_voting_member_is_the_single_actor(ni, oracle, key, name, autoreset):
    """K = 1, VOTING: actions, flags, rewards, final state, counters and tallies bit for bit nig_rollout_mlp's with that actor
    (and the oracle's rollout), uncertainty exactly 0, and no UNCERTAIN bit at threshold 0 (0 > 0 is false)."""
    _one_voting_member_is_the_single_actor(ni, oracle, key, name, autoreset, dict(B=B, T=T, max_steps=MAXS))


@pytest.mark.parametrize("B,autoreset", [(M.B_BIG, True), (M.B_BIG, False), (M.B_SMALL, True)])
@pytest.mark.parametrize("key,name", M.MFMA_ENVS)
def test_one_voting_member_is_the_single_actor_matrix(ni, oracle, key, name, B, autoreset):
    """test_one_voting_member_is_the_single_actor on every MFMA env at the closed-loop matrix's shapes.  The oracle's own rollout
    starts from reset(); from the distinct start states of the two Advanced envs the oracle's actor on every recorded observation
    and its env step on every recorded action take its place."""
    _one_voting_member_is_the_single_actor(ni, oracle, key, name, autoreset, dict(B=B, T=M.T_NEW, max_steps=M.MAXS_NEW, start=True))


def _one_voting_member_is_the_single_actor(ni, oracle, key, name, autoreset, shape):
    S, A = _dims(ni, name)
    B, T, MAXS, start = shape["B"], shape["T"], shape["max_steps"], shape.get("start", False)
    ws = _matrix_members(ni, key, name, 1, 301)[0] if start else _members(ni, name, 1, 301)[0]
    env, o = _run(ni, name, [ws], "voting", None, 0.0, autoreset=autoreset, **shape)
    ref = ni.make_batched(name, B, autoreset=autoreset, tally=True, max_episode_steps=MAXS, seed=SEED)
    ref.set_mlp_policy(ws)
    act = torch.zeros(T, A, ref.ld, dtype=torch.float32, device=ref.device)
    fl = torch.zeros(T, ref.ld, dtype=torch.int32, device=ref.device)
    rw = torch.zeros(T, ref.ld, dtype=torch.float32, device=ref.device)
    ref.reset()
    if start:
        M.install_start(ni, ref, key, SEED)
    ref.rollout_mlp(T, rw, fl, None, act)
    torch.cuda.synchronize()
    live = o["live"]
    assert np.array_equal(o["flags"], fl[:, :B].cpu().numpy()) and np.array_equal(_bits(o["rew"]), _bits(rw[:, :B].cpu().numpy()))
    assert np.array_equal(_bits(o["act"])[live], _bits(act[:, :, :B].permute(0, 2, 1).cpu().numpy())[live])
    assert np.array_equal(_bits(o["mem"][:, 0])[live], _bits(o["act"])[live])
    for a, b in ((env.get_state(), ref.get_state()), (env.ctr, ref.ctr), (env.life_viol, ref.life_viol), (env.tally, ref.tally),
                 (env.ep_return, ref.ep_return)):
        assert torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))
    if start and key in M.CLONED:
        for k in range(T):
            assert np.array_equal(_bits(o["act"][k])[live[k]], _bits(oracle.mlp_actions(key, ws, o["obs"][k]))[live[k]]), k
        assert M.check_env_steps(oracle, ni._lib, key, o["obs"], o["act"], o["flags"], SEED, MAXS) > 0
        if B == M.B_BIG:
            assert M.distinct_rows(o["act"][0]) >= 600, "step 0: the lanes are no clones of each other"
    else:
        r = oracle.rollout_mlp(key, B, T, ws, max_steps=MAXS, autoreset=autoreset, nthreads=8, trajectories=True)
        assert np.array_equal(_bits(o["act"])[live], _bits(r["act"])[live])
        assert np.array_equal(_bits(env.get_state().cpu().numpy()), _bits(r["state"]))
        assert np.array_equal(env.current_step.cpu().numpy(), r["step"]) and np.array_equal(env.done.cpu().numpy(), r["done"] != 0)
    if start and key in M.FLOAT64_KEYS:
        assert M.worst(f"{key} B={B}: the voting member's actions of step 0 against float64", o["act"][0], M.actor64(ws, o["obs"][0]), M.ACT_ATOL) <= 1.0
    assert np.all(o["unc"][live] == 0.0) and not o["uncertain"].any()
    env.close(); ref.close()


@pytest.mark.parametrize("key,name", [("cr", "ChemicalReactor-v0"), ("pg", "PowerGrid-v0"), ("hvac", "HVACControl-v0")])
def test_identical_members(ni, key, name):
    """K = 4 identical members, average method, weights 1/4 each (exact in binary): the float64 action is the member's action as
    a double, so act_out is the member's action bit for bit; the uncertainty is exactly 0."""
    S, A = _dims(ni, name)
    ws = _members(ni, name, 1, 311)[0]
    env, o = _run(ni, name, [ws] * 4, "weighted", [0.25] * 4, -1.0)
    live = o["live"]
    act, unc, _ = _law(o, "weighted", [0.25] * 4)
    assert np.array_equal(act[live], o["mem"][:, 0].astype(np.float64)[live])
    assert np.array_equal(_bits(o["act"])[live], _bits(o["mem"][:, 0])[live])
    assert np.all(o["unc"][live] == 0.0) and np.all(unc == 0.0)
    assert o["uncertain"][live].all()                       # 0 > -1: a negative threshold flags every live step
    env.close()


def test_thresholds(ni):
    """NIG_FLAG_UNCERTAIN is exactly unc_out > threshold: at a value that occurs (that lane is not flagged), at inf (never) and
    at a negative value (always).  The threshold changes nothing but the flag bit."""
    name = "ChemicalReactor-v0"
    S, A = _dims(ni, name)
    ms = _members(ni, name, 3, 400)
    method, w = LAWS[0]
    env, o0 = _run(ni, name, ms, method, w, 0.2)
    env.close()
    u0 = np.sort(o0["unc"][0])
    occurring = float(u0[len(u0) // 2])
    for thr in (occurring, float("inf"), -0.5):
        env, o = _run(ni, name, ms, method, w, thr)
        env.close()
        live = o["live"]
        for k in ("act", "mem", "obs", "rew", "unc"):
            assert np.array_equal(_bits(o[k]), _bits(o0[k])), k
        assert np.array_equal(o["flags"] & ~ni._lib.FLAG_UNCERTAIN, o0["flags"] & ~ni._lib.FLAG_UNCERTAIN)
        assert np.array_equal(o["uncertain"][live], (o["unc"] > np.float32(thr))[live])
        if thr == occurring:
            at = o["unc"][0] == np.float32(thr)
            assert at.any() and not o["uncertain"][0][at].any() and o["uncertain"][0].any()
        elif thr > 0:
            assert not o["uncertain"].any()
        else:
            assert o["uncertain"][live].all()


@pytest.mark.parametrize("method,w", [LAWS[0], LAWS[2]], ids=["mean", "voting"])
@pytest.mark.parametrize("b", [1, 33, 129, 65536])
@pytest.mark.parametrize("key,name", [("cr", "ChemicalReactor-v0"), ("pg", "PowerGrid-v0")])
def test_batches(ni, oracle, key, name, b, method, w):
    """One lane, part of a wave, a block plus a lane and 65 536 lanes: members against the oracle (a sample of the lanes at the
    large batch), action and uncertainty against the law, tallies and total_violations against a host replay of the flag words."""
    S, A = _dims(ni, name)
    K, T_ = (8, 12) if b < 1000 else (2, 6)
    ms = _members(ni, name, K, 500)
    env, o = _run(ni, name, ms, method, w, 0.1, B=b, T=T_, max_steps=5)
    live, L = o["live"], ni._lib
    assert live.all()
    lanes = np.arange(b) if b < 1000 else np.unique(np.concatenate([np.arange(300), np.arange(b - 300, b),
                                                                    np.random.default_rng(1).integers(0, b, 1500)]))
    for k in range(T_):
        for m in range(K):
            want = oracle.mlp_actions(key, ms[m], o["obs"][k][lanes])
            assert np.array_equal(_bits(o["mem"][k, m][lanes]), _bits(want)), (k, m)
    act, unc, _ = _law(o, method, w)
    assert np.array_equal(_bits(o["act"]), _bits(act.astype(np.float32))) and np.array_equal(_bits(o["unc"]), _bits(unc))
    assert np.array_equal(o["uncertain"], o["unc"] > np.float32(0.1))
    f = o["flags"].astype(np.int64)
    ended = (f & (L.FLAG_TERMINATED | L.FLAG_TRUNCATED)) != 0
    nviol = ((f >> L.FLAG_NVIOL_SHIFT) & 3) + ((f & L.FLAG_NVIOL_HI) != 0) * 4
    assert ended.any()
    assert np.array_equal(env.tally[L.T_EPISODES].cpu().numpy(), ended.sum(axis=0).astype(np.float64))
    assert np.array_equal(env.total_violations.cpu().numpy(), nviol.sum(axis=0))
    step_now = (f[-1] >> L.FLAG_STEP_SHIFT) * ~ended[-1]
    assert np.array_equal(env.current_step.cpu().numpy(), step_now)
    env.close()


@pytest.mark.parametrize("method,w", [LAWS[1], LAWS[2]], ids=["weighted", "voting"])
@pytest.mark.parametrize("autoreset", [False, True], ids=["frozen", "autoreset"])
def test_two_launches_and_two_shards_are_one_rollout(ni, method, w, autoreset):
    """Two launches continue one rollout, and two handles of half the lanes (env_index0 set) are one handle: every output word
    and everything the handle keeps, bit for bit."""
    name = "PowerGrid-v0"
    S, A = _dims(ni, name)
    ms = _members(ni, name, 5, 600)
    b = 1000
    env, o = _run(ni, name, ms, method, w, 0.1, B=b, autoreset=autoreset)
    env2, o2 = _run(ni, name, ms, method, w, 0.1, B=b, autoreset=autoreset, launches=(5, 9))
    keys = ("act", "mem", "obs", "rew", "unc", "flags")
    live = o["live"]
    for k in keys:
        x, y = (o[k], o2[k]) if k != "mem" else (o[k].transpose(0, 2, 1, 3), o2[k].transpose(0, 2, 1, 3))
        assert np.array_equal(_bits(x)[live] if x.dtype == np.float32 else x[live], _bits(y)[live] if y.dtype == np.float32 else y[live]), k
    for a, c in ((env.get_state(), env2.get_state()), (env.ctr, env2.ctr), (env.life_viol, env2.life_viol), (env.ep_return, env2.ep_return)):
        assert torch.equal(a.contiguous().view(torch.uint8), c.contiguous().view(torch.uint8))
    assert torch.equal(env.tally[ni._lib.T_EPISODES], env2.tally[ni._lib.T_EPISODES])
    assert torch.allclose(env.tally, env2.tally, rtol=1e-12, atol=0)      # (sums of several episodes merge as one partial per launch)
    env2.close()
    lo, olo = _run(ni, name, ms, method, w, 0.1, B=b // 2, autoreset=autoreset)
    hi, ohi = _run(ni, name, ms, method, w, 0.1, B=b // 2, autoreset=autoreset, env_index0=b // 2)
    for k in keys:
        ax = 2 if k == "mem" else 1
        both = np.concatenate([olo[k], ohi[k]], axis=ax)
        x, y = (o[k], both) if k != "mem" else (o[k].transpose(0, 2, 1, 3), both.transpose(0, 2, 1, 3))
        assert np.array_equal(_bits(x)[live] if x.dtype == np.float32 else x[live], _bits(y)[live] if y.dtype == np.float32 else y[live]), k
    st = torch.cat([lo.get_state(), hi.get_state()], dim=0)
    assert torch.equal(env.get_state().contiguous().view(torch.int32), st.contiguous().view(torch.int32))
    assert torch.equal(env.ctr, torch.cat([lo.ctr, hi.ctr]))
    env.close(); lo.close(); hi.close()


@pytest.mark.parametrize("autoreset", [True, False], ids=["autoreset", "frozen"])
@pytest.mark.parametrize("mode", ["tight", "odd", "wide"])
@pytest.mark.parametrize("key,Bf", [("cr", 129), ("pg", 333)])
def test_footprint(ni, key, Bf, mode, autoreset):
    """The entry point in canary arenas at pitch == B, B + an odd gap and a pitch that is no multiple of 64: the documented words
    are written, everything else keeps the canary, the handle's workspace pads are untouched."""
    K, chunks = 3, (6, 4)
    r = Rig(ni, key, Bf, autoreset=autoreset, max_steps=4)
    S, A, ld, L, FL = r.S, r.A, r.ld, r.L, ni._lib
    _install(ni, r.env, _raw_members(S, A, K, 700), "mean", LAWS[0][1], 0.1)
    a = Arena("cuda")
    os_, lda = pitch(mode, Bf, ld, 1), pitch(mode, Bf, ld, 2)
    assert mode != "wide" or (os_ % 64 and lda % 64)
    sa = A * lda + gap(mode, 2)
    bufs = []
    for c, T_ in enumerate(chunks):
        bufs.append((T_, a.add(f"reward_out{c}", "f32", Layout(T_, os_, 1, os_, Bf)), a.add(f"flags_out{c}", "flags", Layout(T_, os_, 1, os_, Bf)),
                     a.add(f"unc_out{c}", "f32", Layout(T_, os_, 1, os_, Bf)),
                     a.add(f"obs_out{c}", "f32", Layout(T_, ceil4(Bf * S) + gap(mode, 1, mult4=True), 1, Bf * S, Bf * S, lane_width=S), align=16),
                     a.add(f"act_out{c}", "f32", Layout(T_, sa, A, lda, Bf)),
                     a.add(f"member_act_out{c}", "f32", Layout(T_ * K, sa, A, lda, Bf), extra_outer=K)))
    a.build()
    r.reset()
    written = {}
    p = lambda b: C.c_void_p(b.ptr)
    for T_, rew, fl, un, obs, act, mem in bufs:
        rc = L.nig_rollout_mlp_ensemble(r.h, T_, p(rew), p(fl), os_, p(obs), obs.layout.outer_stride, p(act), lda, sa, p(un), p(mem), r.st())
        assert rc == 0, L.nig_last_error()
        torch.cuda.synchronize()
        f = fl.rows(T_)[:, 0]
        live = (f & FL.FLAG_INACTIVE) == 0
        assert autoreset == bool(live.all())
        for b_, n, lv in ((rew, T_, None), (fl, T_, None), (un, T_, live), (obs, T_, live), (act, T_, live),
                          (mem, T_ * K, live.repeat_interleave(K, dim=0))):
            written[b_.name] = dict(n_outer=n, live=None if autoreset else lv)
    clean([str(x) for x in a.check(written)] + r.workspace_findings(), f"{key} {mode}")
    r.close()


def test_refusals(ni):
    """Every refused call returns its code, names the argument in nig_last_error() and launches nothing: the outputs keep their
    canary and the handle its launch counter."""
    L, lib = ni._lib.lib(), ni._lib
    env = ni.make_batched("ChemicalReactor-v0", 256, seed=SEED)
    S, A = env.state_dim, env.action_dim
    ms = _raw_members(S, A, 9, 800)
    flat = [[np.ascontiguousarray(x) for pair in m for x in pair] for m in ms]
    cols = lambda K: [(C.c_void_p * K)(*[w[j].ctypes.data for w in flat[:K]]) for j in range(6)]
    wts = (C.c_double * 9)(*([0.1] * 9))
    st = env._stream()

    def set_(K, hidden=256, method=0, weights=wts, wsum=1.0, arrays=None, h=None):
        return L.nig_set_mlp_ensemble(h or env._h, K, hidden, *(arrays if arrays is not None else cols(max(K, 1))), method, weights, wsum, 0.2, st)

    out = torch.full((4, 3 + 2 * A, env.ld), -7.0, dtype=torch.float32, device=env.device)
    fl = torch.full((4, 3 + 2 * A, env.ld), -1, dtype=torch.int32, device=env.device)      # (row 0 used: reward_out's row stride)

    def roll(h=None, lda=None):
        P = lambda t: C.c_void_p(t.data_ptr())
        lda = env.ld if lda is None else lda
        return L.nig_rollout_mlp_ensemble(h or env._h, 4, P(out[:, 0]), P(fl), out.stride(0), None, 0, P(out[:, 2:2 + A]), lda, out.stride(0),
                                          P(out[:, 1]), None, st)
    env.reset()
    t0 = env.counter
    assert roll() == 1 and b"no ensemble installed" in L.nig_last_error()
    for rc, want, word in ((set_(0), 1, b"n_members"), (set_(9), 1, b"n_members"),
                           (set_(2, arrays=[None] + cols(2)[1:]), 1, b"NULL member array"),
                           (set_(2, arrays=[(C.c_void_p * 2)(flat[0][0].ctypes.data, None)] + cols(2)[1:]), 1, b"NULL member array"),
                           (set_(2, method=2), 1, b"method"), (set_(2, weights=None), 1, b"weights"),
                           (set_(2, weights=(C.c_double * 2)(0.5, float("nan"))), 1, b"weights"),
                           (set_(2, weights=(C.c_double * 2)(0.5, float("inf"))), 1, b"weights"),
                           (set_(2, wsum=float("nan")), 1, b"weight_sum"), (set_(2, wsum=float("inf")), 1, b"weight_sum"),
                           (set_(2, wsum=0.0), 1, b"weight_sum"), (set_(2, hidden=128), 4, b"hidden")):
        assert rc == want, (rc, want, word, L.nig_last_error())
    for args, word in ((dict(K=0), b"n_members"), (dict(K=2, method=2), b"method"), (dict(K=2, wsum=0.0), b"weight_sum"), (dict(K=2, hidden=128), b"hidden")):
        set_(**args)
        assert word in L.nig_last_error() and b"nig_set_mlp_ensemble" in L.nig_last_error()
    assert roll() == 1 and b"no ensemble installed" in L.nig_last_error()            # the refused installs installed nothing
    assert set_(2, method=1, weights=None, wsum=0.0) == 0                             # VOTING ignores weights and weight_sum
    assert roll(lda=env.batch - 1) == 1 and b"pitch" in L.nig_last_error()
    assert L.nig_rollout_mlp_ensemble(env._h, 0, None, None, 0, None, 0, None, 0, 0, None, None, st) == 1
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((fl == -1).all()) and env.counter == t0
    with pytest.raises(lib.NigError):                       # the single actor is a separate installation
        env.rollout_mlp(2)
    env.set_mlp_policy(ms[0])
    assert roll() == 0
    env.rollout_mlp(2)
    torch.cuda.synchronize()
    assert bool((fl[:, 0, :env.batch] != -1).all()) and bool((fl[:, 1:] == -1).all())
    env.close()
    odd = ni.make_batched("WaterTreatment-v0", 64)          # odd state dim: no MFMA actor
    Sw, Aw = odd.state_dim, odd.action_dim
    mw = [[np.ascontiguousarray(x) for pair in _random_actor(Sw, Aw, 3) for x in pair]] * 2
    colw = [(C.c_void_p * 2)(*[w[j].ctypes.data for w in mw]) for j in range(6)]
    assert L.nig_set_mlp_ensemble(odd._h, 2, 256, *colw, 1, None, 0.0, 0.2, odd._stream()) == 4 and b"env shape" in L.nig_last_error()
    assert L.nig_rollout_mlp_ensemble(odd._h, 2, None, None, 0, None, 0, None, 0, 0, None, None, odd._stream()) == 4
    with pytest.raises(ValueError):
        odd.set_mlp_ensemble([], None, None, "median", 0.2)
    odd.close()


def _flax(layers):
    return {"params": {"MLP_0": {f"Dense_{i}": {"kernel": W, "bias": b} for i, (W, b) in enumerate(layers)}}}


@pytest.mark.parametrize("method", ["mean", "voting"])
@pytest.mark.parametrize("name", ["ChemicalReactor-v0", "PowerGrid-v0"])
def test_evaluate_with_safety_runs_the_fused_ensemble(ni, monkeypatch, name, method):
    """A reference-shaped ensemble agent (agents with Flax trees, weights, ensemble_method; one member untrained) reaches
    rollout_mlp_ensemble, and its 13-key dict equals the dict of the per-step loop around the same ensemble's torch form."""
    S, A = _dims(ni, name)
    nets = _members(ni, name, 4, 900)
    mk = lambda ws, tr: types.SimpleNamespace(state={"actor": types.SimpleNamespace(params=_flax(ws)), "safety": None},
                                               is_trained=tr, constraint_threshold=0.1)
    agent = types.SimpleNamespace(agents=[mk(nets[0], True), mk(nets[1], False), mk(nets[2], True), mk(nets[3], True)],
                                  weights=np.array([0.4, 0.3, 0.2, 0.1]), ensemble_method=method, uncertainty_threshold=0.2,
                                  is_trained=True, state={"ensemble": "initialized"})
    pol = ni.EnsemblePolicy.from_agent(agent)
    assert pol.fusable and len(pol.members) == 3
    a = ni.make_batched(name, 256, autoreset=False, tally=True, max_episode_steps=48)
    b = ni.make_batched(name, 256, autoreset=False, tally=True, max_episode_steps=48)

    class StepLoop:                                         # no `agents`, no `install`: evaluate_with_safety steps it one env.step at a time
        is_trained = True

        def predict_device(self, obs):
            return pol.predict_device(obs)
    want = ni.evaluate_with_safety(StepLoop(), b, n_episodes=256)

    def boom(*_a, **_k):
        raise AssertionError("the fused ensemble path must not step on the host")
    monkeypatch.setattr(a, "step", boom)
    calls = []
    real = a.rollout_mlp_ensemble
    monkeypatch.setattr(a, "rollout_mlp_ensemble", lambda *x, **k: (calls.append(x), real(*x, **k)))
    got = ni.evaluate_with_safety(agent, a, n_episodes=256)
    assert calls
    assert len(got) == 13 and set(got) == set(want)
    for k in want:
        print(f"{name} {method} {k}: fused {got[k]!r} step loop {want[k]!r}")
    for k in want:
        assert got[k] == pytest.approx(want[k], rel=1e-5, abs=1e-6), k
    a.close(); b.close()
