"""gpu: the LayerNorm MFMA actor ("nig-mlp-ln-v1", csrc/nig_mlp_ln.hpp) -- nig_set_mlp_policy_ln and nig_rollout_mlp's dispatch on the
actor slot's kind.  The law's arithmetic is restated on the host by tests/mlp_ln_ref.c (held to a float64 model of the formula by
test_mlp_ln_host.py); here the device's action rows are that restatement bit for bit on the device's own obs_out, and the env stepped
exactly as nig_step steps it on that action.  Shapes: closed_loop_matrix's B_BIG (700: five full 128-env blocks, one full wave and a
28-lane ragged wave) and B_SMALL (5: one partial wave), T_NEW = 7 steps of episodes of at most MAXS_NEW = 5, so that a restart falls
inside the launch."""
import ctypes as C

import numpy as np
import pytest
import torch

import closed_loop_matrix as M
import mlp_ln_ref as ref
from footprint import Arena, Layout
from test_gpu_footprint import Rig, ceil4, clean, gap, pitch
from test_gpu_mlp_shape import FILL, FLAGFILL, INVALID, SEED, UNSUPPORTED, Out, _bits, _code, _make, _play, _same

pytestmark = pytest.mark.gpu
f32 = np.float32
T = M.T_NEW


@pytest.fixture(scope="module")
def ni():
    import neorl_industrial_gym_amd as ni
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return ni


def _dims(ni, name):
    sp = ni._lib.env_spec(ni.batched.ENV_IDS[name])
    return sp.state_dim, sp.action_dim


def _policy(ni, key, S, A, seed=21):
    """ref.random_ln_actor made fit for the matrix's envs (test_gpu_mlp_shape._actor's two adjustments): the first layer scaled by
    20 / (1 + mean |s_i|) per state column, so that no single column of 1e2 .. 1e5 decides every unit's sign behind the LayerNorm, and
    AdvancedPowerGrid's two head biases that keep its episodes going."""
    ws, norms = ref.random_ln_actor(S, A, seed)
    sc = M.state_scale(ni, key, SEED)
    ws = M.continuing(key, [((ws[0][0] * f32(20.0) * sc[:, None]).astype(f32), ws[0][1]), ws[1], ws[2]])
    return ni.LayerNormMLPPolicy(ws, norms)


def _follows_the_law(oracle, o, pol, live=None):
    """every live action row is the restatement on the device's own observation, bit for bit"""
    for k in range(o["obs"].shape[0]):
        rows = slice(None) if live is None else live[k]
        want = ref.act(oracle, pol.weights, pol.norms, o["obs"][k][rows], pol.eps)
        assert np.array_equal(_bits(o["act"][k][rows]), _bits(want)), k


def _stepped_as_nig_step(ni, key, name, B, o):
    """A second handle from the same start, stepped by nig_step on the rollout's own action rows: before every step its state is the
    rollout's observation, after it reward and flag words are the rollout's, and at the end state and counters are -- bit for bit."""
    env = _make(ni, name, B)
    env.reset()
    M.install_start(ni, env, key, SEED)
    for k in range(o["obs"].shape[0]):
        assert np.array_equal(_bits(env.get_state().cpu().numpy()), _bits(o["obs"][k])), (k, "state")
        act = torch.as_tensor(o["act_raw"][k], device=env.device)
        env.step(act[:, :B], layout="soa")
        torch.cuda.synchronize()
        assert np.array_equal(_bits(env.reward.cpu().numpy()[:B]), _bits(o["rew"][k][:B])), (k, "reward")
        assert np.array_equal(env.flags.cpu().numpy().view(np.uint32)[:B], o["flags"][k]), (k, "flags")
    assert np.array_equal(_bits(env.get_state().cpu().numpy()), _bits(o["state"])) and np.array_equal(env.ctr.cpu().numpy(), o["ctr"])
    assert np.array_equal(env.reduce_tally().cpu().numpy().view(np.uint64), o["tally"].view(np.uint64))
    env.close()


# ---- 1. the anchor ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [M.B_BIG, M.B_SMALL])
@pytest.mark.parametrize("key,name", M.MFMA_ENVS)
def test_actions_are_the_law_bit_for_bit_and_the_env_stepped_as_nig_step(ni, oracle, key, name, B):
    S, A = _dims(ni, name)
    pol = _policy(ni, key, S, A)

    def install(env):
        assert env.mlp_policy_norm is False and env.mlp_policy_dims == ()
        env.set_mlp_policy_ln(pol)
        assert env.mlp_policy_norm is True and env.mlp_policy_dims == (256, 256)
    o = _play(ni, key, name, B, install, n=T)
    assert not (o["flags"] & ni._lib.FLAG_INACTIVE).any() and np.isfinite(o["act"]).all()
    _follows_the_law(oracle, o, pol)
    _stepped_as_nig_step(ni, key, name, B, o)
    assert M.distinct_rows(o["act"][0]) >= min(B, 4), "the lanes' actions differ"
    assert (np.abs(o["act"][0]) < 1).mean() > 0.5, "most actions lie inside the tanh's range"
    fl = o["flags"]
    assert key == "apg" or ((fl & ni._lib.FLAG_DID_RESET) != 0).any(), "a restart falls inside the launch"
    if key in M.FLOAT64_KEYS:                                   # the shapes only the matrix reaches: also held to the float64 formula
        want = ref.model64(pol.weights, pol.norms, o["obs"][0])["action"]
        assert M.worst(f"{key}: actions against the float64 model", o["act"][0], want, M.ACT_ATOL) <= 1.0


# ---- 2. the layout: every hidden unit is where the law says ------------------------------------------------------------------------
def layout_policy(S, A):
    """Weights that make every hidden unit identifiable: gamma in [0.5, 1.5] and beta in [4, 5], 256 distinct values each in a shuffled
    order -- a unit of either layer is active on all but a few lanes in a thousand (y = gamma x a normalised value + beta), so trading
    two units' gamma or beta moves both layers' outputs on every lane -- and a head scaled by 1 / 32, which keeps tanh away from +-1."""
    ws, _ = ref.random_ln_actor(S, A, 33)
    rng = np.random.default_rng(35)
    norms = [((0.5 + rng.permutation(256) / 256.0).astype(f32), (4.0 + rng.permutation(256) / 256.0).astype(f32)) for _ in range(2)]
    return [ws[0], ws[1], ((ws[2][0] / f32(32)).astype(f32), ws[2][1])], norms


@pytest.mark.parametrize("key,name", M.MFMA_ENVS[:2])          # ChemicalReactor: the 4 x 4 x 1 head; PowerGrid: the 16 x 16 x 1 head
def test_every_hidden_unit_sits_in_its_own_register_and_lane_half(ni, oracle, key, name):
    """The device equals the restatement on all 700 lanes; and the restatement disagrees with the device as soon as two units' gamma or
    beta trade places on the host -- unit r with r ^ 4 (the other lane half's row of the same register), with r ^ 1 (the neighbouring
    register) and with r ^ 32 (the same place in the next tile), for every unit of both layers: a row mapped to the wrong register,
    lane half or tile would have to show."""
    S, A = _dims(ni, name)
    B, n = M.B_BIG, 8
    pol = ni.LayerNormMLPPolicy(*layout_policy(S, A))
    # states of this test's own, N(0, 1) in every column (one step: the actor sees them as they are)
    x = np.random.default_rng(34).normal(0, 1, (B, S)).astype(f32)
    o = _play(ni, key, name, B, lambda env: env.set_mlp_policy_ln(pol), n=1, states=x)
    assert np.array_equal(_bits(o["obs"][0]), _bits(x))
    _follows_the_law(oracle, o, pol)
    obs, got = x[:n], _bits(o["act"][0][:n])
    assert np.abs(o["act"][0]).max() < 0.999 and M.distinct_rows(o["act"][0]) == B
    _, h1, h2 = ref.pre(pol.weights, pol.norms, obs, pol.eps, hidden=True)
    assert (h1 > 0).mean() > 0.99 and (h2 > 0).mean() > 0.99 and (h1 > 0).any(axis=0).all() and (h2 > 0).any(axis=0).all(), \
        "every unit is active on the compared lanes: its gamma and beta reach the output"
    survived = []
    for layer in range(2):
        for which in range(2):
            for flip in (4, 1, 32):
                for r in range(256):
                    if r & flip:
                        continue
                    norms = [list(nb) for nb in pol.norms]
                    arr = norms[layer][which].copy()
                    arr[[r, r ^ flip]] = arr[[r ^ flip, r]]
                    norms[layer][which] = arr
                    if np.array_equal(_bits(ref.act(oracle, pol.weights, norms, obs, pol.eps)), got):
                        survived.append((layer, which, flip, r))
    assert not survived, survived[:8]


# ---- 3. the actor slot -------------------------------------------------------------------------------------------------------------
def test_the_installs_replace_each_others_actor(ni):
    key, name, B = "cr", "ChemicalReactor-v0", M.B_BIG
    S, A = 12, 3
    pol, reference = _policy(ni, key, S, A), M.random_actor(S, A, 5)
    import mlp_shape_ref
    shaped = mlp_shape_ref.random_actor(S, A, (128, 128), 3)
    fresh_ln = _play(ni, key, name, B, lambda env: env.set_mlp_policy_ln(pol), n=T)
    fresh_reference = _play(ni, key, name, B, lambda env: env.set_mlp_policy(reference), n=T)
    fresh_shaped = _play(ni, key, name, B, lambda env: env.set_mlp_policy_dims(shaped), n=T)
    seen = []

    def note(env):
        seen.append((env.mlp_policy_norm, env.mlp_policy_dims))

    def ln_then(install_other):
        def run(env):
            note(env)
            env.set_mlp_policy_ln(pol)
            note(env)
            install_other(env)
            note(env)
        return run

    def then_ln(install_other):
        def run(env):
            install_other(env)
            env.set_mlp_policy_ln(_policy(ni, key, S, A, seed=8))     # (another LayerNorm actor first: the slot's image is reused)
            env.set_mlp_policy_ln(pol)
            note(env)
        return run
    _same(_play(ni, key, name, B, ln_then(lambda env: env.set_mlp_policy(reference)), n=T), fresh_reference)
    _same(_play(ni, key, name, B, ln_then(lambda env: env.set_mlp_policy_dims(shaped)), n=T), fresh_shaped)
    _same(_play(ni, key, name, B, then_ln(lambda env: env.set_mlp_policy(reference)), n=T), fresh_ln)
    _same(_play(ni, key, name, B, then_ln(lambda env: env.set_mlp_policy_dims(shaped)), n=T), fresh_ln)
    assert seen == [(False, ()), (True, (256, 256)), (False, (256, 256)), (False, ()), (True, (256, 256)), (False, (128, 128)),
                    (True, (256, 256)), (True, (256, 256))]
    assert not np.array_equal(fresh_ln["act"], fresh_reference["act"])


def test_an_ln_install_leaves_critic_ensemble_and_bf16_working(ni):
    name, B = "ChemicalReactor-v0", M.B_SMALL
    S, A = 12, 3
    reference = M.random_actor(S, A, 5)

    def outputs(with_ln):
        env = _make(ni, name, B)
        env.set_mlp_policy(reference)
        env.set_mlp_safety(M.random_critic(S, A, 6), 0.5)
        env.set_mlp_ensemble([reference, M.random_actor(S, A, 7)], None, None, "voting", 0.2)
        env.set_mlp_policy_bf16(reference)
        if with_ln:
            env.set_mlp_policy_ln(_policy(ni, "cr", S, A))
            env.set_mlp_policy(reference)
        res = []
        for launch in (lambda o, pr: env.rollout_mlp_safe(3, o.rw, o.fl, o.obs, o.act, pr),
                       lambda o, pr: env.rollout_mlp_ensemble(3, o.rw, o.fl, o.obs, o.act, pr, None),
                       lambda o, pr: env.rollout_mlp_bf16(3, o.rw, o.fl, o.obs, o.act, None)):
            env.counter = 0
            env.reset()
            o, pr = Out(env, 3), torch.full((3, env.ld), FILL, dtype=torch.float32, device=env.device)
            launch(o, pr)
            d = o.numpy()
            d["pr"] = pr.cpu().numpy()
            res.append(d)
        env.close()
        return res
    for a, b in zip(outputs(False), outputs(True)):
        _same(a, b, names=("rew", "flags", "obs", "act", "pr"))


def test_ensemble_and_bf16_run_beside_an_installed_ln_actor(ni):
    """The ensemble and the bf16 actor have slots of their own: with the LayerNorm actor IN the actor slot they run as they do beside
    the reference actor."""
    name, B = "ChemicalReactor-v0", M.B_SMALL
    S, A = 12, 3
    reference = M.random_actor(S, A, 5)

    def outputs(install_actor):
        env = _make(ni, name, B)
        env.set_mlp_ensemble([reference, M.random_actor(S, A, 7)], None, None, "voting", 0.2)
        env.set_mlp_policy_bf16(reference)
        install_actor(env)
        res = []
        for launch in (lambda o, pr: env.rollout_mlp_ensemble(3, o.rw, o.fl, o.obs, o.act, pr, None),
                       lambda o, pr: env.rollout_mlp_bf16(3, o.rw, o.fl, o.obs, o.act, None)):
            env.counter = 0
            env.reset()
            o, pr = Out(env, 3), torch.full((3, env.ld), FILL, dtype=torch.float32, device=env.device)
            launch(o, pr)
            d = o.numpy()
            d["pr"] = pr.cpu().numpy()
            res.append(d)
        env.close()
        return res
    for a, b in zip(outputs(lambda env: env.set_mlp_policy(reference)), outputs(lambda env: env.set_mlp_policy_ln(_policy(ni, "cr", S, A)))):
        _same(a, b, names=("rew", "flags", "obs", "act", "pr"))


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------------
def _raw_install(env, pol, hidden=256, eps=1e-6, null=None):
    """nig_set_mlp_policy_ln itself: its return code; `null`: the index of a pointer argument passed as NULL"""
    (W1, b1), (W2, b2), (W3, b3) = [(np.ascontiguousarray(W, dtype=f32), np.ascontiguousarray(b, dtype=f32)) for W, b in pol.weights]
    (g1, e1), (g2, e2) = [(np.ascontiguousarray(g, dtype=f32), np.ascontiguousarray(b, dtype=f32)) for g, b in pol.norms]
    keep = [W1, b1, g1, e1, W2, b2, g2, e2, W3, b3]
    ptrs = [None if i == null else a.ctypes.data_as(C.c_void_p) for i, a in enumerate(keep)]
    with torch.cuda.device(env.device):
        return env._L.nig_set_mlp_policy_ln(env._h, hidden, *ptrs, C.c_float(eps), env._stream())


def test_with_an_ln_actor_the_other_families_refuse_and_launch_nothing(ni):
    name, B = "ChemicalReactor-v0", M.B_SMALL
    S, A = 12, 3
    env = _make(ni, name, B)
    env.reset()
    env.set_mlp_policy(M.random_actor(S, A, 5))                # every prerequisite of every family, installed beside the reference actor
    env.set_mlp_safety(M.random_critic(S, A, 6), 0.5)
    env.set_mlp_safety_ensemble([M.random_critic(S, A, 8, n_out=2), M.random_critic(S, A, 9, n_out=2)], 1.0, 0.5, 0.2)
    env.set_mlp_constraint(M.random_critic(S, A, 10, n_out=3), 0.5, 0.01)
    env.set_disturbance(ni.Disturbance(obs_noise=0.1, action_noise=0.1, clip=(-1, 1), hold="step"))
    env.set_mlp_policy_ln(_policy(ni, "cr", S, A))
    o = Out(env, 1)
    ch = torch.full((1, env.ld), FLAGFILL, dtype=torch.int32, device=env.device)
    rows = {n: torch.full((1, env.ld), FILL, dtype=torch.float32, device=env.device) for n in ("pr", "rk")}
    xf = torch.full((1, env.ld), FLAGFILL, dtype=torch.int32, device=env.device)
    families = {"rollout_mlp_safe": lambda: env.rollout_mlp_safe(1, o.rw, o.fl, o.obs, o.act, rows["pr"]),
                "rollout_mlp_search": lambda: env.rollout_mlp_search(1, 3, o.rw, o.fl, o.obs, o.act, rows["pr"], rows["rk"], ch),
                "rollout_mlp_gated": lambda: env.rollout_mlp_gated(1, o.rw, o.fl, o.obs, o.act),
                "rollout_mlp_projected": lambda: env.rollout_mlp_projected(1, 3, 0.1, o.rw, o.fl, o.obs, o.act, None, None, ch, None),
                "rollout_mlp_disturbed": lambda: env.rollout_mlp_disturbed(1, o.rw, o.fl, o.obs, o.act, None),
                "rollout_mlp_limited": lambda: env.rollout_mlp_limited(1, o.rw, o.fl, o.obs, o.act, xf),
                "rollout_mlp_safe_limited": lambda: env.rollout_mlp_safe_limited(1, o.rw, o.fl, o.obs, o.act, rows["pr"], xf),
                "rollout_mlp_search_limited": lambda: env.rollout_mlp_search_limited(1, 3, o.rw, o.fl, o.obs, o.act, rows["pr"], rows["rk"], ch, xf),
                "rollout_mlp_gated_limited": lambda: env.rollout_mlp_gated_limited(1, o.rw, o.fl, o.obs, o.act, xflags_out=xf),
                "rollout_mlp_projected_limited": lambda: env.rollout_mlp_projected_limited(1, 3, 0.1, o.rw, o.fl, o.obs, o.act, None, None, ch, None,
                                                                                          xflags_out=xf),
                "rollout_mlp_disturbed_limited": lambda: env.rollout_mlp_disturbed_limited(1, o.rw, o.fl, o.obs, o.act, None, xf)}
    state0, ctr0, t0 = env.get_state().clone(), env.ctr.clone(), env.counter
    for entry, call in families.items():
        assert _code(call) == UNSUPPORTED, entry
        assert "LayerNorm actor" in env._L.nig_last_error().decode(), (entry, env._L.nig_last_error())
        assert env.counter == t0 and o.untouched(), entry
        assert bool((ch == FLAGFILL).all()) and bool((xf == FLAGFILL).all()) and all(bool((r == FILL).all()) for r in rows.values()), entry
        assert torch.equal(env.get_state(), state0) and torch.equal(env.ctr, ctr0) and env.mlp_policy_norm is True, entry
    env.rollout_mlp(1, o.rw, o.fl, o.obs, o.act)               # positive control: the same buffers run
    assert not o.untouched() and env.counter == t0 + 1
    env.close()
    water = _make(ni, "WaterTreatment-v0", B)                  # odd state dim: no MFMA actor
    wpol = ni.LayerNormMLPPolicy(*ref.random_ln_actor(water.state_dim, water.action_dim, 1))
    assert _code(lambda: water.set_mlp_policy_ln(wpol)) == UNSUPPORTED
    assert water.mlp_policy_norm is False and water.mlp_policy_dims == ()
    water.close()


def test_a_refused_install_leaves_the_previous_actor_running(ni):
    key, name, B = "cr", "ChemicalReactor-v0", M.B_BIG
    S, A = 12, 3
    reference, pol = M.random_actor(S, A, 5), _policy(ni, key, S, A)
    fresh = {"reference": _play(ni, key, name, B, lambda env: env.set_mlp_policy(reference), n=T),
             "ln": _play(ni, key, name, B, lambda env: env.set_mlp_policy_ln(pol), n=T)}
    other = _policy(ni, key, S, A, seed=9)

    def refused(first):
        def run(env):
            first(env)
            kind = (env.mlp_policy_norm, env.mlp_policy_dims)
            for eps in (0.0, -1e-6, float("nan"), float("inf"), -float("inf")):
                assert _raw_install(env, other, eps=eps) == INVALID, eps
            for hidden in (128, 255, 512, 0, -256):
                assert _raw_install(env, other, hidden=hidden) == UNSUPPORTED, hidden
            for null in range(10):
                assert _raw_install(env, other, null=null) == INVALID, null
            assert env._L.nig_set_mlp_policy_ln(None, 256, *([None] * 10), C.c_float(1e-6), None) == INVALID
            assert (env.mlp_policy_norm, env.mlp_policy_dims) == kind
        return run
    _same(_play(ni, key, name, B, refused(lambda env: env.set_mlp_policy(reference)), n=T), fresh["reference"])
    _same(_play(ni, key, name, B, refused(lambda env: env.set_mlp_policy_ln(pol)), n=T), fresh["ln"])
    # eps is part of the law: another eps, other actions
    loose = ni.LayerNormMLPPolicy(pol.weights, pol.norms, eps=1e-2)
    o = _play(ni, key, name, B, lambda env: env.set_mlp_policy_ln(loose), n=1)
    assert not np.array_equal(o["act"], fresh["ln"]["act"][:1])


# ---- 5. frozen lanes ---------------------------------------------------------------------------------------------------------------
def test_frozen_lanes_store_nothing_and_live_lanes_follow_the_law(ni, oracle):
    """No auto-reset, B = 5, 7 steps of episodes of at most 5: lanes 1 and 3 are held from the start and share their wave with live
    ones, every lane is frozen once its episode ended, the last steps run with no live lane at all."""
    L = ni._lib
    key, name, B, n = "cr", "ChemicalReactor-v0", M.B_SMALL, T
    pol = _policy(ni, key, 12, 3)
    env = _make(ni, name, B, autoreset=False)
    env.set_mlp_policy_ln(pol)
    env.reset()
    held = np.array([1, 3])
    c = env.ctr.clone()
    c[torch.as_tensor(held, device=env.device)] |= L.CTR_DONE
    assert env._L.nig_set_state(env._h, None, B, C.c_void_p(c.data_ptr()), env._stream()) == 0
    torch.cuda.synchronize()
    state0, ctr0 = env.get_state().cpu().numpy().copy(), env.ctr.cpu().numpy().copy()
    out = Out(env, n)
    out.rollout_mlp()
    o = out.numpy()
    fl = o["flags"]
    live = (fl & L.FLAG_INACTIVE) == 0
    ended = live & ((fl & (L.FLAG_TERMINATED | L.FLAG_TRUNCATED)) != 0)
    is_held = np.isin(np.arange(B), held)
    assert np.array_equal(live[0], ~is_held) and np.array_equal(live[1:], live[:-1] & ~ended[:-1]) and not (fl & L.FLAG_DID_RESET).any()
    assert not live[M.MAXS_NEW:].any() and live[M.MAXS_NEW - 1].any()
    last_step = np.zeros(B, np.uint32)
    for k in range(n):
        fz = ~live[k]
        assert np.array_equal(fl[k][fz], (np.uint32(L.FLAG_INACTIVE) | (last_step << np.uint32(L.FLAG_STEP_SHIFT)))[fz]), k
        last_step = np.where(live[k], fl[k] >> np.uint32(L.FLAG_STEP_SHIFT), last_step)
        assert not _bits(o["rew"][k][:B])[fz].any(), k
        assert np.all(_bits(o["obs"][k])[fz] == _bits(f32(FILL))) and np.all(_bits(o["act"][k])[fz] == _bits(f32(FILL))), k
        assert np.all(o["act"][k][live[k]] != f32(FILL))
    state1, ctr1 = env.get_state().cpu().numpy(), env.ctr.cpu().numpy()
    assert np.array_equal(_bits(state1)[held], _bits(state0)[held]) and np.array_equal(ctr1[held], ctr0[held])
    assert np.all((ctr1.view(np.uint32) & L.CTR_DONE) != 0), "every lane ends done"
    env.close()
    _follows_the_law(oracle, o, pol, live=live)


# ---- 6. the footprint --------------------------------------------------------------------------------------------------------------
def test_footprint_at_pitches_beyond_ld(ni):
    """One canary arena (tests/footprint.py): B_BIG lanes, every output at a pitch of its own beyond ld and a step stride with a gap; the
    workspace in an arena of its own.  Pads, stride gaps, the step beyond n_steps and the red zones keep the canary; every documented
    word is written."""
    key, B, mode = "cr", M.B_BIG, "wide"
    r = Rig(ni, key, B, autoreset=True, max_steps=M.MAXS_NEW)
    S, A, ld, L = r.S, r.A, r.ld, r.L
    r.env.set_mlp_policy_ln(_policy(ni, key, S, A))
    a = Arena("cuda")
    os_, lda = pitch(mode, B, ld, 1), pitch(mode, B, ld, 2)
    assert os_ > ld and lda > ld
    rew = a.add("reward_out", "f32", Layout(T, os_, 1, os_, B))
    fl = a.add("flags_out", "flags", Layout(T, os_, 1, os_, B))
    obs = a.add("obs_out", "f32", Layout(T, ceil4(B * S) + gap(mode, 1, mult4=True), 1, B * S, B * S, lane_width=S), align=16)
    act = a.add("act_out", "f32", Layout(T, A * lda + gap(mode, 2), A, lda, B))
    a.build()
    r.reset()
    p = lambda b: C.c_void_p(b.ptr)
    rc = L.nig_rollout_mlp(r.h, T, p(rew), p(fl), os_, p(obs), obs.layout.outer_stride, p(act), lda, act.layout.outer_stride, r.st())
    assert rc == 0, L.nig_last_error()
    torch.cuda.synchronize()
    findings = [str(f) for f in a.check({b.name: dict(n_outer=T) for b in (rew, fl, obs, act)})] + r.workspace_findings()
    r.close()
    clean(findings, "nig_rollout_mlp with a LayerNorm actor")


# ---- 7. routing --------------------------------------------------------------------------------------------------------------------
class _LawAgent:
    """The law's actions computed on the host (tests/mlp_ln_ref.c + the oracle's det_tanhf), observation by observation: the agent
    evaluate_with_safety can only play through its per-step host loop -- on exactly the actions the device computes."""
    is_trained = True

    def __init__(self, oracle, pol):
        self.oracle, self.pol = oracle, pol

    def predict_device(self, obs):
        a = ref.act(self.oracle, self.pol.weights, self.pol.norms, obs.cpu().numpy(), self.pol.eps)
        return torch.as_tensor(a, device=obs.device)


def _close(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k] == pytest.approx(b[k], rel=1e-12, abs=1e-12), k


def test_evaluate_plays_an_ln_policy_with_rollout_mlp_and_equals_the_host_loop(ni, oracle):
    key, name, B = "cr", "ChemicalReactor-v0", 64
    pol = _policy(ni, key, 12, 3)
    make = lambda: ni.make_batched(name, B, tally=True, autoreset=False, max_episode_steps=M.MAXS_NEW, seed=SEED)
    benv = make()
    agent, rollout, disturbed = ni.utils._install_agent(pol, benv)
    assert agent is pol and disturbed is None and rollout is not None and rollout.__func__ is type(benv).rollout_mlp
    assert benv.mlp_policy_norm is True
    fused = ni.evaluate_with_safety(pol, benv, n_episodes=B)
    torch.cuda.synchronize()
    assert int(round(float(benv.reduce_tally()[ni._lib.T_EPISODES].item()))) == B
    henv = make()
    law = _LawAgent(oracle, pol)
    assert ni.utils._install_agent(law, henv)[1] is None
    host = ni.evaluate_with_safety(law, henv, n_episodes=B)
    assert henv.mlp_policy_norm is False
    _close(fused, host)
    assert 1.0 <= fused["length_mean"] <= M.MAXS_NEW
    # evaluate_episodes: the same round with one record per episode
    e1, e2 = make(), make()
    e_fused = ni.evaluate_episodes(pol, e1, n_episodes=B)
    e_host = ni.evaluate_episodes(law, e2, n_episodes=B)
    assert e1.mlp_policy_norm is True and e2.mlp_policy_norm is False
    e1.close(), e2.close()
    for k in e_fused:
        if k != "launches" and isinstance(e_fused[k], (int, float, np.integer, np.floating)):
            assert e_fused[k] == pytest.approx(e_host[k], rel=1e-12, abs=1e-12), k
    assert e_fused["length_mean"] == fused["length_mean"] and e_fused["return_mean"] == pytest.approx(fused["return_mean"], rel=1e-12)
    benv.close(), henv.close()
    # where the kernel family does not reach -- added constraints, an env without the MFMA actor -- the policy's torch form plays
    lim = make()
    lim.add_safety_constraint(ni.BoxConstraint("cap", {("state", 0): (-1e30, 1e30)}, penalty=0.0))
    assert ni.utils._install_agent(pol, lim)[1] is None
    res = ni.evaluate_with_safety(pol, lim, n_episodes=B)
    assert np.isfinite(res["return_mean"]) and 1.0 <= res["length_mean"] <= M.MAXS_NEW
    lim.close()
    water = ni.make_batched("WaterTreatment-v0", B, tally=True, autoreset=False, max_episode_steps=M.MAXS_NEW, seed=SEED)
    wpol = ni.LayerNormMLPPolicy(*ref.random_ln_actor(water.state_dim, water.action_dim, 1))
    assert ni.utils._install_agent(wpol, water)[1] is None
    res = ni.evaluate_with_safety(wpol, water, n_episodes=B)
    assert np.isfinite(res["return_mean"]) and 1.0 <= res["length_mean"] <= M.MAXS_NEW
    water.close()
