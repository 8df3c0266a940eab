"""gpu: the shaped MFMA actor ("nig-mlp-shape-v1", include/nig.h) -- nig_set_mlp_policy_dims and nig_rollout_mlp's dispatch on the
actor slot's kind.  The law's arithmetic is restated on the host by tests/mlp_shape_ref.c (held to a float64 network and to the
padding rule by test_mlp_shape_host.py); here the device's action rows are that restatement bit for bit on the device's own
obs_out, the env stepped on exactly that action, and the layout is checked once more without any assumption on the summation
order (integer data).  Shapes: closed_loop_matrix's B_BIG (700: six blocks, the last ragged) and B_SMALL (5: one partial wave),
3 steps of episodes of at most MAXS_NEW, so that a restart falls inside the launch."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import closed_loop_matrix as M
import mlp_shape_ref as ref

pytestmark = pytest.mark.gpu
f32 = np.float32
SEED, T, FILL, FLAGFILL = 0x5EED, 3, -7.0, 0x5A5A5A5B
INVALID, UNSUPPORTED = 1, 4
CLASS_DIMS = ref.CLASSES                               # every shipped class, installed at its full widths


@pytest.fixture(scope="module")
def ni():
    import neorl_industrial_gym_amd as ni
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return ni


def _bits(x):
    return np.ascontiguousarray(x, dtype=f32).view(np.uint32)


def _actor(ni, key, S, A, dims, seed=21):
    """ref.random_actor made fit for the matrix's envs: closed_loop_matrix.matrix_actor's two adjustments for any depth.  The first
    layer is scaled by 20 / (1 + mean |s_i|) per state column on EVERY env: at these widths the unscaled construction drives the tanh
    head of ChemicalReactor to +-1 on all 700 lanes, where an action row says nothing about its pre-activation."""
    ws = ref.random_actor(S, A, dims, seed)
    sc = M.state_scale(ni, key, SEED)
    ws[0] = ((ws[0][0] * f32(20.0) * sc[:, None]).astype(f32), ws[0][1])
    if key == "apg":
        b = np.array(ws[-1][1], dtype=f32)
        b[4:6] = 5.0
        ws[-1] = (ws[-1][0], b)
    return ws


class Out:
    """The output tensors of an n-step run, canary-filled; obs rows padded to a multiple of 4 floats (rollout_mlp() calls the C entry
    point directly: the Python method takes a contiguous [n, B, S] tensor, which `obs` is where B * S is a multiple of 4)."""
    def __init__(self, env, n):
        B, S, A, ld, dev = env.batch, env.state_dim, env.action_dim, env.ld, env.device
        self.env, self.n, self.ostep = env, n, (B * S + 3) // 4 * 4
        self.rw = torch.full((n, ld), FILL, dtype=torch.float32, device=dev)
        self.fl = torch.full((n, ld), FLAGFILL, dtype=torch.int32, device=dev)
        self.obs_rows = torch.full((n, self.ostep), FILL, dtype=torch.float32, device=dev)
        self.obs = self.obs_rows.view(n, B, S) if self.ostep == B * S else None
        self.act = torch.full((n, A, ld), FILL, dtype=torch.float32, device=dev)

    def rollout_mlp(self):
        env, P = self.env, lambda t: C.c_void_p(t.data_ptr())
        with torch.cuda.device(env.device):
            rc = env._L.nig_rollout_mlp(env._h, self.n, P(self.rw), P(self.fl), env.ld, P(self.obs_rows), self.ostep, P(self.act), env.ld,
                                        env.action_dim * env.ld, env._stream())
        assert rc == 0, env._L.nig_last_error()

    def numpy(self):
        torch.cuda.synchronize()
        B, S = self.env.batch, self.env.state_dim
        return dict(rew=self.rw.cpu().numpy(), flags=self.fl.cpu().numpy().view(np.uint32)[:, :B],
                    obs=self.obs_rows.cpu().numpy()[:, :B * S].reshape(self.n, B, S),
                    act=np.ascontiguousarray(self.act.cpu().numpy()[:, :, :B].transpose(0, 2, 1)), act_raw=self.act.cpu().numpy(),
                    flags_raw=self.fl.cpu().numpy().view(np.uint32))

    def untouched(self):
        torch.cuda.synchronize()
        return (bool((self.rw == FILL).all()) and bool((self.fl == FLAGFILL).all()) and bool((self.obs_rows == FILL).all())
                and bool((self.act == FILL).all()))


def _make(ni, name, B, autoreset=True):
    return ni.make_batched(name, B, autoreset=autoreset, tally=True, max_episode_steps=M.MAXS_NEW, seed=SEED)


def _play(ni, key, name, B, install, n=T, autoreset=True, states=None):
    env = _make(ni, name, B, autoreset)
    install(env)
    env.reset()
    if states is not None:
        env.set_state(states, current_step=0, violation_count=0, done=False)
    else:
        M.install_start(ni, env, key, SEED)
    out = Out(env, n)
    t0 = env.counter
    out.rollout_mlp()
    o = out.numpy()
    assert env.counter == t0 + n
    assert np.all(o["act_raw"][:, :, B:] == f32(FILL)) and np.all(o["rew"][:, B:] == f32(FILL)) and np.all(o["flags_raw"][:, B:] == FLAGFILL)
    o["state"], o["ctr"], o["tally"] = env.get_state().cpu().numpy().copy(), env.ctr.cpu().numpy().copy(), env.reduce_tally().cpu().numpy().copy()
    env.close()
    return o


def _same(a, b, names=("rew", "flags", "obs", "act", "state", "ctr", "tally")):
    for n in names:
        assert np.array_equal(np.ascontiguousarray(a[n]).view(np.uint8), np.ascontiguousarray(b[n]).view(np.uint8)), n


def _follows_the_law(oracle, ni, key, o, ws, B, live=None):
    """every live action row is the restatement on the device's own observation, bit for bit; the env stepped on it"""
    L = ni._lib
    live = ((o["flags"] & L.FLAG_INACTIVE) == 0) if live is None else live
    for k in range(o["obs"].shape[0]):
        want = ref.act(oracle, ws, o["obs"][k][live[k]])
        assert np.array_equal(_bits(o["act"][k][live[k]]), _bits(want)), (key, k)
    return M.check_env_steps(oracle, L, key, o["obs"], o["act"], o["flags"], SEED, M.MAXS_NEW)


# ---- 1. the anchor ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [M.B_BIG, M.B_SMALL])
@pytest.mark.parametrize("cls", ref.SHIPPED)
@pytest.mark.parametrize("key,name", M.MFMA_ENVS)
def test_actions_are_the_law_bit_for_bit_and_the_env_stepped_on_them(ni, oracle, key, name, cls, B):
    sp = ni._lib.env_spec(ni.batched.ENV_IDS[name])
    S, A = sp.state_dim, sp.action_dim
    ws = _actor(ni, key, S, A, CLASS_DIMS[cls])
    assert ni.policies.actor_shape_class(CLASS_DIMS[cls]) == cls

    def install(env):
        env.set_mlp_policy_dims(ws)
        assert env.mlp_policy_dims == CLASS_DIMS[cls]
    o = _play(ni, key, name, B, install)
    assert not (o["flags"] & ni._lib.FLAG_INACTIVE).any() and np.isfinite(o["act"]).all()
    checked = _follows_the_law(oracle, ni, key, o, ws, B)
    assert M.distinct_rows(o["act"][0]) >= min(B, 4), "the lanes' actions differ"
    assert (np.abs(o["act"][0]) < 1).mean() > 0.5, "most actions lie inside the tanh's range"
    assert checked > 0 or key == "apg" or B == M.B_SMALL


# ---- 2. the layout, whatever the summation order ------------------------------------------------------------------------------------
def _integer_net(S, A, dims, seed):
    """Small-integer weights, a few per unit, so that sum |w| |h| stays below 2^24 in every layer for integer states in [-2, 2]: every
    partial sum of every order is an exactly representable integer.  The head is scaled by a power of two that brings the largest
    pre-activation to at most 2, where tanh separates neighbouring values."""
    rng = np.random.default_rng(seed)
    ws, K = [], S
    for H in list(dims) + [A]:
        W = rng.integers(-2, 3, (K, H)) * (rng.random((K, H)) < min(1.0, 6.0 / K))
        W[rng.integers(0, K, H), np.arange(H)] = rng.choice([-2, -1, 1, 2], H)          # no unit without an input
        ws.append((W.astype(np.int64), rng.integers(-3, 4, H).astype(np.int64)))
        K = H
    return ws


@pytest.mark.parametrize("cls", ref.SHIPPED)
@pytest.mark.parametrize("key,name", M.MFMA_ENVS[:2])          # ChemicalReactor: the 4 x 4 x 1 head; PowerGrid: the 16 x 16 x 1 head
def test_layout_on_integer_data_whatever_the_order(ni, oracle, key, name, cls):
    sp = ni._lib.env_spec(ni.batched.ENV_IDS[name])
    S, A, B = sp.state_dim, sp.action_dim, M.B_BIG
    dims = CLASS_DIMS[cls]
    iw = _integer_net(S, A, dims, seed=77)
    rng = np.random.default_rng(78)
    x = rng.integers(-2, 3, (B, S)).astype(np.int64)
    h, mag = x, np.abs(x)
    for i, (W, b) in enumerate(iw):                            # the integer network, and the bound on any partial sum of any order
        mag = mag @ np.abs(W) + np.abs(b)
        assert mag.max() < 2 ** 24, (i, mag.max())
        h = h @ W + b
        if i + 1 < len(iw):
            h = np.maximum(h, 0)                               # (|relu(z)| <= |z|: mag still bounds it)
    assert all((np.maximum(x @ iw[0][0] + iw[0][1], 0) > 0).any(axis=0).sum() > d // 2 for d in dims[:1]), "most first-layer units are active"
    shift = int(np.ceil(np.log2(max(np.abs(h).max(), 1) / 2.0)))
    scale = 2.0 ** -max(shift, 0)
    ws = [(W.astype(f32), b.astype(f32)) for W, b in iw[:-1]] + [((iw[-1][0] * scale).astype(f32), (iw[-1][1] * scale).astype(f32))]
    pre = (h * scale).astype(f32)
    assert np.array_equal(pre.astype(np.float64), h * scale) and np.abs(pre).max() <= 2.0 and len(np.unique(pre)) > 8
    want = oracle.detmath_unary("tanhf", pre)
    o = _play(ni, key, name, B, lambda env: env.set_mlp_policy_dims(ws), n=1, states=x.astype(f32))
    assert np.array_equal(_bits(o["obs"][0]), _bits(x.astype(f32)))
    assert np.array_equal(_bits(o["act"][0]), _bits(want))
    assert np.array_equal(_bits(ref.act(oracle, ws, x.astype(f32))), _bits(want)), "the restatement agrees on exact data"


# ---- 3. padded networks ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(96, 64), (300, 200)])
@pytest.mark.parametrize("key,name", M.MFMA_ENVS[:2])
def test_a_padded_network_follows_the_law_of_its_padded_form(ni, oracle, key, name, dims):
    sp = ni._lib.env_spec(ni.batched.ENV_IDS[name])
    S, A, B = sp.state_dim, sp.action_dim, M.B_BIG
    ws = _actor(ni, key, S, A, dims)
    cls = ni.policies.actor_shape_class(dims)
    padded = ni.policies.pad_actor(ws, CLASS_DIMS[cls])

    def install(env):
        env.set_mlp_policy_dims(ws)
        assert env.mlp_policy_dims == dims
    o = _play(ni, key, name, B, install)
    _follows_the_law(oracle, ni, key, o, padded, B)
    _same(o, _play(ni, key, name, B, lambda env: env.set_mlp_policy_dims(padded)))


@pytest.mark.parametrize("key,name", M.MFMA_ENVS[:2])
def test_a_reference_class_network_is_the_hand_padded_one_in_the_existing_kernel(ni, key, name):
    sp = ni._lib.env_spec(ni.batched.ENV_IDS[name])
    S, A, B = sp.state_dim, sp.action_dim, M.B_BIG
    ws = _actor(ni, key, S, A, (200, 200))
    assert ni.policies.actor_shape_class((200, 200)) == "reference"
    by_dims = _play(ni, key, name, B, lambda env: env.set_mlp_policy_dims(ws))
    by_hand = _play(ni, key, name, B, lambda env: env.set_mlp_policy(ni.policies.pad_actor(ws, (256, 256))))
    _same(by_dims, by_hand)


# ---- 4. the actor slot -------------------------------------------------------------------------------------------------------------
def test_either_install_replaces_the_others_actor(ni):
    key, name, B = "cr", "ChemicalReactor-v0", M.B_BIG
    S, A = 12, 3
    shaped, reference = _actor(ni, key, S, A, (128, 128)), M.random_actor(S, A, 5)
    fresh_shaped = _play(ni, key, name, B, lambda env: env.set_mlp_policy_dims(shaped))
    fresh_reference = _play(ni, key, name, B, lambda env: env.set_mlp_policy(reference))
    seen = []

    def shaped_then_reference(env):
        seen.append(env.mlp_policy_dims)
        env.set_mlp_policy_dims(shaped)
        seen.append(env.mlp_policy_dims)
        env.set_mlp_policy(reference)
        seen.append(env.mlp_policy_dims)

    def reference_then_shaped(env):
        env.set_mlp_policy(reference)
        env.set_mlp_policy_dims(_actor(ni, key, S, A, (512, 512)))      # (a larger class first: the slot's image is reused)
        seen.append(env.mlp_policy_dims)
        env.set_mlp_policy_dims(shaped)
        seen.append(env.mlp_policy_dims)
    _same(_play(ni, key, name, B, shaped_then_reference), fresh_reference)
    _same(_play(ni, key, name, B, reference_then_shaped), fresh_shaped)
    assert seen == [(), (128, 128), (256, 256), (512, 512), (128, 128)]


def test_a_shaped_install_leaves_critic_ensemble_and_bf16_working(ni):
    name, B = "ChemicalReactor-v0", M.B_SMALL
    S, A = 12, 3
    reference = M.random_actor(S, A, 5)

    def outputs(with_shaped):
        env = _make(ni, name, B)
        env.set_mlp_policy(reference)
        env.set_mlp_safety(M.random_critic(S, A, 6), 0.5)
        env.set_mlp_ensemble([reference, M.random_actor(S, A, 7)], None, None, "voting", 0.2)
        env.set_mlp_policy_bf16(reference)
        if with_shaped:
            env.set_mlp_policy_dims(ref.random_actor(S, A, (512, 256), 3))
            env.set_mlp_policy(reference)
        res = []
        for launch in (lambda o, pr: env.rollout_mlp_safe(T, o.rw, o.fl, o.obs, o.act, pr),
                       lambda o, pr: env.rollout_mlp_ensemble(T, o.rw, o.fl, o.obs, o.act, pr, None),
                       lambda o, pr: env.rollout_mlp_bf16(T, o.rw, o.fl, o.obs, o.act, None)):
            env.counter = 0
            env.reset()
            o, pr = Out(env, T), torch.full((T, env.ld), FILL, dtype=torch.float32, device=env.device)
            launch(o, pr)
            d = o.numpy()
            d["pr"] = pr.cpu().numpy()
            res.append(d)
        env.close()
        return res
    for a, b in zip(outputs(False), outputs(True)):
        _same(a, b, names=("rew", "flags", "obs", "act", "pr"))


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------
def _code(call):
    import neorl_industrial_gym_amd as ni
    try:
        call()
    except ni._lib.NigError as e:
        return int(re.match(r"libnig error (\d+)", str(e)).group(1))
    return 0


def test_with_a_shaped_actor_the_other_families_refuse_and_launch_nothing(ni):
    name, B = "ChemicalReactor-v0", M.B_SMALL
    S, A = 12, 3
    env = _make(ni, name, B)
    env.reset()
    env.set_mlp_policy(M.random_actor(S, A, 5))                # every prerequisite of every family, installed beside the reference actor
    env.set_mlp_safety(M.random_critic(S, A, 6), 0.5)
    env.set_mlp_safety_ensemble([M.random_critic(S, A, 8, n_out=2), M.random_critic(S, A, 9, n_out=2)], 1.0, 0.5, 0.2)
    env.set_mlp_constraint(M.random_critic(S, A, 10, n_out=3), 0.5, 0.01)
    env.set_disturbance(ni.Disturbance(obs_noise=0.1, action_noise=0.1, clip=(-1, 1), hold="step"))
    env.set_mlp_policy_dims(ref.random_actor(S, A, (128, 128), 3))
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
                "rollout_mlp_safe_limited": lambda: env.rollout_mlp_safe_limited(1, o.rw, o.fl, o.obs, o.act, rows["pr"], xf)}
    state0, ctr0, t0 = env.get_state().clone(), env.ctr.clone(), env.counter
    for entry, call in families.items():
        assert _code(call) == UNSUPPORTED, entry
        assert "shaped actor" in env._L.nig_last_error().decode(), entry
        assert env.counter == t0 and o.untouched(), entry
        assert bool((ch == FLAGFILL).all()) and bool((xf == FLAGFILL).all()) and all(bool((r == FILL).all()) for r in rows.values()), entry
        assert torch.equal(env.get_state(), state0) and torch.equal(env.ctr, ctr0) and env.mlp_policy_dims == (128, 128), entry
    env.rollout_mlp(1, o.rw, o.fl, o.obs, o.act)               # positive control: the same buffers run
    assert not o.untouched() and env.counter == t0 + 1
    # bad arguments: NIG_ERR_INVALID, and the installed actor stays
    Lc = env._L
    assert Lc.nig_get_mlp_policy_dims(None, None) == -1
    ws = [(np.ascontiguousarray(W), np.ascontiguousarray(b)) for W, b in ref.random_actor(S, A, (64, 64), 4)]
    Wp = (C.c_void_p * 4)(*[W.ctypes.data for W, _ in ws], None)
    bp = (C.c_void_p * 4)(*[b.ctypes.data for _, b in ws], None)
    hid = lambda *d: (C.c_int32 * 3)(*d)
    for n_hidden, hidden, Wa, ba in ((1, hid(64, 0, 0), Wp, bp), (4, hid(64, 64, 64), Wp, bp), (2, hid(64, 513, 0), Wp, bp), (2, hid(0, 64, 0), Wp, bp),
                                     (2, None, Wp, bp), (2, hid(64, 64, 0), None, bp), (2, hid(64, 64, 0), Wp, None),
                                     (3, hid(64, 64, 64), Wp, bp)):                   # (the fourth layer's pointer is NULL)
        assert Lc.nig_set_mlp_policy_dims(env._h, n_hidden, hidden, Wa, ba, env._stream()) == INVALID, (n_hidden, hidden)
        assert env.mlp_policy_dims == (128, 128)
    env.close()
    water = _make(ni, "WaterTreatment-v0", B)                  # odd state dim: no MFMA actor
    assert _code(lambda: water.set_mlp_policy_dims(ref.random_actor(water.state_dim, water.action_dim, (128, 128), 1))) == UNSUPPORTED
    assert water.mlp_policy_dims == ()
    water.close()


# ---- 6. frozen lanes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ref.SHIPPED)
def test_frozen_lanes_store_nothing_and_live_lanes_follow_the_law(ni, oracle, cls):
    """No auto-reset, B = 5, 7 steps of episodes of at most 5: lanes 1 and 3 are held from the start and share their wave with live
    ones, every lane is frozen once its episode ended, the last steps run with no live lane at all."""
    L = ni._lib
    key, name, B, n = "cr", "ChemicalReactor-v0", M.B_SMALL, M.T_NEW
    ws = _actor(ni, key, 12, 3, CLASS_DIMS[cls])
    env = _make(ni, name, B, autoreset=False)
    env.set_mlp_policy_dims(ws)
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
    _follows_the_law(oracle, ni, key, o, ws, B, live=live)


# ---- 7. routing --------------------------------------------------------------------------------------------------------------------
def test_evaluate_with_safety_plays_a_shaped_policy_with_rollout_mlp(ni):
    name, B, n = "ChemicalReactor-v0", 64, 128
    ws = ref.random_actor(12, 3, (128, 128), 21)
    pol = ni.MLPPolicy(ws)
    assert pol.fusable is False and pol.shape_class == "128x128" and pol.hidden_dims == (128, 128)
    benv = ni.make_batched(name, B, tally=True, autoreset=False, max_episode_steps=M.MAXS_NEW, seed=SEED)
    agent, rollout, disturbed = ni.utils._install_agent(pol, benv)
    assert agent is pol and disturbed is None and rollout is not None and rollout.__func__ is type(benv).rollout_mlp
    assert benv.mlp_policy_dims == (128, 128)
    res = ni.evaluate_with_safety(pol, benv, n_episodes=n)
    torch.cuda.synchronize()
    assert int(round(float(benv.reduce_tally()[ni._lib.T_EPISODES].item()))) == n
    # the same rounds by direct rollout_mlp calls on a second, identically seeded handle; the tallies from its rows
    L = ni._lib
    env = ni.make_batched(name, B, tally=True, autoreset=False, max_episode_steps=M.MAXS_NEW, seed=SEED)
    env.set_mlp_policy_dims(ws)
    lens, viols, rets = [], [], []
    for _ in range(n // B):
        env.ctr.fill_(L.CTR_DONE)
        env.reset(mask=torch.ones(B, dtype=torch.uint8, device=env.device))
        rw = torch.zeros(M.MAXS_NEW, env.ld, dtype=torch.float32, device=env.device)
        fl = torch.zeros(M.MAXS_NEW, env.ld, dtype=torch.int32, device=env.device)
        env.rollout_mlp(M.MAXS_NEW, rw, fl)
        torch.cuda.synchronize()
        rec = ni.episodes_from_rows(rw[:, :B].cpu().numpy(), fl[:, :B].cpu().numpy().view(np.uint32), bool(env.spec.reward_is_f32), 1)
        assert np.all(rec["count"] == 1)
        lens.append((rec["w"][0][0] & L.CTR_STEP_MASK).astype(np.int64)), viols.append((rec["w"][0][0] >> L.CTR_VIOL_SHIFT).astype(np.int64))
        rets.append(rec["ret"][0])
    env.close()
    ln, vi, ret = np.concatenate(lens), np.concatenate(viols), np.concatenate(rets)
    assert res["length_mean"] == ln.sum() / n and res["safety_violations"] == int(vi.sum())
    assert abs(res["return_mean"] - ret.sum() / n) <= 1e-5 * max(1.0, np.abs(ret).sum() / n)      # (float32 rows against the float64 tally)
    # wrapped, the same agent takes the host loop and still returns
    for wrapped in (ni.Disturbed(pol, ni.Disturbance(action_noise=0.1, clip=(-1.0, 1.0))),
                    ni.MLPPolicy(ws, safety_weights=M.random_critic(12, 3, 6), constraint_threshold=0.5).shielded()):
        _, rollout, _ = ni.utils._install_agent(wrapped, benv)
        assert rollout is None
        r = ni.evaluate_with_safety(wrapped, benv, n_episodes=B)
        assert np.isfinite(r["return_mean"]) and 1.0 <= r["length_mean"] <= M.MAXS_NEW
    benv.close()
