"""-m gpu: the MLP actor on the bf16 matrix unit (nig_set_mlp_policy_bf16 / nig_rollout_mlp_bf16, "nig-mlp-bf16-v1" in
include/nig.h) on every env the MFMA actor is compiled for, at the closed-loop matrix's shapes.

  1. layout: exact-integer data (tests/mlp_bf16_cases.py), h1, h2 and the action bit for bit -- no tolerance;
  2. real weights: each layer from the DEVICE's own previous layer (hid_out), inside a float32 accumulation-error radius;
  3. the step took that action: nig_step fed with act_out reproduces reward, flags and the next observation bit for bit;
  4. cut launches and repeated launches give the same bits;
  5. neighbours: the float32 actor's result is untouched, the refusals write nothing, pad columns keep their fill;
  6. evaluate_with_safety(policy.bf16(), ...) plays its episodes with rollout_mlp_bf16, and its 13 aggregates are those of the rows;
  7. frozen lanes (no auto-reset; lanes held from the start, mixed with live ones in one wave): flags, reward and the untouched
     obs / act / hid words; the live lanes of the same launch under 2 and 3;
  8. the tally, the running return and the lifetime violations against the episode records of the kernel's own rows;
  9. a lane's bits do not depend on the batch size (1 .. 129 against 700), on the shard (env_index0) or on how the launch
     counter was reached;
 10. bf16-subnormal operands (set C of tests/mlp_bf16_cases.py).

Bounds of 2: e = 2 K 2^-24 abs, K the number of terms including the bias, abs = sum |term| from policies.mlp_bf16_reference: a
float32 sum of K exact terms in any order is within K 2^-24 abs of the real sum when every addition rounds to nearest, and the
matrix unit's internal rounding mode is not documented: truncation doubles the bound.  det_tanhf is within 2 ulp everywhere
(tests/test_detmath.py) and |a| <= 1: 3 2^-24 covers it and the float32 rounding of z3."""
import ctypes as C

import numpy as np
import pytest
import torch

import closed_loop_matrix as M
import mlp_bf16_cases as K

pytestmark = pytest.mark.gpu
SEED, FILL, FLAGFILL, HIDFILL = 0x5EED, -7.0, 0x5A5A5A5B, 0x7A7B
CASES = [pytest.param(k, n, B, id=f"{k}-{B}") for k, n in M.MFMA_ENVS for B in (M.B_BIG, M.B_SMALL)]
f32 = np.float32
CTR_DONE = 0x8000                 # NIG_CTR_DONE (asserted against the package's constant in the frozen-lane test)


@pytest.fixture(scope="module")
def ni():
    import neorl_industrial_gym_amd as ni
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return ni


def _bits(x):
    return np.ascontiguousarray(x, dtype=f32).view(np.uint32)


def _words(x):
    return (_bits(x) >> np.uint32(16)).astype(np.uint16)


def _bf_value(words):
    return (np.ascontiguousarray(words).astype(np.uint32) << np.uint32(16)).view(f32)


class Out:
    """The output tensors of a T-step run, canary-filled; obs rows padded to a multiple of 4 floats (the C entry point is called
    directly: the Python method takes a contiguous [n, B, S] tensor)."""
    def __init__(self, env, T, hid=True):
        B, S, A, ld, dev = env.batch, env.state_dim, env.action_dim, env.ld, env.device
        self.env, self.T, self.ostep = env, T, (B * S + 3) // 4 * 4
        self.rw = torch.full((T, ld), FILL, dtype=torch.float32, device=dev)
        self.fl = torch.full((T, ld), FLAGFILL, dtype=torch.int32, device=dev)
        self.obs = torch.full((T, self.ostep), FILL, dtype=torch.float32, device=dev)
        self.act = torch.full((T, A, ld), FILL, dtype=torch.float32, device=dev)
        self.hid = torch.full((T, 512, ld), HIDFILL, dtype=torch.int16, device=dev) if hid else None

    def launch(self, k0, n, entry="nig_rollout_mlp_bf16"):
        """Steps k0 .. k0 + n of the run in one launch; returns the status code."""
        env, P = self.env, lambda t: C.c_void_p(t.data_ptr())
        L = env._L
        tail = ()
        if entry == "nig_rollout_mlp_bf16":
            tail = (P(self.hid[k0:]), env.ld, 512 * env.ld) if self.hid is not None else (None, 0, 0)
        with torch.cuda.device(env.device):
            return getattr(L, entry)(env._h, n, P(self.rw[k0:]), P(self.fl[k0:]), env.ld, P(self.obs[k0:]), self.ostep, P(self.act[k0:]), env.ld,
                                     env.action_dim * env.ld, *tail, env._stream())

    def numpy(self):
        torch.cuda.synchronize()
        env, B, S = self.env, self.env.batch, self.env.state_dim
        o = dict(rew=self.rw.cpu().numpy(), flags=self.fl.cpu().numpy(), obs_raw=self.obs.cpu().numpy(), act_raw=self.act.cpu().numpy(),
                 hid_raw=None if self.hid is None else self.hid.cpu().numpy().view(np.uint16))
        o["obs"] = o["obs_raw"][:, :B * S].reshape(self.T, B, S)
        o["act"] = np.ascontiguousarray(o["act_raw"][:, :, :B].transpose(0, 2, 1))           # [T, B, A]
        if self.hid is not None:
            o["h1"] = np.ascontiguousarray(o["hid_raw"][:, :256, :B].transpose(0, 2, 1))    # [T, B, 256] bf16 words
            o["h2"] = np.ascontiguousarray(o["hid_raw"][:, 256:, :B].transpose(0, 2, 1))
        o["state"], o["ctr"] = env.get_state().cpu().numpy().copy(), env.ctr.cpu().numpy().copy()
        return o

    def untouched(self):
        torch.cuda.synchronize()
        return (bool((self.rw == FILL).all()) and bool((self.fl == FLAGFILL).all()) and bool((self.obs == FILL).all())
                and bool((self.act == FILL).all()) and (self.hid is None or bool((self.hid == HIDFILL).all())))

    def pads_kept(self, o):
        B, S = self.env.batch, self.env.state_dim
        assert np.all(o["rew"][:, B:] == f32(FILL)) and np.all(o["flags"][:, B:] == np.int32(FLAGFILL))
        assert np.all(o["act_raw"][:, :, B:] == f32(FILL)) and np.all(o["obs_raw"][:, B * S:] == f32(FILL))
        if o["hid_raw"] is not None:
            assert np.all(o["hid_raw"][:, :, B:] == HIDFILL)


def _make(ni, name, B, autoreset=True, env_index0=0):
    return ni.make_batched(name, B, autoreset=autoreset, tally=True, max_episode_steps=M.MAXS_NEW, seed=SEED, env_index0=env_index0)


def _hold(env, lanes):
    """Mark `lanes` done through nig_set_state's counter words (frozen until a reset); returns the installed (state, ctr)."""
    c = env.ctr.clone()
    c[torch.as_tensor(lanes, device=env.device)] |= CTR_DONE
    with torch.cuda.device(env.device):
        assert env._L.nig_set_state(env._h, None, env.batch, C.c_void_p(c.data_ptr()), env._stream()) == 0, env._L.nig_last_error()
    torch.cuda.synchronize()
    return env.get_state().cpu().numpy().copy(), env.ctr.cpu().numpy().copy()


def _run(ni, key, name, B, ws, T, launches=None, states=None, autoreset=True, env_index0=0, hold=None, counter=None):
    """hold: lanes marked done before the first launch; counter: the launch counter the first launch starts from (set after the
    reset, so that the start states are those of a run from counter 0); env_index0: lane 0's global index."""
    env = _make(ni, name, B, autoreset, env_index0)
    env.set_mlp_policy_bf16(ws)
    env.reset()
    if states is not None:
        env.set_state(states, current_step=0, violation_count=0, done=False)
    else:
        assert env_index0 == 0 or key not in M.CLONED, "a shard of a CLONED env is given its rows of the whole run's start states"
        M.install_start(ni, env, key, SEED)
    installed = _hold(env, hold) if hold is not None else None
    if counter is not None:
        env.counter = counter
    out = Out(env, T)
    t0, k0 = env.counter, 0
    for n in (launches or (T,)):
        assert out.launch(k0, n) == 0, env._L.nig_last_error()
        k0 += n
    assert k0 == T
    o = out.numpy()
    assert env.counter == t0 + T
    out.pads_kept(o)
    o["t0"], o["installed"] = t0, installed
    # what the launch leaves in the handle beside state and ctr
    o["life_viol"], o["ep_ret"] = env.life_viol.cpu().numpy().copy(), env.ep_return.cpu().numpy().copy()
    o["tally"], o["reduce_tally"] = env.tally.cpu().numpy().copy(), env.reduce_tally().cpu().numpy().copy()
    o["total_violations"] = env.total_violations.cpu().numpy().copy()
    env.close()
    return o


def _real_weights(key, S, A):
    return M.continuing(key, M.random_actor(S, A, 21))


# ---- 1. layout ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["A", "B"])
@pytest.mark.parametrize("key,name,B", CASES)
def test_layout_bit_for_bit_on_integer_data(ni, oracle, key, name, B, which):
    """Every partial sum is exactly representable, so no summation order can matter: h1, h2 are the reference's word for word,
    the action is det_tanhf of the exact z3 bit for bit."""
    from neorl_industrial_gym_amd.policies import mlp_bf16_reference
    sp = ni._lib.env_spec(ni.batched.ENV_IDS[name])
    S, A = sp.state_dim, sp.action_dim
    ws, states = (K.set_a if which == "A" else K.set_b)(key, S, A, B)
    ref = mlp_bf16_reference(ws, states)
    K.quanta_ok(ref, ws, states)                               # host assertion: all magnitudes below 2^24 quanta
    ties, lo = K.ties_and_lo(ref, states)
    if which == "B":
        assert ties >= 1 and lo >= 1
    o = _run(ni, key, name, B, ws, 1, states=states)
    assert np.array_equal(_bits(o["obs"][0]), _bits(states))
    for layer in ("h1", "h2"):
        bad = np.argwhere(o[layer][0] != _words(ref[layer]))
        assert bad.size == 0, (layer, len(bad), "first (lane, unit):", bad[:4].tolist())
    z3 = ref["z3"].astype(f32)
    assert np.array_equal(z3.astype(np.float64), ref["z3"])
    want = oracle.detmath_unary("tanhf", z3).reshape(B, A)
    bad = np.argwhere(_bits(o["act"][0]) != _bits(want))
    assert bad.size == 0, (len(bad), "first (lane, row):", bad[:4].tolist())


# ---- 2. real weights --------------------------------------------------------------------------------------------------------------
def _layers_inside_their_radius(ws, S, obs, h1w, h2w, act, worst, k):
    """One step's rows of some lanes (obs [n, S], h1w / h2w [n, 256] bf16 words, act [n, A]): each layer from the device's own
    previous layer inside the module docstring's radius; `worst` collects what the caller prints and asserts on."""
    from neorl_industrial_gym_amd.policies import bf16_round, mlp_bf16_reference
    h1, h2 = _bf_value(h1w), _bf_value(h2w)
    ref = mlp_bf16_reference(ws, obs, h1=h1, h2=h2)
    for layer, dev, terms in (("1", h1, 2 * S + 1), ("2", h2, 257)):
        z, e = ref["z" + layer], 2.0 * terms * 2.0 ** -24 * ref["abs" + layer]
        lo, hi = bf16_round(np.maximum(z - e, 0).astype(f32)), bf16_round(np.maximum(z + e, 0).astype(f32))
        bad = np.argwhere((dev < lo) | (dev > hi))
        assert bad.size == 0, (k, "h" + layer, len(bad), "first (lane, unit):", bad[:4].tolist())
        worst["one word, h" + layer] = min(worst.get("one word, h" + layer, 1.0), float((lo == hi).mean()))
    e3 = 2.0 * 257 * 2.0 ** -24 * ref["abs3"]
    err = np.abs(act.astype(np.float64) - np.tanh(ref["z3"]))
    worst["action error / bound"] = max(worst.get("action error / bound", 0.0), float(np.max(err / (e3 + 3 * 2.0 ** -24))))
    assert np.all(err <= e3 + 3 * 2.0 ** -24), (k, float(err.max()))


@pytest.mark.parametrize("key,name,B", CASES)
def test_each_layer_from_the_devices_own_previous_layer(ni, key, name, B):
    sp = ni._lib.env_spec(ni.batched.ENV_IDS[name])
    S, A, T = sp.state_dim, sp.action_dim, 3
    ws = _real_weights(key, S, A)
    o = _run(ni, key, name, B, ws, T)
    assert np.isfinite(o["obs"]).all() and np.isfinite(o["act"]).all()
    worst = {}
    for k in range(T):
        _layers_inside_their_radius(ws, S, o["obs"][k], o["h1"][k], o["h2"][k], o["act"][k], worst, k)
    print(key, B, {n: round(v, 4) for n, v in worst.items()})
    # the check discriminates: 2 e is a few 1e-4 of |z| (abs / |z| ~ 10) against bf16's spacing of 2^-8 |z|, so the interval holds one
    # word for most units (printed above: the fraction of them, the least over the steps)
    assert worst["one word, h1"] > 0.5 and worst["one word, h2"] > 0.5


# ---- 3. the step took that action -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,name,B", CASES)
def test_the_step_took_that_action(ni, key, name, B):
    """nig_step on a second handle, fed with act_out from the same state, counter word and launch counter, reproduces the reward,
    the flags and the next obs_out row bit for bit, over 4 steps with in-kernel resets (episodes of at most 5 steps)."""
    L = ni._lib
    sp = ni._lib.env_spec(ni.batched.ENV_IDS[name])
    S, A, T = sp.state_dim, sp.action_dim, 4
    o = _run(ni, key, name, B, _real_weights(key, S, A), T)
    e2 = _make(ni, name, B)
    assert not (o["flags"][:, :B] & L.FLAG_INACTIVE).any(), "auto-reset: every lane is live on every step"
    checked = 0
    for k in range(T):
        fl = o["flags"][k][:B]
        step_after = (fl.astype(np.uint32) >> L.FLAG_STEP_SHIFT).astype(np.int64)
        e2.state_soa.copy_(torch.from_numpy(np.ascontiguousarray(o["obs"][k].T)).to(e2.device))
        e2.ctr.copy_(torch.from_numpy((step_after - 1).astype(np.int32)).to(e2.device))
        e2.counter = o["t0"] + k
        nxt, rew, _, _, _ = e2.step(torch.from_numpy(np.ascontiguousarray(o["act"][k])).to(e2.device), layout="aos")
        torch.cuda.synchronize()
        nxt, rew, f2 = nxt.cpu().numpy().copy(), rew.cpu().numpy().copy(), e2.flags.cpu().numpy().copy()
        assert np.array_equal(_bits(o["rew"][k][:B]), _bits(rew)), k
        assert np.array_equal(fl[:B], f2), k
        # (the next observation on the lanes that neither finished nor reset on step k: test_the_step_took_that_action_matrix's rule)
        cont = (fl[:B] & (L.FLAG_TERMINATED | L.FLAG_TRUNCATED | L.FLAG_DID_RESET)) == 0
        nxt_dev = o["obs"][k + 1] if k + 1 < T else o["state"]
        assert np.array_equal(_bits(nxt_dev)[cont], _bits(nxt)[cont]), k
        checked += int(cont.sum())
    assert checked > (B if B > 100 else 0)
    e2.close()


# ---- 4. cut launches ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,name,B", CASES)
def test_cut_and_repeated_launches_give_the_same_bits(ni, key, name, B):
    sp = ni._lib.env_spec(ni.batched.ENV_IDS[name])
    ws = _real_weights(key, sp.state_dim, sp.action_dim)
    one = _run(ni, key, name, B, ws, 4)
    for other in (_run(ni, key, name, B, ws, 4, launches=(1, 1, 1, 1)), _run(ni, key, name, B, ws, 4)):
        for n in ("rew", "flags", "obs_raw", "act_raw", "hid_raw", "state", "ctr"):
            assert np.array_equal(one[n].view(np.uint8), other[n].view(np.uint8)), n
    # (the actions of unscaled random weights saturate on some envs; the hidden rows tell the lanes apart)
    assert M.distinct_rows(_bf_value(one["h2"][0])) >= 4, "the lanes do not share one hidden row"


# ---- 5. neighbours ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,name,B", CASES)
def test_the_float32_actor_is_untouched_by_the_bf16_install(ni, key, name, B):
    sp = ni._lib.env_spec(ni.batched.ENV_IDS[name])
    ws = _real_weights(key, sp.state_dim, sp.action_dim)
    runs = []
    for both in (False, True):
        env = _make(ni, name, B)
        if both:
            env.set_mlp_policy_bf16(M.random_actor(sp.state_dim, sp.action_dim, 99))
        env.set_mlp_policy(ws)
        if both:
            env.set_mlp_policy_bf16(M.random_actor(sp.state_dim, sp.action_dim, 98))
        env.reset()
        M.install_start(ni, env, key, SEED)
        out = Out(env, 3, hid=False)
        assert out.launch(0, 3, "nig_rollout_mlp") == 0
        runs.append(out.numpy())
        out.pads_kept(runs[-1])
        env.close()
    for n in ("rew", "flags", "obs_raw", "act_raw", "state", "ctr"):
        assert np.array_equal(runs[0][n].view(np.uint8), runs[1][n].view(np.uint8)), n


def _refused(env, out, code, text):
    t0 = env.counter
    state0, ctr0 = env.get_state().clone(), env.ctr.clone()
    rc = out.launch(0, 1)
    msg = env._L.nig_last_error().decode()
    assert rc == code and text in msg, (rc, msg)
    assert out.untouched() and env.counter == t0
    assert torch.equal(env.get_state(), state0) and torch.equal(env.ctr, ctr0)


def test_the_refusals_launch_nothing(ni):
    INVALID, UNSUPPORTED = 1, 4
    S, A = 12, 3
    env = _make(ni, "ChemicalReactor-v0", M.B_SMALL)
    env.reset()
    env.set_mlp_policy(M.random_actor(S, A, 1))                # the float32 actor is not the bf16 actor
    _refused(env, Out(env, 1), INVALID, "no bf16 actor installed")
    env.set_mlp_policy_bf16(M.random_actor(S, A, 1))
    out = Out(env, 1)
    assert out.launch(0, 1) == 0                                # positive control: the same arguments run
    assert not out.untouched()
    env.add_safety_constraint(ni.BoxConstraint("inert", {("state", 0): (-np.inf, np.inf)}, -1.0))
    _refused(env, Out(env, 1), UNSUPPORTED, "_limited")
    env.close()
    env = _make(ni, "WaterTreatment-v0", M.B_SMALL)             # odd state dim: no MFMA actor
    env.reset()
    with pytest.raises(ni._lib.NigError, match=r"libnig error 4"):
        env.set_mlp_policy_bf16(M.random_actor(env.state_dim, env.action_dim, 1))
    _refused(env, Out(env, 1), UNSUPPORTED, "env shape not supported")
    env.close()
    # hid_out's pitches below their minima
    env = _make(ni, "ChemicalReactor-v0", M.B_SMALL)
    env.reset()
    env.set_mlp_policy_bf16(M.random_actor(S, A, 1))
    out = Out(env, 1)
    P = lambda t: C.c_void_p(t.data_ptr())
    for ldh, sh in ((env.batch - 1, 512 * env.ld), (env.ld, 512 * env.ld - 1)):
        rc = env._L.nig_rollout_mlp_bf16(env._h, 1, P(out.rw), P(out.fl), env.ld, P(out.obs), out.ostep, P(out.act), env.ld, A * env.ld,
                                         P(out.hid), ldh, sh, env._stream())
        assert rc == INVALID and "bad hidden-activation pitch" in env._L.nig_last_error().decode()
        assert out.untouched() and env.counter == 0
    env.close()


# ---- 6. routing ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,name", M.MFMA_ENVS)
def test_evaluate_with_safety_plays_a_bf16_policy_with_the_bf16_kernel(ni, key, name):
    sp = ni._lib.env_spec(ni.batched.ENV_IDS[name])
    pol = ni.MLPPolicy(_real_weights(key, sp.state_dim, sp.action_dim)).bf16()
    benv = ni.make_batched(name, M.B_SMALL, tally=True, autoreset=False, max_episode_steps=M.MAXS_NEW, seed=SEED)
    calls = {"bf16": 0, "f32": 0}
    inner, inner32 = benv.rollout_mlp_bf16, benv.rollout_mlp

    def counted(*a, **k):
        calls["bf16"] += 1
        return inner(*a, **k)

    def counted32(*a, **k):
        calls["f32"] += 1
        return inner32(*a, **k)

    benv.rollout_mlp_bf16, benv.rollout_mlp = counted, counted32
    n = 2 * M.B_SMALL
    res = ni.evaluate_with_safety(pol, benv, n_episodes=n)
    assert calls["bf16"] >= 2 and calls["f32"] == 0, calls
    assert len(res) == 13 and set(res) >= {"return_mean", "length_mean", "safety_violations", "success_rate", "constraint_satisfaction_rate"}
    assert 1.0 <= res["length_mean"] <= M.MAXS_NEW + 1 and np.isfinite(res["return_mean"])
    torch.cuda.synchronize()
    assert int(round(float(benv.reduce_tally()[ni._lib.T_EPISODES].item()))) == n, "n episodes counted"
    extra = 1 if name.startswith("Advanced") else 0          # (the Advanced envs truncate on the step after the cap)
    benv.close()
    # the same rounds by direct rollout_mlp_bf16 calls on a second, identically seeded handle; the 13 aggregates from its rows
    L, B = ni._lib, M.B_SMALL
    env = ni.make_batched(name, B, tally=True, autoreset=False, max_episode_steps=M.MAXS_NEW, seed=SEED)
    env.set_mlp_policy_bf16(_real_weights(key, sp.state_dim, sp.action_dim))
    n_en, ret_f32 = int(env.spec.n_constraints), bool(env.spec.reward_is_f32)
    Tn = M.MAXS_NEW + extra
    rets, lens, viols, crits, bounds = [], [], [], [], []
    for _ in range(n // B):
        env.ctr.fill_(L.CTR_DONE)
        env.reset(mask=torch.ones(B, dtype=torch.uint8, device=env.device))
        rw = torch.zeros(Tn, env.ld, dtype=torch.float32, device=env.device)
        fl = torch.zeros(Tn, env.ld, dtype=torch.int32, device=env.device)
        env.rollout_mlp_bf16(Tn, rw, fl)
        torch.cuda.synchronize()
        r, f = rw[:, :B].cpu().numpy(), fl[:, :B].cpu().numpy().view(np.uint32)
        rec = ni.episodes_from_rows(r, f, ret_f32, 1)
        assert np.all(rec["count"] == 1), "one episode per lane and round"
        rets.append(rec["ret"][0]), lens.append((rec["w"][0][0] & L.CTR_STEP_MASK).astype(np.int64))
        viols.append((rec["w"][0][0] >> L.CTR_VIOL_SHIFT).astype(np.int64)), crits.append(((rec["w"][1][0] >> L.FLAG_NCRIT_SHIFT) & 3).astype(np.int64))
        live = (f & L.FLAG_INACTIVE) == 0
        bounds.append((np.abs(r.astype(np.float64)) * live).sum(0) * 2.0 ** -23)
    env.close()
    ret, ln, vi, cr, bound = (np.concatenate(x) for x in (rets, lens, viols, crits, bounds))
    # integer-valued entries: equal
    assert res["length_mean"] == ln.sum() / n and res["safety_violations"] == int(vi.sum()) and res["critical_violations"] == int(cr.sum())
    assert res["emergency_shutdowns"] == int((cr > 0).sum()) and res["safety_violations_per_episode"] == int(vi.sum()) / n
    assert res["length_std"] == float(np.sqrt(max((ln.astype(np.float64) ** 2).sum() / n - (ln.sum() / n) ** 2, 0.0)))
    assert res["constraint_satisfaction_rate"] == float((n_en * ln - vi).sum()) / float((n_en * ln).sum())
    # float entries: a return from the float32 rows is within sum |r| 2^-23 of the kernel's own (the bound derived in
    # tests/test_gpu_episodes.py::test_reduce_episodes_equals_the_kernels_own_tally); mean, min and max move by no more than the
    # mean / the largest of these; the standard deviation is 1-Lipschitz in the root mean square of the differences, and the
    # tally's sqrt(E[x^2] - E[x]^2) in float64 adds sqrt((n + 3) 2^-53 E[x^2]) per side
    assert abs(res["return_mean"] - ret.sum() / n) <= bound.sum() / n + 1e-15 * np.abs(ret).sum() / n
    assert abs(res["return_min"] - ret.min()) <= bound.max() and abs(res["return_max"] - ret.max()) <= bound.max()
    sd = float(np.sqrt(max((ret * ret).sum() / n - (ret.sum() / n) ** 2, 0.0)))
    assert abs(res["return_std"] - sd) <= bound.max() + 2.0 * np.sqrt((n + 3) * 2.0 ** -53 * (ret * ret).sum() / n)
    if np.all(np.abs(ret) > bound):                          # no return close enough to zero for its sign to turn
        assert res["successful_episodes"] == int((ret > 0).sum()) and res["success_rate"] == int((ret > 0).sum()) / n


# ---- 7. frozen lanes ----------------------------------------------------------------------------------------------------------------
def _held_lanes(B):
    """Every fifth lane of block 1 (128 envs per block), lanes 30 .. 34 of block 0 (both sides of a wave's edge: 32 envs per wave)
    and the last lane."""
    assert B > 256
    return sorted(set(range(128, 256, 5)) | set(range(30, 35)) | {B - 1})


@pytest.mark.parametrize("key,name", M.MFMA_ENVS)
def test_frozen_lanes_store_nothing_and_live_lanes_follow_the_law(ni, key, name):
    """No auto-reset, B = 700, 7 steps of episodes of at most 5: lanes held from the start share their waves with live ones on
    step 0, every lane is frozen once its episode ended, and the last step (the last two where truncation comes with step 5)
    runs with no live lane at all.  A frozen lane-step writes NIG_FLAG_INACTIVE | step and +0.0f and nothing else; a live one
    is held to the layer radii and to nig_step as in 2 and 3; cutting the launch changes no byte."""
    L = ni._lib
    assert L.CTR_DONE == CTR_DONE
    sp = L.env_spec(ni.batched.ENV_IDS[name])
    S, A, B, T = sp.state_dim, sp.action_dim, M.B_BIG, M.T_NEW
    ws = _real_weights(key, S, A)
    held = np.array(_held_lanes(B))
    o = _run(ni, key, name, B, ws, T, autoreset=False, hold=held)
    fl = o["flags"][:, :B].view(np.uint32)
    live = (fl & L.FLAG_INACTIVE) == 0
    ended = live & ((fl & (L.FLAG_TERMINATED | L.FLAG_TRUNCATED)) != 0)
    is_held = np.isin(np.arange(B), held)
    # the live mask follows the flags
    assert np.array_equal(live[0], ~is_held)
    assert np.array_equal(live[1:], live[:-1] & ~ended[:-1])
    assert not (fl & L.FLAG_DID_RESET).any()
    # truncation: with the step that makes the episode MAXS_NEW long (the Advanced envs: one step later, they test the episode
    # step before its increment), so every step from there on runs all-frozen
    cap = M.MAXS_NEW + (1 if name.startswith("Advanced") else 0)
    assert cap < T and not live[cap:].any() and live[cap - 1].any() and live[0].sum() == B - len(held)
    # frozen lane-steps
    last_step = np.zeros(B, np.uint32)                       # a held lane: episode step 0, as installed
    for k in range(T):
        fz = ~live[k]
        assert np.array_equal(fl[k][fz], (np.uint32(L.FLAG_INACTIVE) | (last_step << np.uint32(L.FLAG_STEP_SHIFT)))[fz]), k
        last_step = np.where(live[k], fl[k] >> np.uint32(L.FLAG_STEP_SHIFT), last_step)
        assert not _bits(o["rew"][k][:B])[fz].any(), (k, "reward of a frozen lane-step is +0.0f")
        assert np.all(_bits(o["obs"][k])[fz] == _bits(f32(FILL))) and np.all(_bits(o["act"][k])[fz] == _bits(f32(FILL))), k
        assert np.all(o["h1"][k][fz] == HIDFILL) and np.all(o["h2"][k][fz] == HIDFILL), k
        # ... and the live ones wrote every word (no bf16 of a ReLU output is the fill, no action is -7)
        assert np.all(o["h1"][k][live[k]] != HIDFILL) and np.all(o["h2"][k][live[k]] != HIDFILL) and np.all(o["act"][k][live[k]] != f32(FILL))
    state0, ctr0 = o["installed"]
    assert np.array_equal(_bits(o["state"])[held], _bits(state0)[held]) and np.array_equal(o["ctr"][held], ctr0[held])
    assert np.all((ctr0[held] & CTR_DONE) != 0) and np.all((o["ctr"].view(np.uint32) & CTR_DONE) != 0), "every lane ends done"
    # live lane-steps: the layers, and the step took that action (a second handle without auto-reset, teacher-forced)
    e2 = _make(ni, name, B, autoreset=False)
    worst, checked = {}, 0
    for k in range(cap):
        lv = live[k]
        _layers_inside_their_radius(ws, S, o["obs"][k][lv], o["h1"][k][lv], o["h2"][k][lv], o["act"][k][lv], worst, k)
        step_after = (fl[k] >> np.uint32(L.FLAG_STEP_SHIFT)).astype(np.int64)
        st = np.where(lv[:, None], o["obs"][k], o["state"])                       # (a frozen lane: a valid state; it stays frozen)
        c2 = np.where(lv, step_after - 1, CTR_DONE).astype(np.int32)
        e2.state_soa.copy_(torch.from_numpy(np.ascontiguousarray(st.T)).to(e2.device))
        e2.ctr.copy_(torch.from_numpy(c2).to(e2.device))
        e2.counter = o["t0"] + k
        a2 = np.where(lv[:, None], o["act"][k], f32(0))
        nxt, rew, _, _, _ = e2.step(torch.from_numpy(np.ascontiguousarray(a2)).to(e2.device), layout="aos")
        torch.cuda.synchronize()
        nxt, rew, f2 = nxt.cpu().numpy().copy(), rew.cpu().numpy().copy(), e2.flags.cpu().numpy().copy().view(np.uint32)
        assert np.array_equal(_bits(o["rew"][k][:B])[lv], _bits(rew)[lv]), k
        assert np.array_equal(fl[k][lv], f2[lv]), k
        cont = lv & ~ended[k]
        nxt_dev = o["obs"][k + 1] if k + 1 < T else o["state"]
        assert np.array_equal(_bits(nxt_dev)[cont], _bits(nxt)[cont]), k
        # a lane that ended keeps the state its last step left (nothing resets it)
        assert np.array_equal(_bits(o["state"])[ended[k]], _bits(nxt)[ended[k]]), k
        checked += int(cont.sum())
    e2.close()
    print(key, {n: round(v, 4) for n, v in worst.items()}, "continuing lane-steps:", checked)
    # (a lane live on the last live step continued on every step before it; RobotAssembly ends most of its episodes at once)
    assert checked >= (cap - 1) * int(live[cap - 1].sum()) > 0 and worst["one word, h1"] > 0.5 and worst["one word, h2"] > 0.5
    # cut launches: the same bytes in every output and every handle observable
    for cuts in ((2, 5), (1,) * 7):
        other = _run(ni, key, name, B, ws, T, launches=cuts, autoreset=False, hold=held)
        for n in ("rew", "flags", "obs_raw", "act_raw", "hid_raw", "state", "ctr", "life_viol", "ep_ret", "tally", "reduce_tally", "total_violations"):
            assert np.array_equal(np.ascontiguousarray(o[n]).view(np.uint8), np.ascontiguousarray(other[n]).view(np.uint8)), (cuts, n)


# ---- 8. the tally from the rows -------------------------------------------------------------------------------------------------
TALLY_ENVS = [(k, n) for k, n in M.MFMA_ENVS if k in ("cr", "pg", "ra", "hvac")]   # float32 rewards (cr) and float64; frequent (pg) and rare ends
B_TALLY = 257                                                                       # two blocks and one lane


def _violations_of(L, f):
    """The violation count of a flag word: two bits at NVIOL_SHIFT and NVIOL_HI."""
    return ((f >> np.uint32(L.FLAG_NVIOL_SHIFT)) & np.uint32(3)).astype(np.int64) + 4 * ((f & np.uint32(L.FLAG_NVIOL_HI)) != 0)


def _open(ni, key, name, B, autoreset):
    sp = ni._lib.env_spec(ni.batched.ENV_IDS[name])
    env = _make(ni, name, B, autoreset)
    env.set_mlp_policy_bf16(_real_weights(key, sp.state_dim, sp.action_dim))
    env.reset()
    return env


@pytest.mark.parametrize("key,name", TALLY_ENVS)
def test_the_tally_equals_the_records_of_the_kernels_own_rows(ni, key, name):
    """tests/test_gpu_episodes.py::test_reduce_episodes_equals_the_kernels_own_tally for this kernel (its own episode loop, its own
    hand-off to LaneTally / store_episode, both lane halves computing and one storing): one episode per lane, one launch."""
    L, B, T = ni._lib, B_TALLY, M.MAXS_NEW
    env = _open(ni, key, name, B, autoreset=False)
    out = Out(env, T, hid=False)
    assert out.launch(0, T) == 0, env._L.nig_last_error()
    log = env.episode_log(1)
    env.collect_episodes(log, T, out.rw, out.fl)
    got, want = log.reduce(B).cpu().numpy(), env.reduce_tally().cpu().numpy()
    assert np.all(log.count.cpu().numpy() == 1) and got[L.T_EPISODES] == B
    lane_ret = env.tally[L.T_RET_SUM].cpu().numpy()                     # one episode per lane: its return as the kernel summed it
    mine = log.returns[0].cpu().numpy()
    rew, fl = out.rw[:, :B].cpu().numpy(), out.fl[:, :B].cpu().numpy().view(np.uint32)
    live = (fl & L.FLAG_INACTIVE) == 0
    assert live[0].all() and ((fl & (L.FLAG_TERMINATED | L.FLAG_TRUNCATED)) != 0)[live].sum() == B
    if env.spec.reward_is_f32:
        assert np.array_equal(got[:L.T_ROWS].view(np.uint64), want.view(np.uint64)), (got, want)
        assert np.array_equal(mine.view(np.uint64), lane_ret.view(np.uint64))
    else:
        integer_rows = [L.T_EPISODES, L.T_LEN_SUM, L.T_LEN_SQ, L.T_VIOL, L.T_CRIT, L.T_SHUTDOWN, L.T_SATISFIED, L.T_CONSTRAINTS]
        assert np.array_equal(got[integer_rows], want[integer_rows])
        bound = (np.abs(rew.astype(np.float64)) * live).sum(0) * 2.0 ** -23      # (that test's derived bound)
        err = np.abs(mine - lane_ret)
        print(f"{key}: max |return - kernel's| = {err.max():.3e}, bound min {bound.min():.3e}, worst ratio {np.max(err / np.maximum(bound, 1e-300)):.3f}")
        assert np.all(err <= bound)
        if np.all(np.abs(lane_ret) > bound):
            assert got[L.T_SUCCESS] == want[L.T_SUCCESS]
    # the running return of a finished lane is cleared; the lifetime violations are the rows' violation fields, lane by lane
    assert not env.ep_return.cpu().numpy().view(np.uint64).any()
    assert np.array_equal(env.total_violations.cpu().numpy(), (_violations_of(L, fl) * live).sum(0))
    assert np.array_equal(env.life_viol.cpu().numpy(), (_violations_of(L, fl) * live).sum(0))
    env.close()


@pytest.mark.parametrize("key,name", TALLY_ENVS)
def test_several_episodes_per_lane_in_one_launch(ni, key, name):
    """Auto-reset, 12 steps of episodes of at most 5: the log collected from the rows is episodes_from_rows word for word, and the
    integer rows of the kernel's tally are what those records sum to; the running return and violations are the log's carry."""
    L, B, T, CAP = ni._lib, B_TALLY, 12, 12
    env = _open(ni, key, name, B, autoreset=True)
    out = Out(env, T, hid=False)
    assert out.launch(0, T) == 0, env._L.nig_last_error()
    log = env.episode_log(CAP)
    env.collect_episodes(log, T, out.rw, out.fl)
    torch.cuda.synchronize()
    rew, fl = out.rw[:, :B].cpu().numpy(), out.fl[:, :B].cpu().numpy().view(np.uint32)
    assert not (fl & L.FLAG_INACTIVE).any()
    want = ni.episodes_from_rows(rew, fl, bool(env.spec.reward_is_f32), CAP)
    count = log.count.cpu().numpy().view(np.uint32)
    assert np.array_equal(count, want["count"]) and count.min() >= T // M.MAXS_NEW and count.max() <= CAP
    assert np.array_equal(log.carry_ret.cpu().numpy().view(np.uint64), want["carry_ret"].view(np.uint64))
    assert np.array_equal(log.carry_w.cpu().numpy().view(np.uint32), want["carry_w"])
    have = np.arange(CAP)[:, None] < count.astype(np.int64)[None, :]
    assert np.array_equal(log.returns.cpu().numpy().view(np.uint64)[have], want["ret"].view(np.uint64)[have])
    words = log.words.cpu().numpy().view(np.uint32)
    for j in range(5):
        assert np.array_equal(words[j][have], want["w"][j][have]), f"record word {j}"
    w0, w1 = want["w"][0][have], want["w"][1][have]
    ncrit = (w1 >> np.uint32(L.FLAG_NCRIT_SHIFT)) & np.uint32(3)
    tally = env.reduce_tally().cpu().numpy()
    for row, value in ((L.T_EPISODES, int(count.sum())), (L.T_LEN_SUM, int((w0 & np.uint32(L.CTR_STEP_MASK)).sum())),
                       (L.T_VIOL, int((w0 >> np.uint32(L.CTR_VIOL_SHIFT)).sum())), (L.T_CRIT, int(ncrit.sum())), (L.T_SHUTDOWN, int((ncrit > 0).sum()))):
        assert tally[row] == value, (row, tally[row], value)
    # per lane too: a tally column is its own lane's
    assert np.array_equal(env.tally[L.T_EPISODES].cpu().numpy(), count.astype(np.float64))
    # the running episode: its return (bit for bit where the env sums in float32) and its violations are the log's carry
    run_ret, carry = env.ep_return.cpu().numpy(), want["carry_ret"]
    if env.spec.reward_is_f32:
        assert np.array_equal(run_ret.view(np.uint64), carry.view(np.uint64))
    else:
        steps_run = (env.ctr.cpu().numpy() & L.CTR_STEP_MASK).astype(np.int64)
        tail = np.arange(T)[:, None] >= (T - steps_run)[None, :]
        assert np.all(np.abs(run_ret - carry) <= (np.abs(rew.astype(np.float64)) * tail).sum(0) * 2.0 ** -23)
    assert np.array_equal(env.total_violations.cpu().numpy(), _violations_of(L, fl).sum(0))
    env.close()


# ---- 9. batch edges, lane independence, shards, launch counter ----------------------------------------------------------------------
EDGE_ENVS = [(k, n) for k, n in M.MFMA_ENVS if k in ("cr", "supply", "apg")]
T_EDGE = 4
LANE_ROWS = ("rew", "flags", "obs", "act", "h1", "h2")
_BIG = {}


def _big_run(ni, key, name):
    """The reference of the comparisons: B = 700, computed once per env, read-only."""
    if key not in _BIG:
        sp = ni._lib.env_spec(ni.batched.ENV_IDS[name])
        o = _run(ni, key, name, M.B_BIG, _real_weights(key, sp.state_dim, sp.action_dim), T_EDGE)
        for v in o.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _BIG[key] = o
    return _BIG[key]


def _same_lanes(big, o, e0, B, what):
    for n in LANE_ROWS:
        a, b = np.ascontiguousarray(big[n][:, e0:e0 + B]), np.ascontiguousarray(o[n][:, :B])
        assert a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), (what, n)
    for n in ("state", "ctr"):
        assert np.array_equal(np.ascontiguousarray(big[n][e0:e0 + B]).view(np.uint8), np.ascontiguousarray(o[n]).view(np.uint8)), (what, n)


@pytest.mark.parametrize("e0,B", [(0, 1), (0, 31), (0, 32), (0, 33), (0, 127), (0, 128), (0, 129), (128 + 37, 100), (640, 60)],
                         ids=lambda v: str(v))
@pytest.mark.parametrize("key,name", EDGE_ENVS)
def test_a_lane_depends_on_neither_the_batch_nor_the_shard(ni, key, name, e0, B):
    """Lane i of a batch of 1, 31 .. 129 (one lane; a wave of 32 envs less one, full, plus one; a block of 128 likewise) and lane
    i - env_index0 of a shard give the bits of lane i of the 700-lane run, in every row and in the final state and counter word."""
    big = _big_run(ni, key, name)
    sp = ni._lib.env_spec(ni.batched.ENV_IDS[name])
    states = np.array(M.start_states(ni, name, M.B_BIG, SEED)[e0:e0 + B]) if key in M.CLONED else None
    o = _run(ni, key, name, B, _real_weights(key, sp.state_dim, sp.action_dim), T_EDGE, states=states, env_index0=e0)
    _same_lanes(big, o, e0, B, (key, e0, B))
    if B > 1 and key not in M.CLONED:
        assert M.distinct_rows(o["obs"][0]) > B // 2, "the lanes' start states differ"


@pytest.mark.parametrize("key,name", EDGE_ENVS)
def test_the_launch_counter_is_read_and_handed_on(ni, key, name):
    """From launch counter 23: launches of 1 and 3 steps are one launch of 4; and the rows are not those of counter 0 (the envs
    with draws: the generator's key takes the counter)."""
    sp = ni._lib.env_spec(ni.batched.ENV_IDS[name])
    ws, B = _real_weights(key, sp.state_dim, sp.action_dim), 129
    one = _run(ni, key, name, B, ws, T_EDGE, counter=23)
    cut = _run(ni, key, name, B, ws, T_EDGE, counter=23, launches=(1, 3))
    assert one["t0"] == cut["t0"] == 23
    for n in ("rew", "flags", "obs_raw", "act_raw", "hid_raw", "state", "ctr", "life_viol", "ep_ret", "tally"):
        assert np.array_equal(np.ascontiguousarray(one[n]).view(np.uint8), np.ascontiguousarray(cut[n]).view(np.uint8)), n
    zero = _big_run(ni, key, name)
    assert np.array_equal(_bits(zero["obs"][0, :B]), _bits(one["obs"][0])), "the same start states"
    if key not in M.CLONED:
        assert not np.array_equal(_bits(zero["obs"][1:, :B]), _bits(one["obs"][1:])), "the draws of counter 23 are not those of counter 0"


# ---- 10. bf16-subnormal operands ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,name", M.MFMA_ENVS[:2])
def test_subnormal_operands_follow_the_law(ni, key, name):
    """Set C: state words below 2^-126 (subnormal as float32 and as bf16) and the smallest normal value meet weights of 2^100 in
    hidden units of their own, so that every product is exact and normal; h1 is the reference's word for word on every lane."""
    from neorl_industrial_gym_amd.policies import mlp_bf16_reference
    sp = ni._lib.env_spec(ni.batched.ENV_IDS[name])
    S, A, B = sp.state_dim, sp.action_dim, M.B_SMALL
    ws, states, units = K.set_c(key, S, A, B)
    ref = mlp_bf16_reference(ws, states)
    K.set_c_ok(ref, ws, states, units)
    o = _run(ni, key, name, B, ws, 1, states=states)
    assert np.array_equal(_bits(o["obs"][0]), _bits(states))
    print(key, "h1 words of the dedicated units, device:", o["h1"][0][:3, units].tolist(), "reference:", _words(ref["h1"])[:3, units].tolist())
    bad = np.argwhere(o["h1"][0] != _words(ref["h1"]))
    assert bad.size == 0, ("h1", len(bad), "first (lane, unit):", bad[:4].tolist())
    bad = np.argwhere(o["h2"][0] != _words(ref["h2"]))
    assert bad.size == 0, ("h2", len(bad), "first (lane, unit):", bad[:4].tolist())
