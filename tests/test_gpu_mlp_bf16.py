"""-m gpu: the MLP actor on the bf16 matrix unit (nig_set_mlp_policy_bf16 / nig_rollout_mlp_bf16, "nig-mlp-bf16-v1" in
include/nig.h) on every env the MFMA actor is compiled for, at the closed-loop matrix's shapes.

  1. layout: exact-integer data (tests/mlp_bf16_cases.py), h1, h2 and the action bit for bit -- no tolerance;
  2. real weights: each layer from the DEVICE's own previous layer (hid_out), inside a float32 accumulation-error radius;
  3. the step took that action: nig_step fed with act_out reproduces reward, flags and the next observation bit for bit;
  4. cut launches and repeated launches give the same bits;
  5. neighbours: the float32 actor's result is untouched, the refusals write nothing, pad columns keep their fill;
  6. evaluate_with_safety(policy.bf16(), ...) plays its episodes with rollout_mlp_bf16.

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


def _make(ni, name, B, autoreset=True):
    return ni.make_batched(name, B, autoreset=autoreset, tally=True, max_episode_steps=M.MAXS_NEW, seed=SEED)


def _run(ni, key, name, B, ws, T, launches=None, states=None, autoreset=True):
    env = _make(ni, name, B, autoreset)
    env.set_mlp_policy_bf16(ws)
    env.reset()
    if states is not None:
        env.set_state(states, current_step=0, violation_count=0, done=False)
    else:
        M.install_start(ni, env, key, SEED)
    out = Out(env, T)
    t0, k0 = env.counter, 0
    for n in (launches or (T,)):
        assert out.launch(k0, n) == 0, env._L.nig_last_error()
        k0 += n
    assert k0 == T
    o = out.numpy()
    assert env.counter == t0 + T
    out.pads_kept(o)
    o["t0"] = t0
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
@pytest.mark.parametrize("key,name,B", CASES)
def test_each_layer_from_the_devices_own_previous_layer(ni, key, name, B):
    from neorl_industrial_gym_amd.policies import bf16_round, mlp_bf16_reference
    sp = ni._lib.env_spec(ni.batched.ENV_IDS[name])
    S, A, T = sp.state_dim, sp.action_dim, 3
    ws = _real_weights(key, S, A)
    o = _run(ni, key, name, B, ws, T)
    assert np.isfinite(o["obs"]).all() and np.isfinite(o["act"]).all()
    worst = {}
    for k in range(T):
        h1, h2 = _bf_value(o["h1"][k]), _bf_value(o["h2"][k])
        ref = mlp_bf16_reference(ws, o["obs"][k], h1=h1, h2=h2)
        for layer, dev, terms in (("1", h1, 2 * S + 1), ("2", h2, 257)):
            z, e = ref["z" + layer], 2.0 * terms * 2.0 ** -24 * ref["abs" + layer]
            lo, hi = bf16_round(np.maximum(z - e, 0).astype(f32)), bf16_round(np.maximum(z + e, 0).astype(f32))
            bad = np.argwhere((dev < lo) | (dev > hi))
            assert bad.size == 0, (k, "h" + layer, len(bad), "first (lane, unit):", bad[:4].tolist())
            worst["one word, h" + layer] = min(worst.get("one word, h" + layer, 1.0), float((lo == hi).mean()))
        e3 = 2.0 * 257 * 2.0 ** -24 * ref["abs3"]
        err = np.abs(o["act"][k].astype(np.float64) - np.tanh(ref["z3"]))
        worst["action error / bound"] = max(worst.get("action error / bound", 0.0), float(np.max(err / (e3 + 3 * 2.0 ** -24))))
        assert np.all(err <= e3 + 3 * 2.0 ** -24), (k, float(err.max()))
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
    benv.close()
