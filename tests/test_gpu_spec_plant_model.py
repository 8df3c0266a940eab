"""The kernels of the four build-specified plants against the float64 model of their written spec (-m gpu).

The kernels are compared with tests/spec_plant_model.py DIRECTLY, not by way of the CPU statement: the oracle only
supplies the generator's draws (gen_step_noise / gen_reset_noise; the generator is pinned by known answers elsewhere).
The tolerance is the forward-error bound the model derives; next-state decisions follow the margin rule with its 0.5 %
cap on undecidable lane-steps; reset and restart states are compared bit for bit.  Covered: the parity-mode step and
reset kernels (injected float64 draws -- instantiations no other test launches for these plants), the fast-mode step
kernel on an odd and an even launch counter, and every fused form teacher-forced along its own trajectory.
"""
import numpy as np
import pytest

import spec_plant_model as M

gpu = pytest.mark.gpu
SEED = 0x5EED
BATCHES = [1, 65, 257, 1000]     # one lane, a wave + 1, a 256-lane block + 1, a ragged multi-block batch


@pytest.fixture(scope="module")
def ni():
    import torch
    import neorl_industrial_gym_amd as ni
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return ni


def _decode(L, fl):
    fl = np.asarray(fl).astype(np.int64) & 0xFFFFFFFF
    bits = np.stack([(fl >> (L.FLAG_VIOL_SHIFT + k)) & 1 for k in range(3)], axis=-1).astype(bool)
    return dict(terminated=(fl & L.FLAG_TERMINATED) != 0, truncated=(fl & L.FLAG_TRUNCATED) != 0, bits=bits,
                viol=(fl >> L.FLAG_NVIOL_SHIFT) & 3, crit=(fl >> L.FLAG_NCRIT_SHIFT) & 3, shutdown=(fl & L.FLAG_SHUTDOWN) != 0,
                did_reset=(fl & L.FLAG_DID_RESET) != 0, inactive=(fl & L.FLAG_INACTIVE) != 0, step=(fl >> L.FLAG_STEP_SHIFT) & 0xFFFF,
                other=fl & (L.FLAG_VIOL3 | L.FLAG_NVIOL_HI | L.FLAG_SHIELDED | L.FLAG_UNCERTAIN))


_ROWS = {}


def _batch_rows(key, B):
    """B rows of the threshold + edge + dense set of the CPU tests, spread evenly so that a small batch has all three kinds"""
    if key not in _ROWS:
        P = M.plant(key)
        parts = [M.threshold_rows(P), M.edge_rows(P), M.dense_rows(P, 800, seed=11)]
        _ROWS[key] = tuple(np.concatenate([q[k] for q in parts]) for k in range(4))
    st, act, nz, sp = _ROWS[key]
    idx = np.linspace(0, len(st) - 1, B).astype(np.int64) if B < len(st) else np.arange(B) % len(st)
    return st[idx], act[idx], nz[idx], sp[idx]


def _step_once(ni, oracle, env, P, rows, layout, label, inject=True, dt=0.1, cmask=7, max_steps=None):
    """set_state + one step call against the model: next state, reward, reward64 and every StepInfo field"""
    import torch
    L = ni._lib
    st, act, nz, sp = rows
    B = len(st)
    env.set_state(st, current_step=sp, done=np.zeros(B, dtype=bool))
    t = env.counter + 1
    if not inject:
        nz = np.stack([oracle.gen_step_noise(P["name"], SEED, i, t) for i in range(B)])
    a = torch.as_tensor(act if layout == "aos" else act.T.copy(), device=env.device)
    _, rew, te, tr, info = env.step(a, step_noise=nz.T.copy() if inject else None, layout=layout)
    got = _decode(L, info.flags.cpu().numpy())
    got["state_next"] = env.get_state().cpu().numpy()
    got["reward"] = rew.cpu().numpy().astype(np.float64)
    assert np.array_equal(env.reward64.cpu().numpy(), got["reward"]), label        # the float32 reward, widened
    assert np.array_equal(te.cpu().numpy(), got["terminated"]) and np.array_equal(tr.cpu().numpy(), got["truncated"])
    assert np.array_equal(info.violation_count.cpu().numpy(), got["viol"])
    assert np.array_equal(info.critical_violations.cpu().numpy(), got["crit"])
    assert np.array_equal(info.constraint_violated.cpu().numpy().T, got["bits"])
    assert np.array_equal(info.critical_shutdown.cpu().numpy(), got["shutdown"]) and np.array_equal(info.step.cpu().numpy(), got["step"])
    assert np.array_equal(info.done.cpu().numpy(), got["terminated"] | got["truncated"])
    assert not bool(info.did_reset.any()) and not bool(info.inactive.any())
    assert not got["did_reset"].any() and not got["inactive"].any() and not got["other"].any(), label
    assert np.array_equal(got["step"], sp + 1), label
    ref = M.step(P, st, act, nz, sp, max_steps=max_steps, dt=dt, cmask=cmask)
    M.check(ref, got, label)
    # the handle's own bookkeeping follows the flags
    done = got["terminated"] | got["truncated"]
    assert np.array_equal(env.done.cpu().numpy(), done) and np.array_equal(env.current_step.cpu().numpy(), sp + 1)
    return ref, got


@gpu
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("key", M.KEYS)
def test_step_and_reset_kernels(ni, oracle, key, B):
    """Parity mode (injected float64 draws), both action layouts, and reset(init_noise=) bit for bit; then the fast-mode
    kernel on an odd and an even launch counter (the two share one generator block)."""
    P = M.plant(key)
    NP, A, S = M.dims(P)
    env = ni.make_batched(P["name"], B, seed=SEED, autoreset=False)
    env.reset()
    rows = _batch_rows(key, B)
    for layout in ("aos", "soa"):
        _step_once(ni, oracle, env, P, rows, layout, f"{key} B={B} parity step {layout}")
    z = np.random.default_rng(B).standard_normal((B, NP)).astype(np.float32) * np.float32(1.5)
    draws = np.array([y["sd0"] for y in P["y"]], dtype=np.float32).astype(np.float64) * z.astype(np.float64)
    got = env.reset(init_noise=draws.T.copy()).cpu().numpy()
    assert np.array_equal(np.ascontiguousarray(got).view(np.uint32), M.reset(P, z).view(np.uint32))
    assert int(env.current_step.sum()) == 0 and not bool(env.done.any())
    env.counter = 0
    env.reset()                                                           # fast mode: the generator's own draws, counter 0
    want = M.reset(P, draws=np.stack([oracle.gen_reset_noise(P["name"], SEED, i, 0) for i in range(B)]))
    assert np.array_equal(env.get_state().cpu().numpy().view(np.uint32), want.view(np.uint32))
    for parity in ("odd", "even"):
        assert env.counter % 2 == (0 if parity == "odd" else 1)
        _step_once(ni, oracle, env, P, rows, "soa", f"{key} B={B} fast step {parity} counter", inject=False)
    env.close()


@gpu
@pytest.mark.parametrize("key", M.KEYS)
def test_time_step_and_constraint_mask(ni, oracle, key):
    """A handle with dt = 0.05 and 37-step episodes, then the same handle with constraints 0 and 2 only (injected draws) and
    with constraints 1 and 2 only (in-kernel generator)."""
    P = M.plant(key)
    B = 257
    env = ni.make_batched(P["name"], B, seed=SEED, autoreset=False, dt=0.05, max_episode_steps=37)
    env.reset()
    st, act, nz, sp = _batch_rows(key, B)
    rows = (st, act, nz, sp % 40)
    _step_once(ni, oracle, env, P, rows, "soa", f"{key} dt=0.05", dt=0.05, max_steps=37)
    env.set_constraint_mask(5)
    ref, _ = _step_once(ni, oracle, env, P, rows, "aos", f"{key} dt=0.05 cmask=5", dt=0.05, cmask=5, max_steps=37)
    full = M.step(P, *rows, max_steps=37, dt=0.05)
    assert (full["bits"][:, 1] & ~ref["bits"][:, 1]).any()                # the mask took something away
    env.set_constraint_mask(6)                                            # constraint 0 off: the bonus still looks at its box
    ref, _ = _step_once(ni, oracle, env, P, rows, "soa", f"{key} dt=0.05 cmask=6 fast", inject=False, dt=0.05, cmask=6, max_steps=37)
    assert (full["bits"][:, 0] & ~ref["bits"][:, 0]).any()
    env.close()


@gpu
@pytest.mark.parametrize("key", M.KEYS)
def test_autoreset_step_restarts_from_the_injected_draws(ni, oracle, key):
    """Auto-reset handle in parity mode: a finishing lane restarts from model.reset of its reset_noise row, bit for bit."""
    import torch
    P = M.plant(key)
    NP, A, S = M.dims(P)
    B, L = 257, ni._lib
    env = ni.make_batched(P["name"], B, seed=SEED, autoreset=True, max_episode_steps=8)
    env.reset()
    st, act, nz, sp = _batch_rows(key, B)
    sp = (np.arange(B) % 9).astype(np.int32)
    z = np.random.default_rng(77).standard_normal((B, NP)).astype(np.float32)
    draws = np.array([y["sd0"] for y in P["y"]], dtype=np.float32).astype(np.float64) * z.astype(np.float64)
    env.set_state(st, current_step=sp, done=np.zeros(B, dtype=bool))
    final = torch.zeros(S, env.ld, dtype=torch.float32, device=env.device)
    _, rew, te, tr, info = env.step(torch.as_tensor(act, device=env.device), step_noise=nz.T.copy(), reset_noise=draws.T.copy(),
                                    final_obs=final, layout="aos")
    got = _decode(L, info.flags.cpu().numpy())
    done = got["terminated"] | got["truncated"]
    assert np.array_equal(got["did_reset"], done) and done.any() and (~done).any()
    now = env.get_state().cpu().numpy()
    assert np.array_equal(now[done].view(np.uint32), M.reset(P, z)[done].view(np.uint32))
    nxt = np.where(done[:, None], final[:, :B].t().cpu().numpy(), now)     # a finishing lane's last observation: final_obs
    got.update(state_next=nxt, reward=rew.cpu().numpy().astype(np.float64))
    M.check(M.step(P, st, act, nz, sp, max_steps=8), got, f"{key} auto-reset parity step")
    assert np.array_equal(env.current_step.cpu().numpy(), np.where(done, 0, sp + 1))
    env.close()


# ------------------------------------------------------------------------------------------------------------------
# fused forms, teacher-forced along the kernel's own trajectory
# ------------------------------------------------------------------------------------------------------------------
FB, FT, FMAX = 333, 40, 12      # not a multiple of 64, 128 or 192 lanes; several episodes per lane
_DRAWS = {}


def _draws(oracle, name, env0, B=FB, T=FT):
    """step draws [T, B, 2] of launch counters 1 .. T and reset draws [T + 1, B, NP] of counters 0 .. T"""
    k = (name, env0, B, T)
    if k not in _DRAWS:
        nz = np.array([[oracle.gen_step_noise(name, SEED, env0 + i, t) for i in range(B)] for t in range(1, T + 1)])
        rz = np.array([[oracle.gen_reset_noise(name, SEED, env0 + i, t) for i in range(B)] for t in range(T + 1)])
        _DRAWS[k] = (nz, rz)
    return _DRAWS[k]


def _verify(ni, P, label, nz, rz, act, rew, fl, tally, max_steps, *, next_obs=None, acted_obs=None, final_state=None):
    """One model evaluation over all T x B lane-steps of a fused call.

    next_obs [T, B, S]: the observation each step returned (open-loop forms; a finishing lane's row is its last
    observation, the restart state is model.reset of the generator's draws).  acted_obs [T, B, S]: the observation the
    step acted on (closed-loop forms; after a restart it IS the restart state, compared bit for bit, and the finishing
    step's own next state is not recorded).  act [T, B, A], rew / fl [T, B], tally [T_ROWS, B] or None."""
    L = ni._lib
    T, B = rew.shape
    NP, A, S = M.dims(P)
    f = _decode(L, fl)
    done_k = f["terminated"] | f["truncated"]
    assert np.array_equal(f["did_reset"], done_k) and not f["inactive"].any() and not f["other"].any(), label
    restart = np.stack([M.reset(P, draws=rz[t]) for t in range(T + 1)])              # [T + 1, B, S]
    step_pre = np.zeros((T, B), dtype=np.int64)
    for t in range(1, T):
        step_pre[t] = np.where(done_k[t - 1], 0, step_pre[t - 1] + 1)
    assert np.array_equal(f["step"], step_pre + 1), label
    bits32 = lambda x: np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    if acted_obs is None:
        pre = np.empty((T, B, S), dtype=np.float32)
        pre[0] = restart[0]
        for t in range(1, T):
            pre[t] = np.where(done_k[t - 1][:, None], restart[t], next_obs[t - 1])
        nxt, have = next_obs, np.ones((T, B), dtype=bool)
    else:
        pre = acted_obs
        assert np.array_equal(bits32(pre[0]), bits32(restart[0])), label
        for t in range(1, T):                                                         # restart states, bit for bit
            assert np.array_equal(bits32(pre[t][done_k[t - 1]]), bits32(restart[t][done_k[t - 1]])), (label, t)
        nxt = np.concatenate([pre[1:], final_state[None]])
        have = ~done_k
    if final_state is not None:
        want = np.where(done_k[T - 1][:, None], restart[T], nxt[T - 1])
        assert np.array_equal(bits32(final_state), bits32(want)), label
    ref = M.step(P, pre.reshape(T * B, S), act.reshape(T * B, A), nz.reshape(T * B, 2), step_pre.reshape(-1), max_steps=max_steps)
    got = {k: f[k].reshape((T * B,) + f[k].shape[2:]) for k in ("terminated", "truncated", "bits", "viol", "crit", "shutdown")}
    got.update(state_next=nxt.reshape(T * B, S), reward=rew.reshape(-1).astype(np.float64), state_rows=have.reshape(-1))
    out = M.check(ref, got, label)
    if tally is not None:                     # what the model's per-step decisions add up to, on decidable lanes
        done_m = (ref["terminated"] | ref["truncated"]).reshape(T, B)
        viol, crit = ref["viol"].reshape(T, B), ref["crit"].reshape(T, B)
        ok = ~out["undecidable_rows"].reshape(T, B).any(axis=0)
        eps, lens, vsum, csum, run = (np.zeros(B) for _ in range(5))
        for t in range(T):
            run += viol[t]
            eps += done_m[t]
            lens += np.where(done_m[t], step_pre[t] + 1, 0)
            vsum += np.where(done_m[t], run, 0)
            csum += np.where(done_m[t], crit[t], 0)
            run = np.where(done_m[t], 0, run)
        for row, want in ((L.T_EPISODES, eps), (L.T_LEN_SUM, lens), (L.T_VIOL, vsum), (L.T_CRIT, csum)):
            assert np.array_equal(tally[row][ok], want[ok]), (label, row)
        assert ok.mean() > 0.9 and eps.sum() >= B
    return out


def _actor(S, A, seed=11):
    rng = np.random.default_rng(seed)
    return [(rng.normal(0, 0.05 / np.sqrt(S), (S, 256)).astype(np.float32), rng.normal(0, 0.05, 256).astype(np.float32)),
            (rng.normal(0, 1.0 / 16, (256, 256)).astype(np.float32), rng.normal(0, 0.05, 256).astype(np.float32)),
            (rng.normal(0, 1.0 / 8, (256, A)).astype(np.float32), rng.normal(0, 0.1, A).astype(np.float32))]


def _trajectory(T, B, S, dev):
    """A row-major [T, B, S] trajectory whose step pitch is a multiple of four floats, as the library asks (333 x 18 and
    333 x 15 are not): a strided view of a padded buffer."""
    import torch
    pitch = (B * S + 3) // 4 * 4
    return torch.zeros(T * pitch, dtype=torch.float32, device=dev).as_strided((T, B, S), (pitch, S, 1))


def _closed_loop(ni, env, form, T, rew, fl, obs, a_out):
    """env.rollout_policy / rollout_mlp; the Python wrapper takes a contiguous trajectory only, a padded one goes to the same
    C entry point with its pitch."""
    import ctypes as C
    import torch
    if obs.is_contiguous():
        return getattr(env, form)(T, rew, fl, obs, a_out)
    rp, fp, os_, _, _, ap, lda, sa = env._closed_loop_outputs(T, rew, fl, None, a_out)
    with torch.cuda.device(env._dev_index):
        ni._lib.check(getattr(env._L, "nig_" + form)(env._h, int(T), rp, fp, os_, C.c_void_p(obs.data_ptr()), obs.stride(0), ap, lda, sa,
                                                     env._stream()))


FORMS = ["rollout_rows", "rollout_rowmajor", "rollout_sampled", "rollout_policy", "rollout_mlp"]


@gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("key", M.KEYS)
def test_fused_forms_teacher_forced(ni, oracle, key, form):
    import torch
    P = M.plant(key)
    NP, A, S = M.dims(P)
    B, T = FB, FT
    env = ni.make_batched(P["name"], B, seed=SEED, autoreset=True, tally=True, max_episode_steps=FMAX)
    if form == "rollout_mlp" and S % 2:
        with pytest.raises(ni._lib.NigError):                       # the MFMA actor exists for even state dims only
            env.set_mlp_policy(_actor(S, A))
        env.close()
        return
    dev, ld = env.device, env.ld
    nz, rz = _draws(oracle, P["name"], 0)
    rew = torch.zeros(T, ld, dtype=torch.float32, device=dev)
    fl = torch.zeros(T, ld, dtype=torch.int32, device=dev)
    env.reset()
    start = env.get_state().cpu().numpy()
    assert np.array_equal(start.view(np.uint32), M.reset(P, draws=rz[0]).view(np.uint32))
    kw = {}
    if form in ("rollout_rows", "rollout_rowmajor"):
        R = 7
        a_np = np.random.default_rng(21).uniform(-1.3, 1.3, (R, A, ld)).astype(np.float32)
        ring = torch.as_tensor(a_np, device=dev)
        if form == "rollout_rows":
            obs = torch.zeros(T, S, ld, dtype=torch.float32, device=dev)
            env.rollout(T, ring, rew, fl, obs)
            kw["next_obs"] = obs[:, :, :B].permute(0, 2, 1).contiguous().cpu().numpy()
        else:
            obs = _trajectory(T, B, S, dev)
            env.rollout(T, ring, rew, fl, obs)
            kw["next_obs"] = obs.cpu().numpy()
        act = np.stack([a_np[t % R, :, :B].T for t in range(T)])
    elif form == "rollout_sampled":
        ring = torch.stack([env.fill_actions(t + 1) for t in range(T)])
        obs = _trajectory(T, B, S, dev)
        env.rollout_sampled(T, rew, fl, obs)
        kw["next_obs"] = obs.cpu().numpy()
        act = ring[:, :, :B].permute(0, 2, 1).contiguous().cpu().numpy()
    else:
        if form == "rollout_policy":
            rng = np.random.default_rng(3)
            W = np.zeros((A, S), dtype=np.float32)
            W[:, :5] = rng.normal(0, 0.01, (A, 5))
            env.set_policy(ni.DevicePolicy(S, A, W=W, b=rng.normal(0, 0.2, A), sigma=np.full(A, 0.3), half_range=np.linspace(0, 0.2, A),
                                           p_uniform=0.1, uniform_range=0.9, clip=(-1.0, 1.0)))
        else:
            env.set_mlp_policy(_actor(S, A))
        obs = _trajectory(T, B, S, dev)
        a_out = torch.zeros(T, A, ld, dtype=torch.float32, device=dev)
        _closed_loop(ni, env, form, T, rew, fl, obs, a_out)
        kw["acted_obs"] = obs.cpu().numpy()
        act = a_out[:, :, :B].permute(0, 2, 1).contiguous().cpu().numpy()
    _verify(ni, P, f"{key} {form}", nz, rz, act, rew[:, :B].cpu().numpy(), fl[:, :B].cpu().numpy(), env.tally.cpu().numpy(), FMAX,
            final_state=env.get_state().cpu().numpy(), **kw)
    env.close()


@gpu
def test_mixed_batch_segments_teacher_forced(ni, oracle):
    """The HVAC, Water, Steel and Supply segments of ONE seven-env MixedBatchedEnv launch."""
    import torch
    names = ["ChemicalReactor-v0", "RobotAssembly-v0", "HVACControl-v0", "WaterTreatment-v0", "SteelAnnealing-v0",
             "PowerGrid-v0", "SupplyChain-v0"]
    B, T, R = FB, FT, 5
    mix = ni.MixedBatchedEnv([(n, B) for n in names], seed=SEED, autoreset=True, tally=True, max_episode_steps=FMAX)
    dev = mix.device
    mix.reset()
    a_np = np.random.default_rng(22).uniform(-1.3, 1.3, (R, mix.A_max, mix.ld)).astype(np.float32)
    ring = torch.as_tensor(a_np, device=dev)
    rew = torch.zeros(T, mix.ld, dtype=torch.float32, device=dev)
    fl = torch.zeros(T, mix.ld, dtype=torch.int32, device=dev)
    obs = torch.zeros(T, mix.S_max, mix.ld, dtype=torch.float32, device=dev)
    mix.rollout(T, ring, rew, fl, obs)
    torch.cuda.synchronize()
    rew, fl, obs = rew.cpu().numpy(), fl.cpu().numpy(), obs.cpu().numpy()
    seen = 0
    for e, o in zip(mix.envs, mix.offsets):
        if e.env_id not in M.NAMES.values():
            continue
        P = M.plant(e.env_id)
        NP, A, S = M.dims(P)
        nz, rz = _draws(oracle, e.env_id, o)
        act = np.stack([a_np[t % R, :A, o:o + B].T for t in range(T)])
        _verify(ni, P, f"{e.env_id} mixed segment", nz, rz, act, rew[:, o:o + B], fl[:, o:o + B], e.tally.cpu().numpy(), FMAX,
                next_obs=np.ascontiguousarray(obs[:, :S, o:o + B].transpose(0, 2, 1)), final_state=e.get_state().cpu().numpy())
        assert not obs[:, S:, o:o + B].any()                        # rows >= S of a segment are not touched
        seen += 1
    assert seen == 4
    mix.close()
