"""-m gpu: sensor / actuator noise inside the closed-loop kernels ("nig-disturb-v1", include/nig.h: nig_set_disturbance,
nig_rollout_policy_disturbed, nig_rollout_mlp_disturbed) and ni.evaluate_robustness.

The host restatement of the law uses only what the oracle already exposes: oracle.philox and oracle.probit_normal for the draws,
oracle.mlp_actions / oracle.policy_action for the undisturbed policy.  Every comparison is bit equality; the one statistical
statement (fused against host-loop robustness under hold="step", whose draws differ by design) uses the bar of
tests/test_reference_stats.py: 4 combined standard errors of the two samples' means."""
import ctypes as C

import numpy as np
import pytest
import torch

import closed_loop_matrix as M
from test_gpu_ensemble import _bits, _members

pytestmark = pytest.mark.gpu

# Which env brings which kernel shape: tests/closed_loop_matrix.py.  The cases at B = 3000 run the envs the module began with;
# the *_matrix tests run the disturbed MFMA actor on every env it is compiled for and the disturbed policy kernel (kinds mpc and
# pid) on all nine, at the matrix's shapes, AdvancedChemicalReactor and AdvancedPowerGrid from per-lane distinct start states.
B, T, MAXS, SEED = 3000, 14, 9, 0x5EED     # B: a partial last block of both kernels (128-env MLP blocks, 256-lane policy blocks)
LAUNCHES = (5, 9)                          # two launches for one case
FILL = -7.0                                # sentinel of the output buffers
STREAM_POLICY = 0xC0000000
POLICY_ENVS = [("cr", "ChemicalReactor-v0"), ("pg", "PowerGrid-v0"), ("ra", "RobotAssembly-v0")]
ACTOR_ENVS = POLICY_ENVS + [("hvac", "HVACControl-v0")]


@pytest.fixture(scope="module")
def ni():
    import neorl_industrial_gym_amd as ni
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return ni


def _agent(ni, name, kind):
    """(installer(env), kind, object): "actor" -> MLP weights; the others -> a DevicePolicy."""
    sp = ni._lib.env_spec(ni.batched.ENV_IDS[name])
    S, A = sp.state_dim, sp.action_dim
    if kind == "actor":
        return _members(ni, name, 1, 500)[0]
    if kind == "mpc":
        return ni.mpc_agent(S, A)
    if kind == "pid":
        return ni.pid_agent(S, A)
    if kind == "random":
        return ni.random_agent(S, A)
    assert kind == "behaviour"
    pol = ni.behaviour_policy(name, "mixed")       # epsilon-mixture (+ uniform noise on RobotAssembly); give it Gaussian noise too,
    pol.sigma = np.full(A, 0.15, dtype=np.float32)  # so that blocks +1.. of the policy stream are drawn beside +32.. and +48..
    return pol


def _install(env, kind, agent):
    if kind == "actor":
        env.set_mlp_policy(agent)
    else:
        env.set_policy(agent)


# The shape of a run: the module's own, and the closed-loop matrix's two (tests/closed_loop_matrix.py), which start the two envs
# whose reset is the same for every lane from per-lane distinct states
OWN = dict(B=B, T=T, max_steps=MAXS, launches=LAUNCHES, start=False)
MATRIX_SHAPE = {b: dict(B=b, T=M.T_NEW, max_steps=M.MAXS_NEW, launches=(3, M.T_NEW - 3), start=True) for b in (M.B_BIG, M.B_SMALL)}


def _run(ni, name, kind, agent, dist, autoreset=True, disturbed=True, fill=FILL, launches=None, shape=OWN):
    B, T = shape["B"], shape["T"]
    launches = shape["launches"] if launches is None else launches
    env = ni.make_batched(name, B, autoreset=autoreset, tally=True, max_episode_steps=shape["max_steps"], seed=SEED)
    _install(env, kind, agent)
    if dist is not None:
        env.set_disturbance(dist)
    dev, S, A, ld = env.device, env.state_dim, env.action_dim, env.ld
    # (an observation step is a multiple of 4 floats: where B * S is none, the rows are padded and the C entry points are called
    # directly -- the Python methods take contiguous [n, B, S] tensors)
    ostep = (B * S + 3) // 4 * 4
    act = torch.full((T + 1, A, ld), fill, dtype=torch.float32, device=dev)       # (row T: behind the last step)
    obs = torch.full((T + 1, ostep), fill, dtype=torch.float32, device=dev)
    seen = torch.full((T + 1, ostep), fill, dtype=torch.float32, device=dev)
    fl = torch.zeros(T + 1, ld, dtype=torch.int32, device=dev)
    rw = torch.full((T + 1, ld), fill, dtype=torch.float32, device=dev)
    P = lambda t: C.c_void_p(t.data_ptr())
    env.reset()
    if shape["start"]:
        M.install_start(ni, env, M.KEY_OF[name], SEED)
    t0, k0 = env.counter, 0
    for n in launches:
        if ostep != B * S:
            L = ni._lib.lib()
            common = (env._h, n, P(rw[k0:]), P(fl[k0:]), ld, P(obs[k0:]), ostep, P(act[k0:]), ld, A * ld)
            with torch.cuda.device(dev):
                if disturbed:
                    fn = L.nig_rollout_mlp_disturbed if kind == "actor" else L.nig_rollout_policy_disturbed
                    ni._lib.check(fn(*common, P(seen[k0:]), ostep, env._stream()))
                else:
                    ni._lib.check((L.nig_rollout_mlp if kind == "actor" else L.nig_rollout_policy)(*common, env._stream()))
        elif disturbed:
            (env.rollout_mlp_disturbed if kind == "actor" else env.rollout_policy_disturbed)(n, rw[k0:], fl[k0:], obs[k0:].view(-1, B, S), act[k0:],
                                                                                             seen[k0:].view(-1, B, S))
        else:
            (env.rollout_mlp if kind == "actor" else env.rollout_policy)(n, rw[k0:], fl[k0:], obs[k0:].view(-1, B, S), act[k0:])
        k0 += n
    assert k0 == T
    torch.cuda.synchronize()
    assert env.counter == t0 + T
    assert bool((obs[:, B * S:] == fill).all()) and bool((seen[:, B * S:] == fill).all()), "the pad words of the observation rows"
    o = dict(act_raw=act.cpu().numpy(), obs_raw=obs[:, :B * S].reshape(T + 1, B, S).cpu().numpy(), seen_raw=seen[:, :B * S].reshape(T + 1, B, S).cpu().numpy(),
             fl_raw=fl.cpu().numpy(), rw_raw=rw.cpu().numpy(), B=B, T=T, shape=shape,
             t0=t0, state=env.get_state().cpu().numpy(), ctr=env.ctr.cpu().numpy().copy(), tally=env.tally.cpu().numpy().copy(),
             ep_return=env.ep_return.cpu().numpy().copy(), life=env.life_viol.cpu().numpy().copy())
    o.update(act=o["act_raw"][:T, :, :B].transpose(0, 2, 1), obs=o["obs_raw"][:T], seen=o["seen_raw"][:T], flags=o["fl_raw"][:T, :B],
             rew=o["rw_raw"][:T, :B])
    o["live"] = (o["flags"] & ni._lib.FLAG_INACTIVE) == 0
    env.close()
    return o


def _normals(oracle, g, td, block0, n):
    """z [N, n]: normal k = word k & 3 of Philox block STREAM_POLICY + block0 + (k >> 2) at key (g, td, SEED)."""
    N, nb = g.shape[0], (n + 3) // 4
    ctr = np.zeros((N, nb, 4), dtype=np.uint32)
    ctr[:, :, 0] = (g & 0xFFFFFFFF).astype(np.uint32)[:, None]
    ctr[:, :, 1] = (g >> 32).astype(np.uint32)[:, None]
    ctr[:, :, 2] = td.astype(np.uint32)[:, None]
    ctr[:, :, 3] = np.uint32(STREAM_POLICY + block0) + np.arange(nb, dtype=np.uint32)[None, :]
    key = np.tile(np.array([SEED & 0xFFFFFFFF, SEED >> 32], dtype=np.uint32), (N * nb, 1))
    words = oracle.philox(ctr.reshape(-1, 4), key).reshape(N, nb * 4)[:, :n]
    return oracle.probit_normal(np.ascontiguousarray(words)).reshape(N, n)


def _draw_counter(ni, o, k, hold):
    """td of step k for every lane, rebuilt from the flag words: t for fresh draws, t - step_pre for held ones."""
    t = np.uint32(o["t0"] + k + 1)
    step_pre = ((o["flags"][k].astype(np.uint32) >> ni._lib.FLAG_STEP_SHIFT) & 0xFFFF) - 1
    return np.full(o["B"], t, dtype=np.uint32) if hold == "step" else (t - step_pre.astype(np.uint32)).astype(np.uint32)


# (unit of the env's states, of its actions).  The envs the matrix adds: AdvancedChemicalReactor's temperatures are
# ChemicalReactor's, AdvancedPowerGrid's per-unit voltages PowerGrid's; SteelAnnealing's zone temperatures are of the order of 700,
# SupplyChain's stocks of 100 beside rates of 4 and fractions of 0.5, WaterTreatment's pH 7 beside fractions of 0.5; every policy
# commands nominal actions in [-1, 1].
SIG = dict(cr=(0.5, 0.2), pg=(0.05, 0.3), ra=(0.02, 0.25), hvac=(0.3, 0.2),
           acr=(0.5, 0.2), apg=(0.05, 0.3), steel=(1.0, 0.2), supply=(0.3, 0.2), water=(0.2, 0.2))


def _dist(ni, key, S, A, hold, clip=(-0.9, 0.8)):
    so, sa = SIG[key]
    sig_o = (so * (1.0 + 0.1 * np.arange(S))).astype(np.float32)
    sig_o[1] = 0.0                                  # a zero entry among non-zero ones: o_1 = s_1 + 0 * z
    sig_a = (sa * (1.0 + 0.2 * np.arange(A))).astype(np.float32)
    return ni.Disturbance(obs_noise=sig_o, action_noise=sig_a, clip=clip, hold=hold)


_CACHE = {}


def _matrix_agent(ni, key, name, kind):
    agent = _agent(ni, name, kind)
    return M.continuing(key, agent) if kind == "actor" else agent


def _case(ni, key, name, kind, hold, shape=OWN):
    """One disturbed run per (env, agent, hold, shape), shared by the tests below and left unchanged."""
    ck = (key, kind, hold, shape["B"], shape["T"])
    if ck not in _CACHE:
        agent = _matrix_agent(ni, key, name, kind) if shape["start"] else _agent(ni, name, kind)
        probe = ni.make_batched(name, 1)
        S, A = probe.state_dim, probe.action_dim
        probe.close()
        d = _dist(ni, key, S, A, hold)
        _CACHE[ck] = (agent, d, _run(ni, name, kind, agent, d, shape=shape))
    return _CACHE[ck]


# the matrix: the disturbed MFMA actor on every env it is compiled for, the disturbed policy kernel (mpc, pid) on all nine
MATRIX = [(k, n, "actor") for k, n in M.MFMA_ENVS] + [(k, n, kind) for kind in ("mpc", "pid") for k, n in M.POLICY_ENVS_ALL]
# (both holds run the same kernel: the larger batch takes the held vector, the smaller one the fresh draws)
MATRIX_HOLD = {M.B_BIG: "episode", M.B_SMALL: "step"}


CASES = [(k, n, "actor") for k, n in ACTOR_ENVS] + [(k, n, kind) for kind in ("mpc", "pid", "behaviour") for k, n in POLICY_ENVS]


# ---- 1. zero is off ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("autoreset", [False, True], ids=["frozen", "autoreset"])
@pytest.mark.parametrize("key,name,kind", CASES + [("ra", "RobotAssembly-v0", "random")])
def test_zero_is_off(ni, key, name, kind, autoreset):
    _zero_is_off(ni, name, kind, _agent(ni, name, kind), autoreset, ("step", "episode"), OWN)


@pytest.mark.parametrize("B", [M.B_BIG, M.B_SMALL])
@pytest.mark.parametrize("key,name,kind", MATRIX)
def test_zero_is_off_matrix(ni, key, name, kind, B):
    """test_zero_is_off at the closed-loop matrix's shapes: 700 lanes that reset inside the launch, 5 that freeze."""
    _zero_is_off(ni, name, kind, _matrix_agent(ni, key, name, kind), B == M.B_BIG, (MATRIX_HOLD[B],), MATRIX_SHAPE[B])


def _zero_is_off(ni, name, kind, agent, autoreset, holds, shape):
    for hold in holds:
        a = _run(ni, name, kind, agent, ni.Disturbance(hold=hold), autoreset=autoreset, shape=shape)
        b = _run(ni, name, kind, agent, None, autoreset=autoreset, disturbed=False, shape=shape)
        assert a["live"][0].all() and (autoreset or not a["live"][-1].all()), "episodes must end inside the run"
        for f in ("act_raw", "obs_raw", "fl_raw", "rw_raw", "state", "ctr", "tally", "ep_return", "life"):
            assert np.array_equal(_bits(a[f]) if a[f].dtype.kind == "f" else a[f], _bits(b[f]) if b[f].dtype.kind == "f" else b[f]), (hold, f)
        assert np.array_equal(_bits(a["seen_raw"]), _bits(a["obs_raw"])), hold


# ---- 2. the draws -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hold", ["step", "episode"])
@pytest.mark.parametrize("key,name,kind", [(k, n, "actor") for k, n in ACTOR_ENVS] + [(k, n, "behaviour") for k, n in POLICY_ENVS]
                         + [("ra", "RobotAssembly-v0", "random")])
def test_the_draws(ni, oracle, key, name, kind, hold):
    """seen_out == s + sigma_obs * zo with zo rebuilt on the host from obs_out, the flag words and the launch counter."""
    if kind == "random":
        agent = _agent(ni, name, kind)
        d = _dist(ni, key, 24, 7, hold)
        o = _run(ni, name, kind, agent, d)
    else:
        agent, d, o = _case(ni, key, name, kind, hold)
    _the_draws(ni, oracle, key, d, o, hold)


@pytest.mark.parametrize("B", [M.B_BIG, M.B_SMALL])
@pytest.mark.parametrize("key,name,kind", MATRIX)
def test_the_draws_matrix(ni, oracle, key, name, kind, B):
    """test_the_draws at the closed-loop matrix's shapes."""
    agent, d, o = _case(ni, key, name, kind, MATRIX_HOLD[B], MATRIX_SHAPE[B])
    _the_draws(ni, oracle, key, d, o, MATRIX_HOLD[B])


def _the_draws(ni, oracle, key, d, o, hold):
    L, B, T = ni._lib, o["B"], o["T"]
    live = o["live"]
    assert live.all(), "auto-reset handle: every lane is live on every step"
    S = o["obs"].shape[2]
    sig_o, _ = d.sigmas(S, o["act"].shape[2])
    g = np.arange(B, dtype=np.uint64)
    second = False
    for k in range(T):
        td = _draw_counter(ni, o, k, hold)
        zo = _normals(oracle, g, td, 32, S)
        want = (o["obs"][k] + (sig_o[None, :] * zo).astype(np.float32)).astype(np.float32)
        assert np.array_equal(_bits(o["seen"][k]), _bits(want)), k
        if k + 1 < T:
            started = (o["flags"][k] & L.FLAG_DID_RESET) != 0
            step_next = (o["flags"][k + 1].astype(np.uint32) >> L.FLAG_STEP_SHIFT) & 0xFFFF
            assert np.all(step_next[started] == 1)
            second = second or bool(started.any())
    assert second, "no lane starts a second episode inside the launch"
    if hold == "episode":       # the held vector: two consecutive steps of one episode see the same offset draws
        td0, td1 = _draw_counter(ni, o, 0, hold), _draw_counter(ni, o, 1, hold)
        same = (o["flags"][0] & L.FLAG_DID_RESET) == 0
        # (the plant: an AdvancedPowerGrid episode ends whenever a[4] or a[5] is below 0.95, and the disturbance's clip keeps every
        # action at or below 0.8: each of its lanes resets on every step, so no lane holds a vector for two steps.  What holds for
        # it is the statement above: every step's offsets are those of a fresh episode, t - 0.)
        assert same.any() == (key != "apg") and np.all(td0[same] == td1[same]) and np.all(td0[same] == np.uint32(o["t0"] + 1))


# ---- 3. the action ----------------------------------------------------------------------------------------------------------
def _policy_struct(oracle, pol):
    return oracle.make_policy(kind=pol.kind, W=pol.W, b=pol.b, sigma=pol.sigma, half_range=pol.half_range, p_uniform=float(pol.p_uniform),
                              uniform_range=float(pol.uniform_range), clip=(float(pol.clip[0]), float(pol.clip[1])),
                              kp=float(pol.kp), ki=float(pol.ki), kd=float(pol.kd), setpoint=pol.setpoint)


@pytest.mark.parametrize("hold", ["step", "episode"])
@pytest.mark.parametrize("key,name,kind", CASES)
def test_the_action(ni, oracle, key, name, kind, hold):
    """act_out == clip(policy(seen_out) + sigma_act * za): the policy is the oracle's actor, or the oracle's "nig-policy-v1" law
    at the step's own t (its draws keyed at t whatever the hold) with the PID memory carried from step to step."""
    agent, d, o = _case(ni, key, name, kind, hold)
    _the_action(ni, oracle, key, kind, agent, d, o, hold)


@pytest.mark.parametrize("B", [M.B_BIG, M.B_SMALL])
@pytest.mark.parametrize("key,name,kind", MATRIX)
def test_the_action_matrix(ni, oracle, key, name, kind, B):
    """test_the_action at the closed-loop matrix's shapes.  On step 0 the actor's disturbed action on the envs only these cases
    reach is also held to the actor in NumPy float64 (the same noise term added, the same clip)."""
    agent, d, o = _case(ni, key, name, kind, MATRIX_HOLD[B], MATRIX_SHAPE[B])
    _the_action(ni, oracle, key, kind, agent, d, o, MATRIX_HOLD[B])
    if B == M.B_BIG and key in M.CLONED:
        assert M.distinct_rows(o["obs"][0]) >= 600, "step 0: the lanes are no clones of each other"


def _the_action(ni, oracle, key, kind, agent, d, o, hold):
    B, T = o["B"], o["T"]
    S, A = o["obs"].shape[2], o["act"].shape[2]
    _, sig_a = d.sigmas(S, A)
    lo, hi = d.clip
    g = np.arange(B, dtype=np.uint64)
    P = None if kind == "actor" else _policy_struct(oracle, agent)
    integ, eprev = np.zeros((B, 12), dtype=np.float32), np.zeros((B, 12), dtype=np.float32)     # (SupplyChain: 10 actions)
    clipped = 0
    for k in range(T):
        if kind == "actor":
            u = oracle.mlp_actions(key, agent, o["seen"][k])
        else:
            u = np.stack([oracle.policy_action(key, P, o["seen"][k, i], seed=SEED, env_index=i, t=o["t0"] + k + 1, integ=integ[i], eprev=eprev[i])
                          for i in range(B)])
        za = _normals(oracle, g, _draw_counter(ni, o, k, hold), 48, A)
        x = (u + (sig_a[None, :] * za).astype(np.float32)).astype(np.float32)
        x = np.where(x < lo, lo, x)
        x = np.where(x > hi, hi, x).astype(np.float32)
        clipped += int(((x == lo) | (x == hi)).sum())
        assert np.array_equal(_bits(o["act"][k]), _bits(x)), k
        if k == 0 and kind == "actor" and o["shape"]["start"] and key in M.FLOAT64_KEYS:
            x64 = np.clip(M.actor64(agent, o["seen"][0]) + (sig_a[None, :] * za).astype(np.float32), lo, hi)
            assert M.worst(f"{key} B={B}: the disturbed action of step 0 against float64", o["act"][0], x64, M.ACT_ATOL) <= 1.0
    assert 0 < clipped < B * T * A, "the disturbance's clip must bind on some actions and not on others"


# ---- 4. the plant received it -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,name,kind", [(k, n, "actor") for k, n in ACTOR_ENVS] + [(k, n, "mpc") for k, n in POLICY_ENVS])
def test_the_plant_received_it(ni, key, name, kind):
    """act_out as the action ring of nig_rollout on a fresh same-seed handle after the same reset: rewards, flags, the observation
    rows (rollout's row k is the state after step k: the disturbed run's row k + 1 where the episode goes on) and the final
    state, counters and tallies are the disturbed run's."""
    _, _, o = _case(ni, key, name, kind, "step")
    _the_plant_received_it(ni, key, name, o)


@pytest.mark.parametrize("B", [M.B_BIG, M.B_SMALL])
@pytest.mark.parametrize("key,name,kind", MATRIX)
def test_the_plant_received_it_matrix(ni, key, name, kind, B):
    """test_the_plant_received_it at the closed-loop matrix's shapes."""
    _, _, o = _case(ni, key, name, kind, MATRIX_HOLD[B], MATRIX_SHAPE[B])
    _the_plant_received_it(ni, key, name, o)


def _the_plant_received_it(ni, key, name, o):
    L, B, T, shape = ni._lib, o["B"], o["T"], o["shape"]
    env = ni.make_batched(name, B, autoreset=True, tally=True, max_episode_steps=shape["max_steps"], seed=SEED)
    dev, S = env.device, env.state_dim
    ring = torch.from_numpy(np.ascontiguousarray(o["act_raw"][:T])).to(dev)
    rw = torch.zeros(T, env.ld, dtype=torch.float32, device=dev)
    fl = torch.zeros(T, env.ld, dtype=torch.int32, device=dev)
    ostep = (B * S + 3) // 4 * 4                    # (an observation step is a multiple of 4 floats)
    obs = torch.zeros(T, ostep, dtype=torch.float32, device=dev).as_strided((T, B, S), (ostep, S, 1))
    env.reset()
    if shape["start"]:
        M.install_start(ni, env, key, SEED)
    assert env.counter == o["t0"]
    k0 = 0
    for n in shape["launches"]:      # the same launches: a launch adds the episodes that ended in it to the tally as one fp64 partial
        env.rollout(n, ring[k0:], rw[k0:], fl[k0:], obs[k0:])
        k0 += n
    torch.cuda.synchronize()
    assert np.array_equal(_bits(rw[:, :B].cpu().numpy()), _bits(o["rew"]))
    assert np.array_equal(fl[:, :B].cpu().numpy(), o["flags"])
    nxt = obs.cpu().numpy()
    cont = (o["flags"][:T - 1] & (L.FLAG_TERMINATED | L.FLAG_TRUNCATED | L.FLAG_DID_RESET)) == 0
    # (the plant: under the disturbance's clip at 0.8 every AdvancedPowerGrid episode ends on its first step -- a[4], a[5] < 0.95 --
    # so none of its lanes goes on; rewards, flags, final state, counters and tallies below still are the ring rollout's)
    assert cont.sum() > B if key != "apg" else cont.sum() == 0
    assert np.array_equal(_bits(nxt[:T - 1])[cont], _bits(o["obs"][1:])[cont])
    assert np.array_equal(_bits(env.get_state().cpu().numpy()), _bits(o["state"]))
    assert np.array_equal(env.ctr.cpu().numpy(), o["ctr"]) and np.array_equal(env.life_viol.cpu().numpy(), o["life"])
    assert np.array_equal(env.tally.cpu().numpy().view(np.uint64), o["tally"].view(np.uint64))
    assert np.array_equal(env.ep_return.cpu().numpy().view(np.uint64), o["ep_return"].view(np.uint64))
    env.close()


# ---- 5. footprint -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,name,kind", [("cr", "ChemicalReactor-v0", "actor"), ("pg", "PowerGrid-v0", "actor"), ("hvac", "HVACControl-v0", "actor"),
                                           ("cr", "ChemicalReactor-v0", "pid"), ("pg", "PowerGrid-v0", "mpc"), ("ra", "RobotAssembly-v0", "behaviour")])
def test_footprint(ni, key, name, kind):
    """Pad columns, the rows of frozen lanes in seen_out / act_out / obs_out and the row behind the last step keep the sentinel."""
    agent = _agent(ni, name, kind)
    probe = ni.make_batched(name, 1)
    S, A = probe.state_dim, probe.action_dim
    probe.close()
    o = _run(ni, name, kind, agent, _dist(ni, key, S, A, "episode"), autoreset=False)
    live = o["live"]
    assert live[0].all() and not live[-1].all()
    sent = _bits(np.float32(FILL).reshape(1))[0]
    assert np.all(_bits(o["act_raw"][:, :, B:]) == sent) and np.all(_bits(o["rw_raw"][:, B:]) == sent) and not o["fl_raw"][:, B:].any()
    for f in ("act_raw", "obs_raw", "seen_raw", "rw_raw"):
        assert np.all(_bits(o[f][T]) == sent), f                 # the row behind the last step
    assert not o["fl_raw"][T].any()
    assert np.all(_bits(o["seen"])[~live] == sent) and np.all(_bits(o["obs"])[~live] == sent) and np.all(_bits(o["act"])[~live] == sent)
    assert np.all(_bits(o["seen"])[live] != sent) and np.all(_bits(o["act"])[live] != sent)
    assert np.all(o["rew"][~live] == 0.0) and np.all((o["flags"][~live] & ni._lib.FLAG_INACTIVE) != 0)


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals(ni):
    L, lib = ni._lib, ni._lib.lib()
    INVALID, UNSUPPORTED = 1, 4
    env = ni.make_batched("ChemicalReactor-v0", 256, max_episode_steps=MAXS, seed=SEED)
    env.reset()
    S, A, dev = env.state_dim, env.action_dim, env.device
    st = env._stream()
    good = ni.Disturbance(obs_noise=0.1, action_noise=0.2, clip=(-1, 1), hold="episode")
    env.set_disturbance(good)

    def struct(**kw):
        D = good.to_struct(S, A)
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(D, k)[v[0]] = v[1]
            else:
                setattr(D, k, v)
        return D
    bad = [struct(sigma_obs=(3, -0.1)), struct(sigma_obs=(0, float("nan"))), struct(sigma_obs=(S - 1, float("inf"))),
           struct(sigma_act=(1, -1.0)), struct(sigma_act=(0, float("nan"))), struct(sigma_act=(A - 1, float("inf"))),
           struct(clip_lo=1.0, clip_hi=-1.0), struct(clip_lo=float("nan")), struct(clip_hi=float("nan")), struct(hold=2), struct(hold=-1)]
    for D in bad:
        assert lib.nig_set_disturbance(env._h, C.byref(D), st) == INVALID
        assert lib.nig_last_error().decode().startswith("nig_set_disturbance: ")
    # entries beyond the env's dimensions are not the env's: ignored
    assert lib.nig_set_disturbance(env._h, C.byref(struct(sigma_obs=(S, -1.0), sigma_act=(A, float("nan")))), st) == 0
    env.set_disturbance(good)

    rw = torch.full((2, 256), FILL, device=dev)
    fl = torch.full((2, 256), 77, dtype=torch.int32, device=dev)
    obs = torch.full((2, 256, S), FILL, device=dev)
    seen = torch.full((2, 256, S), FILL, device=dev)
    act = torch.full((2, A, 256), FILL, device=dev)
    state0, t0 = env.get_state().clone(), env.counter

    def untouched():
        torch.cuda.synchronize()
        return (bool((rw == FILL).all()) and bool((fl == 77).all()) and bool((obs == FILL).all()) and bool((seen == FILL).all())
                and bool((act == FILL).all()) and torch.equal(env.get_state(), state0) and env.counter == t0)

    def call(fn, n=2, seen_t=seen, seen_stride=None):
        return fn(env._h, n, rw.data_ptr(), fl.data_ptr(), 256, obs.data_ptr(), 256 * S, act.data_ptr(), 256, A * 256,
                  seen_t.data_ptr(), 256 * S if seen_stride is None else seen_stride, st)
    # no policy / actor installed (the disturbance is)
    assert call(lib.nig_rollout_policy_disturbed) == INVALID and b"no policy installed" in lib.nig_last_error() and untouched()
    assert call(lib.nig_rollout_mlp_disturbed) == INVALID and b"no actor installed" in lib.nig_last_error() and untouched()
    env.set_policy(ni.mpc_agent(S, A))
    env.set_mlp_policy(_members(ni, "ChemicalReactor-v0", 1, 500)[0])
    for fn in (lib.nig_rollout_policy_disturbed, lib.nig_rollout_mlp_disturbed):
        # seen_out's pitches: obs_out's rules
        assert call(fn, seen_stride=256 * S - 4) == INVALID and b"seen_out" in lib.nig_last_error() and untouched()
        assert call(fn, seen_stride=0) == INVALID and untouched()
        assert call(fn, seen_stride=256 * S + 2) == INVALID and untouched()
        assert fn(env._h, 2, rw.data_ptr(), fl.data_ptr(), 256, obs.data_ptr(), 256 * S, act.data_ptr(), 256, A * 256,
                  seen.data_ptr() + 4, 256 * S, st) == INVALID and untouched()
        assert call(fn, n=0) == INVALID and untouched()
    # no disturbance installed
    env.set_disturbance(None)
    for fn in (lib.nig_rollout_policy_disturbed, lib.nig_rollout_mlp_disturbed):
        assert call(fn) == INVALID and b"no disturbance installed" in lib.nig_last_error() and untouched()
    # the undisturbed entry points do not need one, and ignore an installed one
    ref = ni.make_batched("ChemicalReactor-v0", 256, max_episode_steps=MAXS, seed=SEED)
    ref.reset()
    ref.set_policy(ni.mpc_agent(S, A))
    a_ref = torch.zeros(2, A, 256, device=dev)
    ref.rollout_policy(2, act_out=a_ref)
    env.set_disturbance(good)
    a_env = torch.zeros(2, A, 256, device=dev)
    env.rollout_policy(2, act_out=a_env)
    torch.cuda.synchronize()
    assert torch.equal(a_env, a_ref)
    # a refused set keeps the installed disturbance: the next call runs with `good`
    assert lib.nig_set_disturbance(env._h, C.byref(bad[0]), st) == INVALID
    env.rollout_policy_disturbed(2, rw, fl, obs, act, seen)
    torch.cuda.synchronize()
    assert not torch.equal(seen, obs) and bool((seen != FILL).all())
    env.close()
    ref.close()
    # an env shape the MFMA actor refuses (odd state dim): UNSUPPORTED, whatever is installed
    odd = ni.make_batched("WaterTreatment-v0", 64, seed=SEED)
    odd.reset()
    odd.set_disturbance(ni.Disturbance(obs_noise=0.1))
    assert lib.nig_rollout_mlp_disturbed(odd._h, 1, None, None, 0, None, 0, None, 0, 0, None, 0, odd._stream()) == UNSUPPORTED
    odd.close()


# ---- 7. evaluate_robustness -------------------------------------------------------------------------------------------------
class _NotFusable:
    """an actor evaluate_with_safety cannot put into the env kernel: the host loop with the wrapper's own draws"""
    is_trained = True

    def __init__(self, pol):
        self.pol, self.state_dim, self.action_dim = pol, pol.state_dim, pol.action_dim

    def predict_device(self, obs):
        return self.pol.predict_device(obs)

    def predict(self, observations, deterministic=True):
        return self.pol.predict(observations)


@pytest.mark.parametrize("which", ["mpc", "actor"])
def test_evaluate_robustness(ni, which):
    name, N, CAP = "ChemicalReactor-v0", 4 * 1024, 50
    levels = (0.0, 0.1, 0.2, 0.3)
    kinds = ("observation_noise", "action_noise", "dynamics_noise")
    template = ni.make_batched(name, 1024, max_episode_steps=CAP, tally=True, autoreset=False, seed=SEED)
    agent = ni.mpc_agent(template.state_dim, template.action_dim) if which == "mpc" \
        else ni.MLPPolicy(_members(ni, name, 1, 500)[0], device=template.device)
    r = ni.evaluate_robustness(agent, template, n_episodes=N)
    assert r["path"] == ("fused-policy" if which == "mpc" else "fused-mlp")
    assert r["noise_levels"] == list(levels) and r["disturbance_types"] == list(kinds)
    assert set(r) == {"robustness_results", "robustness_scores", "overall_robustness", "noise_levels", "disturbance_types", "path"}
    res = r["robustness_results"]
    fresh = ni.make_batched(name, 1024, max_episode_steps=CAP, tally=True, autoreset=False, seed=SEED)
    m = ni.evaluate_with_safety(agent, fresh, n_episodes=N // len(levels))
    viol_lanes = int((fresh.violation_count > 0).sum().item())
    fresh.close()
    for kind in kinds:
        c = res[kind][0.0]
        assert set(c) == {"mean_return", "std_return", "safety_violations", "violation_rate"}
        assert c["mean_return"] == float(m["return_mean"]) and c["std_return"] == float(m["return_std"]), kind
        assert c["safety_violations"] == int(m["safety_violations"]) and c["violation_rate"] == viol_lanes / 1024, kind
    scores, overall = ni.robustness_scores(res, list(levels), list(kinds))
    assert r["robustness_scores"] == scores and r["overall_robustness"] == overall
    # (observation noise need not move a saturated proportional law; tests 2 and 3 above show that it reaches the policy)
    assert all(res["action_noise"][lv]["mean_return"] != res["action_noise"][0.0]["mean_return"] for lv in levels[1:]), "the noise must act"
    assert all(res["dynamics_noise"][lv] == res["dynamics_noise"][0.0] for lv in levels)
    if which == "actor":
        # hold="step": the fused cells against the host loop (torch draws), 4 combined standard errors of the two means
        n = N // len(levels)
        f = ni.evaluate_robustness(agent, template, n_episodes=N, hold="step")
        h = ni.evaluate_robustness(_NotFusable(agent), template, n_episodes=N, hold="step")
        assert f["path"] == "fused-mlp" and h["path"] == "host"
        for kind in kinds:
            for lv in levels:
                a, b = f["robustness_results"][kind][lv], h["robustness_results"][kind][lv]
                se = np.sqrt(a["std_return"] ** 2 / n + b["std_return"] ** 2 / n)
                z = abs(a["mean_return"] - b["mean_return"]) / max(se, 1e-300)
                print(f"{kind} {lv}: fused {a['mean_return']:.4f} host {b['mean_return']:.4f} |diff| / se = {z:.2f}")
                assert abs(a["mean_return"] - b["mean_return"]) <= 4 * se, (kind, lv)
    template.close()
