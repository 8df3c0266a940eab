"""What a handle carries from one call to the next, stated once for tests/test_gpu_handle_lifecycle.py (gpu) and
tests/test_handle_lifecycle_host.py (not gpu).  A plain helper module (no fixtures, no collection hooks): env lists, weights, start
states and shapes are tests/closed_loop_matrix.py's.

CASES names every closed-loop case: an entry point of the C ABI that advances the env inside a kernel, with the inputs it needs
(rollout_policy twice: an affine law and PID; rollout_mlp_ensemble twice: "mean" and "voting"), on the envs it is compiled for.  The
reference of every comparison is a LEAN TWIN: a second handle of the same env, batch, seed and env_index0 that has only ever seen
the one install and the one call under test -- the run the family modules already hold to the oracle.  Outputs and everything the
handle keeps are compared as bit patterns."""
import numpy as np

import closed_loop_matrix as M

SEED, T, MAXS = 0x5EED, M.T_NEW, M.MAXS_NEW
F_CAN, I_CAN, H_CAN = -7.25, 0x5A5A5A5B, 0x7A7B        # canaries: float32 rows, int32 rows, the bf16 actor's int16 hidden rows
N_CAND, PROJ_ITERS, PROJ_STEP = 3, 3, 0.5
ENS_K, GATE_K, GATE_C, PROJ_C = 3, 2, 2, 2

ALL = [k for k, _ in M.POLICY_ENVS_ALL]
MFMA = [k for k, _ in M.MFMA_ENVS]
LIM_ALL = [k for k in ALL if k not in M.CLONED]          # the Advanced pair takes no added constraints (nig_set_limits refuses)
LIM_MFMA = [k for k in MFMA if k not in M.CLONED]
NOISE = ["cr", "pg", "ra"]                               # nig_rollout_noise: the envs the reference can record draws for
ACT64 = ("cr", "pg", "ra")                               # the envs whose step follows a float64 action's type (no narrowed copy)

# case -> (C symbol, env keys, lanes per block of its kernel, the inputs it needs)
CASES = {
    "sampled": ("nig_rollout_sampled", ALL, 256, ()),
    "noise": ("nig_rollout_noise", NOISE, 256, ()),
    "policy_affine": ("nig_rollout_policy", ALL, 256, ("affine",)),
    "policy_pid": ("nig_rollout_policy", ALL, 256, ("pid",)),
    "policy_disturbed": ("nig_rollout_policy_disturbed", ALL, 256, ("affine", "disturbance")),
    "mlp": ("nig_rollout_mlp", MFMA, 128, ("actor",)),
    "mlp_bf16": ("nig_rollout_mlp_bf16", MFMA, 128, ("bf16",)),
    "safe": ("nig_rollout_mlp_safe", MFMA, 128, ("actor", "critic")),
    "search": ("nig_rollout_mlp_search", MFMA, 128, ("actor", "critic")),
    "ens_mean": ("nig_rollout_mlp_ensemble", MFMA, 128, ("ens_mean",)),
    "ens_voting": ("nig_rollout_mlp_ensemble", MFMA, 128, ("ens_voting",)),
    "gated": ("nig_rollout_mlp_gated", MFMA, 128, ("actor", "gate")),
    "projected": ("nig_rollout_mlp_projected", MFMA, 128, ("actor", "predictor")),
    "disturbed": ("nig_rollout_mlp_disturbed", MFMA, 128, ("actor", "disturbance")),
}
# the _limited twins: twin case -> its parent.  A twin has its parent's inputs and block, the symbol <parent's>_limited, and runs on
# the parent's envs that accept limits.  (sampled, noise, the PID law and the bf16 actor have no twin.)
LIMITED = {
    "policy_limited": "policy_affine",
    "policy_disturbed_limited": "policy_disturbed",
    "mlp_limited": "mlp",
    "safe_limited": "safe",
    "search_limited": "search",
    "ens_mean_limited": "ens_mean",
    "ens_voting_limited": "ens_voting",
    "gated_limited": "gated",
    "projected_limited": "projected",
    "disturbed_limited": "disturbed",
}
PARENTS = list(CASES)
TWINS = list(LIMITED)
for _twin, _parent in LIMITED.items():
    _sym, _keys, _block, _inputs = CASES[_parent]
    CASES[_twin] = (_sym + "_limited", LIM_ALL if _block == 256 else LIM_MFMA, _block, _inputs)
CELLS = [(c, k) for c in CASES for k in CASES[c][1]]
# the entry points of the ABI that advance the env inside a kernel and are NOT in the table, with the reason
NOT_A_CASE = {
    "nig_rollout": "the open loop on a caller's ring: test_gpu_abi_round2.py::test_rollout_freezes_done_lanes_of_an_autoreset_handle",
    "nig_rollout_mixed": "several handles in one launch (MixedBatchedEnv): no handle state of its own",
    "nig_rollout_mixed_obs": "several handles in one launch (MixedBatchedEnv): no handle state of its own",
}
# the translation units that instantiate each symbol's launcher (csrc/<prefix><key>.hip), and whether it needs the MFMA actor
UNITS = {
    "nig_rollout_sampled": ("sampled_", False), "nig_rollout_noise": ("env_", False), "nig_rollout_policy": ("env_", False),
    "nig_rollout_policy_disturbed": ("disturbed_", False), "nig_rollout_mlp": ("env_", True), "nig_rollout_mlp_bf16": ("bf16_", True),
    "nig_rollout_mlp_safe": ("env_", True), "nig_rollout_mlp_search": ("search_", True), "nig_rollout_mlp_ensemble": ("ensemble_", True),
    "nig_rollout_mlp_gated": ("gated_", True), "nig_rollout_mlp_projected": ("projected_", True),
    "nig_rollout_mlp_disturbed": ("disturbed_", True),
    "nig_rollout_policy_limited": ("limited_", False), "nig_rollout_mlp_limited": ("limited_", True),
    "nig_rollout_mlp_safe_limited": ("limited_shield_", True), "nig_rollout_mlp_search_limited": ("limited_search_", True),
    "nig_rollout_mlp_ensemble_limited": ("limited_ensemble_", True), "nig_rollout_mlp_gated_limited": ("limited_gated_", True),
    "nig_rollout_mlp_projected_limited": ("limited_projected_", True),
    "nig_rollout_policy_disturbed_limited": ("limited_disturbed_", False), "nig_rollout_mlp_disturbed_limited": ("limited_disturbed_", True),
}


def parent_of(case):
    return LIMITED.get(case, case)


def held_lanes(B, block):
    """The lanes a part-1 case holds.  B = 700: every third lane of the first wave (held and live mixed in one wave), one whole
    wave, one whole block of the kernel (128 lanes for the MFMA kernels, 256 for the policy kernels) and the last lane of the
    partial block.  B = 5: lanes 1 and 4."""
    if B == M.B_SMALL:
        return np.array([1, 4])
    assert B == M.B_BIG and block in (128, 256)
    whole_block = range(256, 256 + block)                # MFMA: block 2; policy kernels: block 1
    return np.array(sorted(set(range(0, 64, 3)) | set(range(64, 128)) | set(whole_block) | {B - 1}))


def held_mask(B, block):
    m = np.zeros(B, dtype=bool)
    m[held_lanes(B, block)] = True
    return m


# ---- the inputs, each in variants that differ in every array and every scalar ------------------------------------------------------
def actor(ni, key, S, A, seed):
    """test_gpu_limits_families.py's actor: ChemicalReactor's first layer scaled per state column, M.matrix_actor for the rest."""
    ws = M.random_actor(S, A, seed)
    if key == "cr":
        sc = M.state_scale(ni, key, SEED)
        ws = [((ws[0][0] * np.float32(20.0) * sc[:, None]).astype(np.float32), ws[0][1]), ws[1], ws[2]]
    return M.matrix_actor(ni, key, ws, SEED)


def critic(ni, key, S, A, seed, n_out=1):
    """test_gpu_limits_families.py's critic: M.random_critic with its state rows scaled by M.state_scale, so that p spreads."""
    cw, sc = M.random_critic(S, A, seed, n_out), M.state_scale(ni, key, SEED)
    return [(np.concatenate([cw[0][0][:S] * sc[:, None], cw[0][0][S:]]).astype(np.float32), cw[0][1]), cw[1], cw[2]]


THR = [0.5, 0.45, 0.55, 0.4]


def set_affine(ni, env, key, v=0):
    from neorl_industrial_gym_amd.policies import DevicePolicy
    S, A = env.state_dim, env.action_dim
    rng, sc = np.random.default_rng(300 + v), M.state_scale(ni, key, SEED)
    env.set_policy(DevicePolicy(S, A, W=rng.normal(0, 1.0, (A, S)) * sc[None, :], b=rng.normal(0, 0.3, A), sigma=np.full(A, 0.05 + 0.02 * v),
                                half_range=np.full(A, 0.03 + 0.01 * v), p_uniform=0.1 + 0.05 * v, uniform_range=1.0 - 0.1 * v,
                                clip=(-1.0 + 0.05 * v, 1.0 - 0.1 * v)))


def set_pid(ni, env, key, v=0):
    A = env.action_dim
    env.set_policy(ni.pid_agent(env.state_dim, A, kp=1.0 - 0.3 * v, ki=0.1 + 0.05 * v, kd=0.01 + 0.02 * v,
                                setpoint=np.random.default_rng(310 + v).normal(0, 0.5, A)))


def set_actor(ni, env, key, v=0):
    env.set_mlp_policy(actor(ni, key, env.state_dim, env.action_dim, 5 + 1000 * v))


def set_bf16(ni, env, key, v=0):
    env.set_mlp_policy_bf16(actor(ni, key, env.state_dim, env.action_dim, 21 + 1000 * v))


def set_critic(ni, env, key, v=0):
    env.set_mlp_safety(critic(ni, key, env.state_dim, env.action_dim, 6 + 1000 * v), THR[v % 4])


def ensemble_weights(v, K):
    """The agent's weight vector of ensemble variant v (method "mean" divides it by its sum)."""
    return list(np.random.default_rng(320 + v).uniform(0.3, 2.0, K))


def set_ensemble(ni, env, key, method, v=0, K=ENS_K):
    from neorl_industrial_gym_amd.policies import ensemble_active_weights
    members = [actor(ni, key, env.state_dim, env.action_dim, 200 + 7 * k + 1000 * v) for k in range(K)]
    if method == "voting":
        env.set_mlp_ensemble(members, None, None, "voting", 0.2 + 0.05 * v)
    else:
        aw, wsum = ensemble_active_weights(ensemble_weights(v, K), K, "mean")
        env.set_mlp_ensemble(members, aw, wsum, "mean", 0.2 + 0.05 * v)


def set_gate(ni, env, key, v=0, K=GATE_K, C=GATE_C):
    S, A = env.state_dim, env.action_dim
    env.set_mlp_safety_ensemble([critic(ni, key, S, A, 8 + m + 1000 * v, n_out=C) for m in range(K)], 1.0 + 0.5 * v, 0.6 - 0.05 * v, 0.2 + 0.03 * v)


def set_predictor(ni, env, key, v=0, C=PROJ_C):
    env.set_mlp_constraint(critic(ni, key, env.state_dim, env.action_dim, 10 + 1000 * v, n_out=C), THR[v % 4], -0.2 + 0.1 * v)


def set_disturbance(ni, env, key, v=0):
    env.set_disturbance(ni.Disturbance(obs_noise=0.1, action_noise=0.1, hold="step") if v % 2 == 0 else
                        ni.Disturbance(obs_noise=0.05, action_noise=0.2, clip=(-0.8, 0.9), hold="episode"))


SETTERS = {"affine": set_affine, "pid": set_pid, "actor": set_actor, "bf16": set_bf16, "critic": set_critic,
           "ens_mean": lambda ni, env, key, v=0, **kw: set_ensemble(ni, env, key, "mean", v, **kw),
           "ens_voting": lambda ni, env, key, v=0, **kw: set_ensemble(ni, env, key, "voting", v, **kw),
           "gate": set_gate, "predictor": set_predictor, "disturbance": set_disturbance}


def install(ni, env, case, key, variants=None):
    """The inputs `case` needs, each in variant variants.get(input, 0)."""
    for inp in CASES[case][3]:
        SETTERS[inp](ni, env, key, (variants or {}).get(inp, 0))


def band(ni, env):
    """One box constraint: a band of a sixth of action row 0's range that leaves out the zero action a gate substitutes and
    most of what a shield halves (and state row 0, unbounded), critical: it fires on most steps of every family on every env,
    changes the reward and ends episodes."""
    return ni.BoxConstraint("band", {("action", 0): (0.011, 0.35), ("state", 0): (-np.inf, np.inf)}, -2.5, critical=True)


def floor(ni, row, lo):
    """One box constraint, critical: state row `row` not below `lo` (action row 0 listed, unbounded).  The added constraints are
    checked on the state a step starts from, so with `lo` in the middle of the lanes' start values it fires on step 0 on
    exactly the lanes below it, whatever the family and the env."""
    return ni.BoxConstraint("floor", {("state", row): (lo, np.inf), ("action", 0): (-np.inf, np.inf)}, -2.5, critical=True)


SPREAD = (0.25, 0.5, 1.0, 1.5, 2.0)


def spread_start(env):
    """After a rewind: lane i's start state times SPREAD[i % 5], episode step 0, not done.  From their reset states most envs
    violate no built-in constraint within T steps; every built-in constraint is a box on state rows (PowerGrid's third: on
    state plus action), and a quarter or twice the reset state lies outside at least one of them on every env -- which the
    caller asserts on the lean twin's flag words."""
    s = env.get_state().cpu().numpy()
    f = np.array(SPREAD, dtype=np.float32)[np.arange(env.batch) % len(SPREAD)]
    env.set_state(np.ascontiguousarray(s * f[:, None]), current_step=0, violation_count=0, done=False)


def make(ni, key, B, tally=False, cons=(), env_index0=0):
    env = ni.make_batched(M.NAMES[key], B, seed=SEED, env_index0=env_index0, autoreset=True, tally=tally, max_episode_steps=MAXS)
    for c in cons:
        env.add_safety_constraint(c)
    return env


def rewind(ni, env, key, t0=0, done=None, case=None, variants=None):
    """A used handle and its twin at the same point: the launch counter, a full reset (the draws are keyed by global lane and launch
    counter), the distinct start states of the two CLONED envs; `done` [B] bool marks lanes held through set_state.  A PID law's
    memory is the agent's and survives a reset (baseline_agents.py:55-57): a PID case installs its law again, as its twin did."""
    env.counter = t0
    env.reset()
    if key in M.CLONED:
        env.set_state(np.array(M.start_states(ni, M.NAMES[key], env.batch, SEED)), current_step=0, violation_count=0,
                      done=False if done is None else done)
    elif done is not None:
        env.set_state(current_step=env.current_step, violation_count=env.violation_count, done=done)
    if case is not None and "pid" in CASES[case][3]:
        set_pid(ni, env, key, (variants or {}).get("pid", 0))


# ---- one launch with every output ------------------------------------------------------------------------------------------------
def run(env, case, n=T, t_ring=100):
    """One launch of n steps of `case` with every output it has, each filled with a canary first.  Returns name -> numpy array
    with the LANES ON THE LAST AXIS (obs / seen, row-major on the device, are transposed); pitched rows keep their pad columns.
    obs / seen need B * S to be a multiple of 4: absent otherwise.  The gate's and the projection's per-constraint rows are given
    four rows a step whatever the installed head's width, so that rows beyond n_outputs show a stray store."""
    import torch
    B, S, A, ld, dev = env.batch, env.state_dim, env.action_dim, env.ld, env.device
    f = lambda *shape: torch.full(shape, F_CAN, dtype=torch.float32, device=dev)
    i = lambda *shape: torch.full(shape, I_CAN, dtype=torch.int32, device=dev)
    rows_ok = (B * S) % 4 == 0
    out = dict(rew=f(n, ld), fl=i(n, ld))
    rew, fl = out["rew"], out["fl"]
    base = parent_of(case)
    xf = (i(n, ld),) if case.endswith("_limited") else ()
    if xf:
        out["xf"] = xf[0]
    if base == "sampled":
        out["obs_held"] = f(n, S, ld)           # (nig_rollout's law: a frozen lane's row is written, with the state it holds)
        env.rollout_sampled(n, rew, fl, out["obs_held"])
    elif base == "noise":
        ks, kr = int(env.spec.k_step), int(env.spec.k_reset)
        g = torch.Generator(device="cpu").manual_seed(77)
        ring = torch.empty(n, A, ld, dtype=torch.float32, device=dev)
        for k in range(n):
            env.fill_actions(t_ring + k, ring[k])
        k0 = t_ring - 100                       # (a cut launch goes on in the same recorded rows)
        assert 0 <= k0 and k0 + n <= T
        sn = (torch.randn(T, ks, ld, generator=g, dtype=torch.float64) * 0.5).to(dev)[k0:k0 + n] if ks else None
        rn = (torch.randn(T, kr, ld, generator=g, dtype=torch.float64) * 0.5).to(dev)[k0:k0 + n] if kr else None
        if sn is None and rn is None:
            rn = torch.zeros(n, 1, ld, dtype=torch.float64, device=dev)
        out["obs_held_rm"] = f(n, B, S)
        env.rollout_noise(n, ring, sn, rn, rew, fl, out["obs_held_rm"])
    else:
        obs = f(n, B, S) if rows_ok else None
        out["act"] = act = f(n, A, ld)
        if obs is not None:
            out["obs"] = obs
        lim = "_limited" if xf else ""
        if base in ("policy_affine", "policy_pid"):
            getattr(env, "rollout_policy" + lim)(n, rew, fl, obs, act, *xf)
        elif base in ("policy_disturbed", "disturbed"):
            seen = f(n, B, S) if rows_ok else None
            if seen is not None:
                out["seen"] = seen
            getattr(env, ("rollout_policy_disturbed" if base == "policy_disturbed" else "rollout_mlp_disturbed") + lim)(n, rew, fl, obs, act, seen, *xf)
        elif base == "mlp":
            getattr(env, "rollout_mlp" + lim)(n, rew, fl, obs, act, *xf)
        elif base == "mlp_bf16":
            out["hid"] = torch.full((n, 512, ld), H_CAN, dtype=torch.int16, device=dev)
            env.rollout_mlp_bf16(n, rew, fl, obs, act, out["hid"])
        elif base == "safe":
            out["prob"] = f(n, ld)
            getattr(env, "rollout_mlp_safe" + lim)(n, rew, fl, obs, act, out["prob"], *xf)
        elif base == "search":
            out.update(prob=f(n, ld), risk=f(n, ld), choice=i(n, ld))
            getattr(env, "rollout_mlp_search" + lim)(n, N_CAND, rew, fl, obs, act, out["prob"], out["risk"], out["choice"], *xf)
        elif base in ("ens_mean", "ens_voting"):
            out.update(unc=f(n, ld), member=f(n, env._ensemble_members, A, ld))
            getattr(env, "rollout_mlp_ensemble" + lim)(n, rew, fl, obs, act, out["unc"], out["member"], *xf)
        elif base == "gated":
            K, Cn = env._gate_shape
            out.update(prob=f(n, 4, ld), unc=f(n, 4, ld), logit=f(n, K, 4, ld))
            getattr(env, "rollout_mlp_gated" + lim)(n, rew, fl, obs, act, out["prob"][:, :Cn], out["unc"][:, :Cn], out["logit"][:, :, :Cn], *xf)
        elif base == "projected":
            Cn = env._constraint_outputs
            out.update(prob=f(n, 4, ld), viol=f(n, 4, ld), iters=i(n, ld), grad=f(n, A, ld))
            getattr(env, "rollout_mlp_projected" + lim)(n, PROJ_ITERS, PROJ_STEP, rew, fl, obs, act, out["prob"][:, :Cn], out["viol"][:, :Cn],
                                                         out["iters"], out["grad"], *xf)
        else:
            raise KeyError(case)
    torch.cuda.synchronize()
    res = {}
    for name, t in out.items():
        a = t.cpu().numpy()
        res[name] = np.ascontiguousarray(a.transpose(0, 2, 1)) if name in ("obs", "seen", "obs_held_rm") else a
    return res


def run_cut(env, case, cuts):
    """The launches of sum(cuts) steps cut into pieces, their rows put together again."""
    parts, t_ring = [], 100
    for n in cuts:
        parts.append(run(env, case, n, t_ring))
        t_ring += n
    return {k: np.concatenate([p[k] for p in parts], axis=0) for k in parts[0]}


def kept(env):
    """Everything the handle keeps, as numpy arrays with the lanes on the last axis."""
    import torch
    torch.cuda.synchronize()
    d = dict(state=env.state_soa.cpu().numpy(), ctr=env.ctr.cpu().numpy(), life=env.life_viol.cpu().numpy())
    if env.tally is not None:
        d.update(ep_ret=env.ep_return.cpu().numpy(), tally=env.tally.cpu().numpy())
    d["counter"] = env.counter
    return d


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def canary_of(a):
    return bits(np.array([H_CAN if a.dtype == np.int16 else (I_CAN if a.dtype == np.int32 else F_CAN)], dtype=a.dtype))[0]


def same(got, want, lanes=None, what=""):
    """Bit equality of two output dicts (or kept() dicts) on `lanes` (a bool mask over the batch; None: every column, pads included)."""
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for k in got:
        if k == "counter":
            assert got[k] == want[k], (what, k, got[k], want[k])
            continue
        g, w = bits(got[k]), bits(want[k])
        if lanes is not None:
            g, w = g[..., :len(lanes)][..., lanes], w[..., :len(lanes)][..., lanes]
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            raise AssertionError(f"{what}: {k} differs in {len(bad)} words, first {bad[:3].tolist()}")


def pads_clean(out, B, what=""):
    for k, a in out.items():
        assert (bits(a[..., B:]) == canary_of(a)).all(), (what, k, "pad columns")
