"""-m gpu: box constraints added by the user, on the device ("nig-limits-v1", include/nig.h nig_set_limits).
  1. the reference: nig_step_limited / nig_step64_limited on the recorded tuples of the reference env with four added
     SafetyConstraints (tests/golden/limits_<key>.npz), and its evaluate_with_safety dict through the batched evaluation;
  2. inert limits (infinite bounds) are off: step and both closed loops equal their parents bit for bit;
  3. the limited closed loops are the limited step kernel fed with their own actions;
  4. the law from the parents' pieces: a limited rollout's every step replayed through parent handles with no built-in
     constraint (raw reward, own termination, next state) and with all (built-in bits), the added bits and the reward order
     restated in NumPy;
  5. twins: added boxes that restate ChemicalReactor's built-ins give the built-ins' bits;
  6. refusals and the memory footprint of the four new entry points.
Shapes are the closed-loop matrix's (tests/closed_loop_matrix.py): B = 700 and 5, T = 7, episodes of at most 5 steps."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import closed_loop_matrix as M
import limits_fixture as F
from conftest import ENV_NAME, KEYS, RTOL, StubAgent, rel_err, result_of
from footprint import Arena, Layout

pytestmark = pytest.mark.gpu

LIMIT_ENVS = [(k, n) for k, n in M.POLICY_ENVS_ALL if k not in M.CLONED]              # seven: all but the Advanced pair
LIMIT_MFMA = [(k, n) for k, n in M.MFMA_ENVS if k not in M.CLONED]                    # six: those with the MFMA actor
CASES = [("policy", k) for k, _ in LIMIT_ENVS] + [("mlp", k) for k, _ in LIMIT_MFMA]
T, MAXS, SEED = M.T_NEW, M.MAXS_NEW, 0x5EED
REWARD_F32 = lambda key: key not in ("pg", "ra")       # Env::reward_t: double for PowerGrid and RobotAssembly, float elsewhere
INT_ROWS = ("T_EPISODES", "T_LEN_SUM", "T_LEN_SQ", "T_VIOL", "T_CRIT", "T_SHUTDOWN", "T_SUCCESS", "T_SATISFIED", "T_CONSTRAINTS")
FLOAT_ROWS = ("T_RET_SUM", "T_RET_SQ", "T_RET_MIN", "T_RET_MAX")


@pytest.fixture(scope="module")
def ni():
    import neorl_industrial_gym_amd as ni
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return ni


def _code(ni, call):
    try:
        call()
    except ni._lib.NigError as e:
        return int(re.match(r"libnig error (\d+)", str(e)).group(1))
    return 0


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


# ---- 1. the reference --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("prefix", ["s1_", "s2_", "s1_a64_", "s2_a64_"])
def test_step_limited_vs_the_reference(ni, key, prefix):
    """Every recorded tuple in its own lane, the reference's draws injected.  Counts, per-constraint bits, terminated and
    truncated exact -- the corner tuples (a built-in critical violation with an added violation, an added critical one alone)
    included; state and reward by the existing parity rule, float32 and float64 actions alike (test_gpu_parity.py's single-step
    and float64-action tests): state words bit-exact but ChemicalReactor's concentration column (np.exp differs by an ulp) and at
    most 8 words of RobotAssembly's velocity columns; float outputs within 1e-5, and within test_gpu_parity.py's tighter
    float64-action bars (state 2e-7, reward 2e-7 for PowerGrid and 1e-9 otherwise) on the float64 tuples."""
    d = F.load(key)
    t = F.tuples(d, prefix)
    n, (S, A) = len(t["reward"]), (t["state_pre"].shape[1], t["action"].shape[1])
    env = ni.make_batched(ENV_NAME[key], n, autoreset=False)
    for c in F.boxes(ni, d, int(prefix[1]), S, A):
        env.add_safety_constraint(c)
    assert len(env.safety_constraints) == 7 and env.has_limits
    env.set_state(t["state_pre"], current_step=t["step_pre"], violation_count=t["viol_pre"])
    act = t["action64"] if "action64" in t else t["action"]
    obs, rew, term, trunc, info = env.step(act, step_noise=t["noise"].T if t["noise"].shape[1] else None, layout="aos")
    torch.cuda.synchronize()
    assert np.array_equal(term.cpu().numpy(), t["terminated"] != 0) and np.array_equal(trunc.cpu().numpy(), t["truncated"] != 0)
    assert np.array_equal(info.violation_count.cpu().numpy(), t["viol"])
    assert np.array_equal(info.critical_violations.cpu().numpy(), t["crit"])
    assert np.array_equal(info.constraint_violated.cpu().numpy().T.astype(np.uint8), t["viol_bits"])
    assert np.array_equal(info.critical_shutdown.cpu().numpy(), t["crit"] > 0)
    assert np.array_equal(info.step.cpu().numpy(), t["step_pre"] + 1)
    assert np.array_equal(env.violation_count.cpu().numpy(), t["violations_after"])
    sm = info.safety_metrics(0)
    assert (sm.total_constraints, sm.violation_count, sm.critical_violations) == (7, int(t["viol"][0]), int(t["crit"][0]))
    gm = env.get_safety_metrics().cpu().numpy()
    assert np.array_equal(gm[1], np.full(n, 7)) and np.array_equal(gm[2], t["viol"]) and np.array_equal(gm[3], t["crit"])
    sn, gn = env.get_state().cpu().numpy(), t["state_next"]
    same = (_bits(sn) == _bits(gn)) | (np.isnan(sn) & np.isnan(gn))
    cols = set(np.unique(np.where(~same)[1]).tolist())
    print(f"{key} {prefix}: state rel err {rel_err(sn, gn).max():.3g}, reward rel err {rel_err(env.reward64.cpu().numpy(), t['reward']).max():.3g}, "
          f"differing state words {int((~same).sum())}")
    assert cols <= ({4} if key == "cr" else ({14, 15, 16} if key == "ra" else set())), cols
    assert (~same).sum() <= (1 << 30 if key == "cr" else 8)
    assert rel_err(sn, gn).max() <= RTOL
    r64 = env.reward64.cpu().numpy()
    assert rel_err(r64, t["reward"]).max() <= RTOL and rel_err(rew.cpu().numpy(), t["reward"]).max() <= RTOL
    if "a64" in prefix:
        assert rel_err(sn, gn).max() <= 2e-7 and rel_err(r64, t["reward"]).max() <= (2e-7 if key == "pg" else 1e-9)
    elif key == "cr":                                   # float32 rewards: bit-exact wherever the next state is
        exact = same.all(axis=1)
        assert exact.sum() > n // 2 and np.array_equal(r64[exact], t["reward"][exact])
    env.close()


@pytest.mark.parametrize("key", KEYS)
def test_evaluate_with_safety_under_added_constraints_vs_the_reference_dict(ni, key):
    """The reference's evaluate_with_safety dict for the stub agent on an env with constraint set 2 added (two of them
    critical), reproduced by the batched evaluation with the recorded draws: the host loop on nig_step_limited."""
    d = F.load(key)
    g = {k[5:]: v for k, v in d.items() if k.startswith("eval_")}
    want = result_of(g)
    off, E, K = g["ep_offsets"], len(g["ep_length"]), g["noise"].shape[1]
    env = ni.make_batched(ENV_NAME[key], E, autoreset=False, tally=True)
    for c in F.boxes(ni, d, 2, env.state_dim, env.action_dim):
        env.add_safety_constraint(c)

    def step_noise(rnd, t):
        if not K:
            return None
        nz = np.zeros((E, K))
        live = np.where(g["ep_length"] > t)[0]
        nz[live] = g["noise"][off[live] + t]
        return nz.T

    got = ni.evaluate_with_safety(StubAgent(g), env, n_episodes=E, step_noise_fn=step_noise, reset_noise_fn=lambda rnd: g["ep_init_noise"].T)
    assert set(got) == set(want)
    for k in ("safety_violations", "critical_violations", "emergency_shutdowns", "successful_episodes"):
        assert got[k] == want[k], k
    for k in ("return_mean", "return_std", "return_min", "return_max", "length_mean", "length_std",
              "safety_violations_per_episode", "constraint_satisfaction_rate", "success_rate"):
        assert got[k] == pytest.approx(want[k], rel=RTOL, abs=1e-9), k
    assert np.array_equal(env.total_violations.cpu().numpy(), g["ep_viol"])
    env.close()


# ---- helpers of 2-5 ----------------------------------------------------------------------------------------------------------
def _make(ni, key, B, autoreset=True, cons=()):
    env = ni.make_batched(M.NAMES[key], B, seed=SEED, autoreset=autoreset, tally=True, max_episode_steps=MAXS)
    for c in cons:
        env.add_safety_constraint(c)
    return env


def _agent(ni, env, kind, key):
    if kind == "policy":
        env.set_policy(ni.random_agent(env.state_dim, env.action_dim))
    else:
        ws = M.random_actor(env.state_dim, env.action_dim, 5)
        if key == "cr":     # state columns of 3e2 .. 2.5e5 drive every tanh head to +-1 (one action row for all lanes: no quantile
            # separates it): the first layer scaled per state column, M.matrix_actor's construction for its large-state envs
            sc = M.state_scale(ni, key, SEED)
            ws = [((ws[0][0] * np.float32(20.0) * sc[:, None]).astype(np.float32), ws[0][1]), ws[1], ws[2]]
        env.set_mlp_policy(M.matrix_actor(ni, key, ws, SEED))


def _rollout(env, kind, limited, n=T):
    """One closed-loop launch of n steps with every output; numpy arrays over the batch's lanes.  (obs_out's step stride is a
    multiple of 4 floats: at B = 5 an env whose B * S is none runs without it, out["obs"] is None.)"""
    B, S, A, ld, dev = env.batch, env.state_dim, env.action_dim, env.ld, env.device
    rew = torch.zeros(n, ld, dtype=torch.float32, device=dev)
    fl = torch.zeros(n, ld, dtype=torch.int32, device=dev)
    xf = torch.full((n, ld), -1, dtype=torch.int32, device=dev)
    obs = torch.zeros(n, B, S, dtype=torch.float32, device=dev) if (B * S) % 4 == 0 else None
    act = torch.zeros(n, A, ld, dtype=torch.float32, device=dev)
    if limited:
        (env.rollout_policy_limited if kind == "policy" else env.rollout_mlp_limited)(n, rew, fl, obs, act, xf)
    else:
        (env.rollout_policy if kind == "policy" else env.rollout_mlp)(n, rew, fl, obs, act)
    torch.cuda.synchronize()
    assert bool((xf[:, B:] == -1).all()), "xflags pad columns"
    return dict(rew=rew[:, :B].cpu().numpy(), fl=fl[:, :B].cpu().numpy(), xf=xf[:, :B].cpu().numpy(), obs=None if obs is None else obs.cpu().numpy(),
                act=act[:, :, :B].cpu().numpy(), act_dev=act)


def _handle(env):
    torch.cuda.synchronize()
    return dict(state=env.get_state().cpu().numpy(), ctr=env.ctr.cpu().numpy(), life=env.life_viol.cpu().numpy(),
                ep_ret=env.ep_return.cpu().numpy(), tally=env.tally.cpu().numpy(), counter=env.counter)


def _inert(ni, S, A):
    inf = np.inf
    return [ni.BoxConstraint("inert_0", {("state", 0): (-inf, inf)}, -11.0, critical=True),
            ni.BoxConstraint("inert_1", {("action", 0): (-inf, inf), ("state", S - 1): (-inf, inf)}, -2.0),
            ni.BoxConstraint("inert_2", {("state", r): (-inf, inf) for r in range(S)}, -3.5, critical=True),
            ni.BoxConstraint("inert_3", {("action", j): (-inf, inf) for j in range(A)}, -0.25)]


def _quantile_boxes(ni, obs, act, critical=True):
    """Four boxes whose bounds are quantiles of a PARENT rollout's rows (obs [N, S], act [N, A]): a state row with an upper
    bound, an action band, a multi-row box, and an action band that is critical.  The state rows are the two with the most
    distinct values."""
    S, A = obs.shape[1], act.shape[1]
    order = np.argsort([-len(np.unique(obs[:, r])) for r in range(S)], kind="stable")
    ra, rb = int(order[0]), int(order[1])
    q = lambda x, p: np.float32(np.quantile(x.astype(np.float64), p))
    return [ni.BoxConstraint("upper", {("state", ra): (-np.inf, q(obs[:, ra], 0.65))}, -7.5),
            ni.BoxConstraint("band", {("action", 0): (q(act[:, 0], 0.2), q(act[:, 0], 0.8))}, -3.0),
            ni.BoxConstraint("box", {("state", rb): (q(obs[:, rb], 0.15), q(obs[:, rb], 0.85)),
                                     ("action", 1): (q(act[:, 1], 0.15), q(act[:, 1], 0.85))}, -12.25),
            ni.BoxConstraint("trip", {("action", A - 1): (q(act[:, A - 1], 0.15), q(act[:, A - 1], 0.85))}, -60.0, critical=critical)]


_PARENT = {}


def _parent_rollout(ni, kind, key, B):
    """The parent closed loop on a fresh same-seed handle, computed once per case and left unchanged."""
    ck = (kind, key, B)
    if ck not in _PARENT:
        env = _make(ni, key, B)
        _agent(ni, env, kind, key)
        env.reset()
        out = _rollout(env, kind, False)
        out.pop("act_dev")
        out["handle"] = _handle(env)
        env.close()
        for v in out.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _PARENT[ck] = out
    return _PARENT[ck]


def _same_tally(L, got, want, what):
    for r in INT_ROWS:
        assert np.array_equal(got[getattr(L, r)], want[getattr(L, r)]), (what, r)
    for r in FLOAT_ROWS:
        assert rel_err(got[getattr(L, r)], want[getattr(L, r)], floor=1e-300).max() <= 1e-12, (what, r)


# ---- 2. inert limits are off -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [M.B_BIG, M.B_SMALL])
@pytest.mark.parametrize("kind,key", CASES)
def test_inert_limits_are_off_in_the_closed_loops(ni, kind, key, B):
    """Four constraints with infinite bounds (two of them critical): rewards, flags, obs / act rows, final state, counters,
    lifetime violations and tally bit-identical to the parent at the same launch; SATISFIED and CONSTRAINTS grow by 4 per
    step of a finished episode; xflags all zero."""
    L = ni._lib
    par = _parent_rollout(ni, kind, key, B)
    env = _make(ni, key, B)
    for c in _inert(ni, env.state_dim, env.action_dim):
        env.add_safety_constraint(c)
    _agent(ni, env, kind, key)
    env.reset()
    got = _rollout(env, kind, True)
    h, ph = _handle(env), par["handle"]
    for k in ("rew", "fl", "obs", "act"):
        assert (got[k] is None and par[k] is None) or np.array_equal(_bits(got[k]), _bits(par[k])), k
    assert not got["xf"].any()
    for k in ("state", "ctr", "life", "ep_ret"):
        assert np.array_equal(h[k].view(np.uint8), ph[k].view(np.uint8)), k
    assert h["counter"] == ph["counter"]
    for r in range(L.T_ROWS):
        extra = 4 * ph["tally"][L.T_LEN_SUM] if r in (L.T_SATISFIED, L.T_CONSTRAINTS) else 0
        assert np.array_equal(h["tally"][r], ph["tally"][r] + extra), r
    assert ph["tally"][L.T_EPISODES].sum() > 0
    env.close()


@pytest.mark.parametrize("B", [M.B_BIG, M.B_SMALL])
@pytest.mark.parametrize("key", [k for k, _ in LIMIT_ENVS])
def test_inert_limits_are_off_in_step(ni, key, B):
    """env.step with four inert constraints (nig_step_limited) against env.step without (nig_step) on a same-seed handle, T
    steps on the generator's uniform actions with auto-reset: every output and the handle, as above."""
    L = ni._lib
    a, b = _make(ni, key, B), _make(ni, key, B)
    for c in _inert(ni, b.state_dim, b.action_dim):
        b.add_safety_constraint(c)
    a.reset(); b.reset()
    for k in range(T):
        act = a.fill_actions(k + 1)[:, :B]
        a.step(act, layout="soa"); b.step(act, layout="soa")
        torch.cuda.synchronize()
        for x, y in ((a.reward, b.reward), (a.reward64, b.reward64), (a.flags, b.flags), (a.get_state(), b.get_state())):
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), k
        assert not bool(b.xflags.any())
    ha, hb = _handle(a), _handle(b)
    for k in ("ctr", "life", "ep_ret"):
        assert np.array_equal(ha[k].view(np.uint8), hb[k].view(np.uint8)), k
    for r in range(L.T_ROWS):
        extra = 4 * ha["tally"][L.T_LEN_SUM] if r in (L.T_SATISFIED, L.T_CONSTRAINTS) else 0
        assert np.array_equal(hb["tally"][r], ha["tally"][r] + extra), r
    assert ha["tally"][L.T_EPISODES].sum() > 0
    a.close(); b.close()


# ---- 3. the closed loops are the step kernel ---------------------------------------------------------------------------------
def _loop_is_step(ni, kind, key, B, cons):
    L = ni._lib
    a, b = _make(ni, key, B, cons=cons), _make(ni, key, B, cons=cons)
    _agent(ni, a, kind, key)
    a.reset(); b.reset()
    assert a.counter == b.counter                     # (reset draws with t and leaves it: both handles step with t + 1 next)
    out = _rollout(a, kind, bool(cons))
    for k in range(T):
        b.step(out["act_dev"][k, :, :B], layout="soa")
        torch.cuda.synchronize()
        assert np.array_equal(_bits(b.reward.cpu().numpy()), _bits(out["rew"][k])), (k, "reward")
        assert np.array_equal(b.flags.cpu().numpy(), out["fl"][k]), (k, "flags")
        if cons:
            assert np.array_equal(b.xflags.cpu().numpy(), out["xf"][k]), (k, "xflags")
        if k + 1 < T and out["obs"] is not None:
            assert np.array_equal(_bits(b.get_state().cpu().numpy()), _bits(out["obs"][k + 1])), (k, "state")
    ha, hb = _handle(a), _handle(b)
    for k in ("state", "ctr", "life", "ep_ret"):
        assert np.array_equal(ha[k].view(np.uint8), hb[k].view(np.uint8)), k
    assert ha["counter"] == hb["counter"] and ha["tally"][L.T_EPISODES].sum() > 0
    _same_tally(L, ha["tally"], hb["tally"], "tally")
    a.close(); b.close()
    return out


@pytest.mark.parametrize("B", [M.B_BIG, M.B_SMALL])
@pytest.mark.parametrize("kind,key", CASES)
def test_the_limited_closed_loop_is_the_limited_step_kernel(ni, kind, key, B):
    """First the parents' own identity with no limits installed (rollout_policy / rollout_mlp against nig_step fed with the
    rollout's act_out); then the same under four added constraints, one critical: rewards, flags, xflags, states, counters,
    lifetime violations bit-equal; tally integer rows exact, float rows within 1e-12 relative (a launch merges its episodes as
    one fp64 partial: a few fp64 roundings)."""
    _loop_is_step(ni, kind, key, B, ())
    par = _parent_rollout(ni, kind, key, M.B_BIG)
    S, A = par["obs"].shape[2], par["act"].shape[1]
    cons = _quantile_boxes(ni, par["obs"].reshape(-1, S), par["act"].transpose(0, 2, 1).reshape(-1, A))
    out = _loop_is_step(ni, kind, key, B, cons)
    if B == M.B_BIG:
        assert out["xf"].any() and ((out["xf"] >> 8) & 7).any()


# ---- 4. the law from the parent's pieces -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,key", CASES)
def test_the_law_from_the_parents_pieces(ni, kind, key):
    L = ni._lib
    B = M.B_BIG
    par = _parent_rollout(ni, kind, key, B)
    S, A = par["obs"].shape[2], par["act"].shape[1]
    cons = _quantile_boxes(ni, par["obs"].reshape(-1, S), par["act"].transpose(0, 2, 1).reshape(-1, A))
    env = _make(ni, key, B, cons=cons)
    _agent(ni, env, kind, key)
    env.reset()
    t0 = env.counter
    out = _rollout(env, kind, True)
    final = env.get_state().cpu().numpy()
    env.close()
    sp = ni._lib.env_spec(ni.batched.ENV_IDS[M.NAMES[key]])
    RT = np.float32 if REWARD_F32(key) else np.float64
    p0, p7 = _make(ni, key, B, autoreset=False), _make(ni, key, B, autoreset=False)
    p0.set_constraint_mask(0)
    fired = np.zeros(4)
    n_trip_resets = 0
    for k in range(T):
        fl, xf, obs, act = out["fl"][k], out["xf"][k], out["obs"][k], out["act"][k]
        assert not (fl & L.FLAG_INACTIVE).any()
        step_pre = ((fl.astype(np.uint32) >> L.FLAG_STEP_SHIFT).astype(np.int64) & 0xFFFF) - 1
        for p in (p0, p7):
            p.set_state(obs, current_step=step_pre, violation_count=0, done=False)
            p.counter = t0 + k
            p.step(act, layout="soa")
        torch.cuda.synchronize()
        raw, own_term = p0.reward64.cpu().numpy(), (p0.flags.cpu().numpy() & L.FLAG_TERMINATED) != 0
        nxt, f7 = p0.get_state().cpu().numpy(), p7.flags.cpu().numpy()
        assert not (p0.flags.cpu().numpy() & (7 << L.FLAG_VIOL_SHIFT)).any()
        # the added bits: the box law on the pre-state and the CLIPPED action
        clipped = np.clip(act.T, np.float32(-1), np.float32(1))
        xb = np.array([[0 if c.check_fn(s, a) else 1 for c in cons] for s, a in zip(obs, clipped)], dtype=np.int64)
        vb = np.stack([(f7 >> (L.FLAG_VIOL_SHIFT + j)) & 1 for j in range(3)], axis=1)
        want_r, crit = F.reward_law(raw, vb, list(sp.penalty), list(sp.critical), xb, [c.penalty for c in cons],
                                    [int(c.critical) for c in cons], RT)
        xcrit = (xb * np.array([int(c.critical) for c in cons])).sum(axis=1)
        want_xf = (xb * (1 << np.arange(4))).sum(axis=1) | (xb.sum(axis=1) << 4) | (xcrit << 8)
        assert np.array_equal(xf, want_xf), (k, "xflags")
        assert np.array_equal(_bits(out["rew"][k]), _bits(want_r.astype(np.float32))), (k, "reward")
        term = own_term | (crit > 0)
        trunc = (f7 & L.FLAG_TRUNCATED) != 0
        done = term | trunc
        builtin_fields = (7 << L.FLAG_VIOL_SHIFT) | (3 << L.FLAG_NVIOL_SHIFT) | (3 << L.FLAG_NCRIT_SHIFT)
        want_fl = (f7 & builtin_fields) | (term * L.FLAG_TERMINATED) | (trunc * L.FLAG_TRUNCATED) | ((crit > 0) * L.FLAG_SHUTDOWN) \
            | (done * L.FLAG_DID_RESET) | ((step_pre + 1) << L.FLAG_STEP_SHIFT)
        assert np.array_equal(fl.astype(np.int64) & 0xFFFFFFFF, want_fl.astype(np.int64) & 0xFFFFFFFF), (k, "flags")
        after = out["obs"][k + 1] if k + 1 < T else final
        assert np.array_equal(_bits(after[~done]), _bits(nxt[~done])), (k, "next state")
        trip = (xcrit > 0) & ~own_term & ~trunc & ((vb * np.array(list(sp.critical))).sum(axis=1) == 0)
        if trip.any():                                   # an added critical constraint alone ended these episodes: a fresh state
            n_trip_resets += int(trip.sum())
            assert ((fl[trip] & L.FLAG_DID_RESET) != 0).all() and ((fl[trip] & L.FLAG_TERMINATED) != 0).all()
            assert (_bits(after[trip]) != _bits(nxt[trip])).any(axis=1).all()
            if k + 1 < T:
                assert (((out["fl"][k + 1][trip].astype(np.uint32) >> L.FLAG_STEP_SHIFT) & 0xFFFF) == 1).all()
        fired += xb.sum(axis=0)
    p0.close(); p7.close()
    rate = fired / (T * B)
    print(f"{kind} {key}: added constraints fired on {np.round(rate, 3)} of the live lane-steps; {n_trip_resets} episodes ended by the added critical one alone")
    assert ((rate >= 0.1) & (rate <= 0.9)).all(), rate
    assert n_trip_resets > 0
    # without auto-reset the lane an added critical constraint stopped is frozen: INACTIVE, reward 0, xflags 0, rows untouched
    env = _make(ni, key, B, autoreset=False, cons=cons)
    _agent(ni, env, kind, key)
    env.reset()
    o2 = _rollout(env, kind, True)
    ended = ((o2["xf"][0] >> 8) & 7) > 0
    assert ended.any() and ((o2["fl"][0][ended] & L.FLAG_TERMINATED) != 0).all() and ((o2["fl"][0][ended] & L.FLAG_DID_RESET) == 0).all()
    assert ((o2["fl"][1:, ended] & L.FLAG_INACTIVE) != 0).all() and not o2["xf"][1:, ended].any() and not o2["rew"][1:, ended].any()
    assert not o2["obs"][1:, ended].any() and not o2["act"][1:, :, ended].any()
    assert ((env.ctr.cpu().numpy()[ended] & L.CTR_DONE) != 0).all()
    env.close()


# ---- 5. twins ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["policy", "mlp", "step"])
def test_added_twins_of_the_builtins_give_the_builtins_bits(ni, kind):
    """ChemicalReactor: three added boxes that restate its built-ins (T <= 350, P <= 506625, 20 <= level <= 90) fire exactly
    where the VIOL bits do, on every step; some fire.  (States forced around the limits: uniform rollouts reach none.)"""
    L, key, B, inf = ni._lib, "cr", M.B_BIG, np.inf
    cons = [ni.BoxConstraint("t", {("state", 0): (-inf, 350.0)}, -1.0), ni.BoxConstraint("p", {("state", 1): (-inf, 506625.0)}, -1.0),
            ni.BoxConstraint("l", {("state", 10): (20.0, 90.0)}, -1.0)]
    env = _make(ni, key, B, cons=cons)
    env.reset()
    rng = np.random.default_rng(3)
    s = env.get_state().cpu().numpy()
    s[0::4, 0] = rng.uniform(345, 355, len(s[0::4])); s[1::4, 1] = rng.uniform(500000, 513000, len(s[1::4]))
    n2 = len(s[2::4])
    s[2::4, 10] = np.where(rng.random(n2) < 0.5, rng.uniform(15, 25, n2), rng.uniform(85, 95, n2))
    s[3, 0], s[7, 0], s[11, 1], s[15, 10], s[19, 10] = 350.0, np.nextafter(np.float32(350), np.float32(400)), 506625.0, 20.0, 90.0
    env.set_state(s, current_step=0, violation_count=0, done=False)
    if kind == "step":
        fls, xfs = [], []
        for k in range(T):
            env.step(env.fill_actions(k + 1)[:, :B], layout="soa")
            fls.append(env.flags.cpu().numpy().copy()); xfs.append(env.xflags.cpu().numpy().copy())
        fl, xf = np.stack(fls), np.stack(xfs)
    else:
        _agent(ni, env, kind, key)
        o = _rollout(env, kind, True)
        fl, xf = o["fl"], o["xf"]
    vb = (fl >> L.FLAG_VIOL_SHIFT) & 7
    assert np.array_equal(xf & 7, vb) and np.array_equal((xf >> 4) & 7, (fl >> L.FLAG_NVIOL_SHIFT) & 3)
    assert all(((vb >> j) & 1).any() for j in range(3)) and not ((xf >> 8) & 7).any()
    env.close()


# ---- 6. refusals and footprint -----------------------------------------------------------------------------------------------
def test_every_other_stepping_entry_point_refuses_while_limits_are_installed(ni):
    L, UNS = ni._lib, 4
    key, B, FILL = "cr", M.B_SMALL, -7.0
    env = _make(ni, key, B)
    S, A, ld, dev = env.state_dim, env.action_dim, env.ld, env.device
    ws = M.random_actor(S, A, 5)
    env.set_policy(ni.mpc_agent(S, A)); env.set_mlp_policy(ws); env.set_mlp_safety(M.random_critic(S, A, 6), 0.5)
    env.set_mlp_ensemble([ws, M.random_actor(S, A, 7)], None, None, "voting", 0.2)
    env.set_mlp_safety_ensemble([M.random_critic(S, A, 8, n_out=2), M.random_critic(S, A, 9, n_out=2)], 1.0, 0.5, 0.2)
    env.set_mlp_constraint(M.random_critic(S, A, 10, n_out=2), 0.1, 0.01)
    env.set_disturbance(ni.Disturbance(obs_noise=0.1, action_noise=0.1, clip=(-1, 1), hold="step"))
    env.reset()
    ring = torch.zeros(1, A, ld, dtype=torch.float32, device=dev)
    rw = torch.full((1, ld), FILL, dtype=torch.float32, device=dev)
    fl = torch.full((1, ld), 0x5A5A5A5B, dtype=torch.int32, device=dev)
    act = torch.full((1, A, ld), FILL, dtype=torch.float32, device=dev)
    plan = env.make_plan(1, ring, rw, fl)
    log = env.episode_log(4)
    lib, h = env._L, env._h
    host = dict(a=np.zeros((A, B), np.float32), a64=np.zeros((A, B)), s=np.full((S, B), FILL, np.float32), r=np.full(B, FILL),
                f=np.full(B, 7, np.uint32))
    hp = lambda x: x.ctypes.data_as(C.c_void_p)
    hs, offs = (C.c_void_p * 1)(h), (C.c_int64 * 1)(0)
    K, KR = int(env.spec.k_step), int(env.spec.k_reset)
    snz = torch.zeros(1, K, ld, dtype=torch.float64, device=dev)
    rnz = torch.zeros(1, KR, ld, dtype=torch.float64, device=dev)
    obs_rows = torch.full((1, B, S), FILL, dtype=torch.float32, device=dev)
    obs_soa = torch.full((1, S, ld), FILL, dtype=torch.float32, device=dev)
    # a library-owned mixed batch of one segment (nig_create_mixed): its borrowed handle gets the limits too
    mixed, info = C.c_void_p(), ni._lib.MixedInfo()
    raw0 = lambda rc: None if rc == 0 else (_ for _ in ()).throw(ni._lib.NigError(f"libnig error {rc}: {lib.nig_last_error().decode()}"))
    raw0(lib.nig_create_mixed(1, (C.c_int32 * 1)(0), (C.c_int64 * 1)(B), env._dev_index, C.c_uint64(SEED), C.c_uint64(0),
                              ni._lib.F_AUTORESET, C.byref(mixed)))
    raw0(lib.nig_mixed_get_info(mixed, C.byref(info)))
    raw0(lib.nig_mixed_reset(mixed, env._stream()))
    mld = int(info.ld)
    mring = torch.zeros(1, int(info.action_dim_max), mld, dtype=torch.float32, device=dev)
    mrw = torch.full((1, mld), FILL, dtype=torch.float32, device=dev)
    mfl = torch.full((1, mld), 0x5A5A5A5B, dtype=torch.int32, device=dev)
    mobs = torch.full((1, int(info.state_dim_max), mld), FILL, dtype=torch.float32, device=dev)
    mseg = C.c_void_p(lib.nig_mixed_segment(mixed, 0))
    p = lambda t: C.c_void_p(t.data_ptr())
    st = env._stream()

    def raw(rc):
        if rc != 0:
            raise ni._lib.NigError(f"libnig error {rc}: {lib.nig_last_error().decode()}")

    calls = {
        "nig_step": lambda: env.step_raw(ring[0], ld),
        "nig_step64": lambda: raw(lib.nig_step64(h, p(torch.zeros(A, ld, dtype=torch.float64, device=dev)), ld, None, None, 0, p(rw), None, p(fl), None, 0, st)),
        "nig_rollout": lambda: env.rollout(1, ring, rw, fl),
        "nig_rollout_sampled": lambda: env.rollout_sampled(1, rw, fl),
        "nig_rollout_policy": lambda: env.rollout_policy(1, rw, fl, None, act),
        "nig_rollout_mlp": lambda: env.rollout_mlp(1, rw, fl, None, act),
        "nig_rollout_mlp_safe": lambda: env.rollout_mlp_safe(1, rw, fl, None, act),
        "nig_rollout_mlp_search": lambda: env.rollout_mlp_search(1, 3, rw, fl, None, act),
        "nig_rollout_mlp_ensemble": lambda: env.rollout_mlp_ensemble(1, rw, fl, None, act),
        "nig_rollout_mlp_gated": lambda: env.rollout_mlp_gated(1, rw, fl, None, act),
        "nig_rollout_mlp_projected": lambda: env.rollout_mlp_projected(1, 4, 0.1, rw, fl, None, act),
        "nig_rollout_policy_disturbed": lambda: env.rollout_policy_disturbed(1, rw, fl, None, act),
        "nig_rollout_mlp_disturbed": lambda: env.rollout_mlp_disturbed(1, rw, fl, None, act),
        "nig_plan_create": lambda: env.make_plan(1, ring, rw, fl),
        "nig_plan_launch": plan.launch,
        "nig_step_host": lambda: raw(lib.nig_step_host(h, hp(host["a"]), None, hp(host["s"]), hp(host["r"]), hp(host["f"]), st)),
        "nig_step_host64": lambda: raw(lib.nig_step_host64(h, hp(host["a64"]), None, hp(host["s"]), hp(host["r"]), hp(host["f"]), st)),
        "nig_rollout_mixed": lambda: raw(lib.nig_rollout_mixed(hs, offs, 1, 1, p(ring), ld, A * ld, 1, p(rw), p(fl), ld, st)),
        "nig_collect_episodes": lambda: log.collect(1, rw, fl),
        "nig_rollout_noise": lambda: env.rollout_noise(1, ring, snz, rnz, rw, fl, obs_rows),
        "nig_rollout_mixed_obs": lambda: raw(lib.nig_rollout_mixed_obs(hs, offs, 1, 1, p(ring), ld, A * ld, 1, p(rw), p(fl), ld, p(obs_soa), ld, S * ld, st)),
        "nig_mixed_step": lambda: raw(lib.nig_mixed_step(mixed, p(mring), p(mrw), p(mfl), st)),
        "nig_mixed_rollout": lambda: raw(lib.nig_mixed_rollout(mixed, 1, p(mring), mring.stride(0), 1, p(mrw), p(mfl), mld, st)),
        "nig_mixed_rollout_obs": lambda: raw(lib.nig_mixed_rollout_obs(mixed, 1, p(mring), mring.stride(0), 1, p(mrw), p(mfl), mld, p(mobs), mobs.stride(0), st)),
    }
    for name in ("nig_mixed_step", "nig_mixed_rollout", "nig_mixed_rollout_obs", "nig_rollout_mixed_obs", "nig_rollout_noise"):
        assert name in calls and hasattr(lib, name)
    assert _code(ni, lambda: env.rollout_policy_limited(1, rw, fl, None, act)) == 1, "no limits installed: NIG_ERR_INVALID"
    env.add_safety_constraint(ni.BoxConstraint("band", {("action", 0): (-0.5, 0.5)}, -1.0))
    one = (ni._lib.LimitStruct * 1)()
    one[0].mask, one[0].lo[0], one[0].hi[0], one[0].penalty = 1, -1.0, 1.0, -1.0
    raw0(lib.nig_set_limits(mseg, 1, one, st))
    mt = C.c_uint32()
    raw0(lib.nig_get_counter(mseg, C.byref(mt)))
    torch.cuda.synchronize()
    before = _handle(env)
    for name, call in calls.items():
        try:
            rc = _code(ni, call)
        except RuntimeError as e:                     # the Python surface's own refusal (none of these go that way today)
            raise AssertionError((name, e))
        assert rc == UNS, (name, rc)
        assert "_limited" in lib.nig_last_error().decode(), name
    torch.cuda.synchronize()
    after = _handle(env)
    assert after["counter"] == before["counter"]
    for k in ("state", "ctr", "life", "ep_ret", "tally"):
        assert np.array_equal(after[k].view(np.uint8), before[k].view(np.uint8)), k
    assert bool((rw == FILL).all()) and bool((fl == 0x5A5A5A5B).all()) and bool((act == FILL).all())
    assert bool((obs_rows == FILL).all()) and bool((obs_soa == FILL).all())
    assert bool((mrw == FILL).all()) and bool((mfl == 0x5A5A5A5B).all()) and bool((mobs == FILL).all())
    mt2 = C.c_uint32()
    raw0(lib.nig_get_counter(mseg, C.byref(mt2)))
    assert mt2.value == mt.value
    raw0(lib.nig_set_limits(mseg, 0, None, st))         # ... and the mixed batch steps again without them
    raw0(lib.nig_mixed_step(mixed, p(mring), p(mrw), p(mfl), st))
    torch.cuda.synchronize()
    assert bool((mrw[0, :B] != FILL).all())
    raw0(lib.nig_mixed_destroy(mixed))
    assert (host["s"] == FILL).all() and (host["r"] == FILL).all() and (host["f"] == 7).all()
    with pytest.raises(RuntimeError, match="added safety constraints"):
        env.get_dataset("random")
    with pytest.raises(RuntimeError, match="added safety constraints"):
        ni.evaluate_episodes(ni.random_agent(S, A), env, n_episodes=2)
    env.remove_safety_constraint("band")              # nig_set_limits(h, 0, ...): everything works again
    assert not env.has_limits and lib.nig_get_limit_count(h) == 0
    env.rollout_policy(1, rw, fl, None, act)
    env.step(ring[0][:, :B], layout="soa")
    torch.cuda.synchronize()
    assert env.counter == before["counter"] + 2 and bool((rw[0, :B] != FILL).all())
    # a built-in name clears its mask bit
    env.remove_safety_constraint("level_safety")
    assert [c.name for c in env.safety_constraints] == ["temperature_limit", "pressure_limit"]
    plan.close(); env.close()


def test_invalid_limits_are_refused_and_the_installed_set_stays(ni):
    INV, UNS = 1, 4
    env = _make(ni, "cr", M.B_SMALL)
    lib, h, S, A = env._L, env._h, env.state_dim, env.action_dim
    st = env._stream()

    def limits(n, **kw):
        arr = (ni._lib.LimitStruct * max(n, 1))()
        for c in range(n):
            arr[c].mask, arr[c].lo[0], arr[c].hi[0], arr[c].penalty = 1, -1.0, 1.0, -1.0
        for k, v in kw.items():
            if k in ("lo", "hi"):
                getattr(arr[0], k)[0] = v
            else:
                setattr(arr[0], k, v)
        return arr

    assert lib.nig_set_limits(h, 2, limits(2), st) == 0 and lib.nig_get_limit_count(h) == 2
    for what, n, arr in (("n > 4", 5, limits(5)), ("n < 0", -1, limits(1)), ("mask bit >= S + A", 1, limits(1, mask=1 << (S + A))),
                         ("empty mask", 1, limits(1, mask=0)), ("lo > hi", 1, limits(1, lo=2.0)), ("NaN bound", 1, limits(1, hi=float("nan"))),
                         ("NULL", 1, None)):
        assert lib.nig_set_limits(h, n, arr, st) == INV, what
        assert lib.nig_get_limit_count(h) == 2, what
    # rows that are not listed may hold anything, NaN included
    assert lib.nig_set_limits(h, 1, limits(1, mask=2, lo=float("nan")), st) == 0 and lib.nig_get_limit_count(h) == 1
    assert lib.nig_set_limits(h, 0, None, st) == 0 and lib.nig_get_limit_count(h) == 0
    assert _code(ni, lambda: env.step(np.zeros((M.B_SMALL, A), np.float32))) == 0
    env.close()
    # the counter word keeps an episode's violations in 16 bits: (3 + n) * max_episode_steps <= 65535
    long = ni.make_batched("ChemicalReactor-v0", M.B_SMALL, max_episode_steps=21845)
    assert lib.nig_set_limits(long._h, 1, limits(1), long._stream()) == INV
    long.close()
    ok = ni.make_batched("ChemicalReactor-v0", M.B_SMALL, max_episode_steps=13107)
    assert lib.nig_set_limits(ok._h, 2, limits(2), ok._stream()) == 0 and lib.nig_set_limits(ok._h, 3, limits(3), ok._stream()) == INV
    ok.close()
    for name in ("AdvancedChemicalReactor-v0", "AdvancedPowerGrid-v0"):
        adv = ni.make_batched(name, M.B_SMALL)
        assert lib.nig_set_limits(adv._h, 1, limits(1), adv._stream()) == UNS
        assert _code(ni, lambda: adv.add_safety_constraint(ni.BoxConstraint("b", {("state", 0): (0.0, 1.0)}, -1.0))) == UNS
        adv.close()


@pytest.mark.parametrize("mode", ["odd", "tight"])
@pytest.mark.parametrize("entry", ["step", "step64", "policy", "mlp"])
def test_footprint_of_the_limited_entry_points(ni, entry, mode):
    """tests/footprint.py arenas around every caller buffer of the four new entry points, on a handle without auto-reset with
    held lanes: pad columns, stride gaps, rows beyond n_steps and the rows of frozen lanes keep the canary, xflags included
    (a frozen lane's xflags word is written: 0); the workspace's pad columns stay as they were."""
    from test_gpu_footprint import Rig, ceil4, clean, gap, pitch
    key, B, n = "cr", 321, 3
    r = Rig(ni, key, B, autoreset=False, max_steps=2)
    S, A, ld, L, lib = r.S, r.A, r.ld, ni._lib, r.L
    r.env.add_safety_constraint(ni.BoxConstraint("trip", {("action", 0): (-0.6, 0.6), ("state", 0): (-np.inf, np.inf)}, -5.0, critical=True))
    closed = entry in ("policy", "mlp")
    if entry == "policy":
        r.env.set_policy(ni.random_agent(S, A))
    elif entry == "mlp":
        r.env.set_mlp_policy(M.random_actor(S, A, 11))
    a = Arena("cuda")
    os_, lda, ldo = pitch(mode, B, ld, 1), pitch(mode, B, ld, 2), pitch(mode, B, ld, 3)
    T_ = n if closed else 1
    rew = a.add("reward_out", "f32", Layout(T_, os_, 1, os_, B))
    fl = a.add("flags_out", "flags", Layout(T_, os_, 1, os_, B))
    xf = a.add("xflags_out", "flags", Layout(T_, os_, 1, os_, B))
    if closed:
        obs = a.add("obs_out", "f32", Layout(n, ceil4(B * S) + gap(mode, 1, mult4=True), 1, B * S, B * S, lane_width=S), align=16)
        act = a.add("act_out", "f32", Layout(n, A * lda + gap(mode, 2), A, lda, B))
    else:
        r64 = a.add("reward64_out", "f64", Layout(1, os_, 1, os_, B))
        fin = a.add("final_obs", "f32", Layout(1, S * ldo, S, ldo, B))
        acts = a.add("actions", "f64" if entry == "step64" else "f32", Layout(1, A * lda, A, lda, B), role="in", extra_outer=0)
    a.build()
    r.reset()
    hold = torch.arange(1, B, 5, device="cuda")
    r.hold(hold)
    p = lambda b: C.c_void_p(b.ptr)
    if closed:
        a.freeze_inputs()
        fn = lib.nig_rollout_policy_limited if entry == "policy" else lib.nig_rollout_mlp_limited
        rc = fn(r.h, n, p(rew), p(fl), os_, p(obs), obs.layout.outer_stride, p(act), lda, act.layout.outer_stride, p(xf), r.st())
        assert rc == 0, lib.nig_last_error()
        torch.cuda.synchronize()
        f = fl.rows(n)[:, 0]
        live = (f & L.FLAG_INACTIVE) == 0
        assert not bool(live[0][hold].any()) and bool(live[0].sum() == B - len(hold)) and not bool(live[-1].any())
        assert bool((xf.rows(n)[:, 0][~live] == 0).all()) and bool((xf.rows(n)[:, 0][live] >> 8).any())
        written = {b.name: dict(n_outer=n) for b in (rew, fl, xf)}
        written.update({b.name: dict(n_outer=n, live=live) for b in (obs, act)})
    else:
        rows = acts.rows()[0]
        vals = torch.rand(A, B, device="cuda", dtype=torch.float64) * 2 - 1
        rows.copy_((vals if entry == "step64" else vals.to(torch.float32)).view(rows.dtype))
        a.freeze_inputs()
        fn = lib.nig_step64_limited if entry == "step64" else lib.nig_step_limited
        for k in range(2):                              # max_steps = 2: the second call finishes every live lane
            if k:
                a.refill("reward_out", "flags_out", "xflags_out", "reward64_out", "final_obs")
            rc = fn(r.h, p(acts), lda, None, None, 0, p(rew), p(r64), p(fl), p(xf), p(fin), ldo, r.st())
            assert rc == 0, lib.nig_last_error()
            torch.cuda.synchronize()
        f = fl.rows(1)[0, 0]
        finished = ((f & (L.FLAG_TERMINATED | L.FLAG_TRUNCATED)) != 0) & ((f & L.FLAG_INACTIVE) == 0)
        assert bool(finished.any()) and not bool(finished[hold].any()) and bool(((f & L.FLAG_INACTIVE) != 0)[hold].all())
        written = {b.name: dict(n_outer=1) for b in (rew, fl, xf, r64)}
        written["final_obs"] = dict(n_outer=1, live=finished[None, :])
    clean([str(x) for x in a.check(written)] + r.workspace_findings(), f"{entry} {mode}")
    r.close()
