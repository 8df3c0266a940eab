"""-m gpu: the fused constraint projection (nig_set_mlp_constraint / nig_rollout_mlp_projected,
BatchedIndustrialEnv.rollout_mlp_projected; "nig-project-v1" in include/nig.h) -- the reference's
ConstrainedIQLAgent.get_safe_action (agents/safety_critical.py:240-370) in the MFMA actor kernel -- against the law restated
on the host (tests/mlp_project_ref.c through tests/projection_ref.py, with the oracle's det_sigmoidf).

Shapes are small on purpose: T steps with max_episode_steps 5 (lanes freeze or reset inside the launch), B = 700 (five full
128-env blocks and a partial one) and B = 5 (one partial wave)."""
import ctypes as C
import functools
import inspect

import numpy as np
import pytest
import torch

import closed_loop_matrix as M
import projection_ref as R
from footprint import Arena, Layout

pytestmark = pytest.mark.gpu

NAMES = dict(M.MFMA_ENVS)                          # every env the family is compiled for (tests/closed_loop_matrix.py)
T, MAXS, SEED = M.T_NEW, M.MAXS_NEW, 0x5EED
BIG = 1.0e30
NEVER = 2.0              # a threshold no sigmoid reaches
ITERS_FILL, GRAD_FILL = -7, 7.5      # what iters_out / grad_out hold before a launch
f32 = np.float32
# (env, C, max_iters): every env of the family, C = 1, 3 and 4, max_iters = 1, 3 and 10
CASES = [("cr", 3, 10), ("pg", 4, 3), ("ra", 1, 1), ("acr", 3, 3), ("apg", 4, 10), ("hvac", 1, 10), ("steel", 4, 1), ("supply", 3, 3)]
MATRIX = [(k, c, mi, B) for k, c, mi in CASES for B in (M.B_BIG, M.B_SMALL)]
NEVER_MATRIX = [(k, c, B) for k, c, _ in CASES for B in (M.B_BIG, M.B_SMALL)]


@pytest.fixture(scope="module")
def ni():
    import neorl_industrial_gym_amd as ni
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return ni


def _random_predictor(S, A, n_out, seed):
    """Logits of order 1 on inputs of order 1 (the state columns are scaled in _nets)."""
    rng, D, h = np.random.default_rng(seed), S + A, 256
    return [(rng.normal(0, 1.0 / np.sqrt(D), (D, h)).astype(f32), rng.normal(0, 0.05, h).astype(f32)),
            (rng.normal(0, 1.0 / np.sqrt(h), (h, h)).astype(f32), rng.normal(0, 0.05, h).astype(f32)),
            (rng.normal(0, np.sqrt(2.0 / h), (h, n_out)).astype(f32), rng.normal(0, 0.1, n_out).astype(f32))]


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32) if x.dtype == np.float32 else (np.ascontiguousarray(x).view(np.uint64) if x.dtype == np.float64 else x)


def _same_f32(a, b):
    """Bit for bit, except that any NaN equals any NaN (the device's and the host's default NaNs differ in their sign bit)."""
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and bool((nan | (_bits(a) == _bits(b))).all())


OUT = ("act", "obs", "reward", "flags", "prob", "viol", "iters", "grad")
PER_C = ("prob", "viol")


def _run(ni, name, autoreset, ws, net, thr, tol, mi, step, B, entry="projected", env_index0=0, t0=0, cuts=(T,), states=None):
    """One rollout of sum(cuts) steps, cut into len(cuts) launches, through nig_rollout_mlp_projected (or nig_rollout_mlp, or the
    gate with `net` as its one member: their own rows).  Host arrays: act / grad [n, B, A], obs [n, B, S], prob / viol [n, C, B],
    iters [n, B].  states: [B, S] start states in place of the reset's."""
    env = ni.make_batched(name, B, seed=SEED, env_index0=env_index0, autoreset=autoreset, tally=True, max_episode_steps=MAXS)
    env.set_mlp_policy(ws)
    Cn = net[2][1].size
    if entry == "projected":
        env.set_mlp_constraint(net, thr, tol)
    elif entry == "gated":
        env.set_mlp_safety_ensemble([net], 1.0, thr, BIG)
    dev, n = env.device, sum(cuts)
    S, A, ld = env.state_dim, env.action_dim, env.ld
    ostep = (B * S + 3) // 4 * 4
    act = torch.zeros(n, A, ld, dtype=torch.float32, device=dev)
    grad = torch.full((n, A, ld), GRAD_FILL, dtype=torch.float32, device=dev)
    obs = torch.zeros(n, ostep, dtype=torch.float32, device=dev)
    fl = torch.zeros(n, ld, dtype=torch.int32, device=dev)
    rw = torch.zeros(n, ld, dtype=torch.float32, device=dev)
    it = torch.full((n, ld), ITERS_FILL, dtype=torch.int32, device=dev)
    pr, vi = (torch.zeros(n, Cn, ld, dtype=torch.float32, device=dev) for _ in range(2))
    p = lambda x: C.c_void_p(x.data_ptr())
    env.counter = t0
    env.reset()
    assert env_index0 == 0 or M.KEY_OF[name] not in M.CLONED
    if states is not None:
        env.set_state(np.array(states, dtype=f32), current_step=0, violation_count=0, done=False)
    else:
        M.install_start(ni, env, M.KEY_OF[name], SEED)
    L, k = ni._lib.lib(), 0
    for m in cuts:
        s = slice(k, k + m)
        with torch.cuda.device(dev):
            if entry == "mlp":
                ni._lib.check(L.nig_rollout_mlp(env._h, m, p(rw[s]), p(fl[s]), ld, p(obs[s]), ostep, p(act[s]), ld, A * ld, env._stream()))
            elif entry == "gated":
                ni._lib.check(L.nig_rollout_mlp_gated(env._h, m, p(rw[s]), p(fl[s]), ld, p(obs[s]), ostep, p(act[s]), ld, A * ld,
                                                      p(pr[s]), None, None, ld, Cn * ld, env._stream()))
            elif ostep != B * S:
                ni._lib.check(L.nig_rollout_mlp_projected(env._h, m, mi, step, p(rw[s]), p(fl[s]), ld, p(obs[s]), ostep, p(act[s]), ld, A * ld,
                                                          p(pr[s]), p(vi[s]), p(it[s]), p(grad[s]), ld, Cn * ld, env._stream()))
            else:
                env.rollout_mlp_projected(m, mi, step, rw[s], fl[s], obs[s].view(m, B, S), act[s], pr[s], vi[s], it[s], grad[s])
        k += m
    torch.cuda.synchronize()
    assert env.counter == t0 + n
    o = dict(act=act[:, :, :B].permute(0, 2, 1).cpu().numpy(), grad=grad[:, :, :B].permute(0, 2, 1).cpu().numpy(),
             obs=obs[:, :B * S].reshape(n, B, S).cpu().numpy(), flags=fl[:, :B].cpu().numpy(), reward=rw[:, :B].cpu().numpy(),
             prob=pr[..., :B].cpu().numpy(), viol=vi[..., :B].cpu().numpy(), iters=it[:, :B].cpu().numpy())
    o["live"] = (o["flags"] & ni._lib.FLAG_INACTIVE) == 0
    o["shielded"] = (o["flags"] & ni._lib.FLAG_SHIELDED) != 0
    o["state"], o["ctr"], o["tally"] = env.get_state().cpu().numpy(), env.ctr.cpu().numpy(), env.tally.cpu().numpy()
    o["t0"], o["env0"] = t0, env_index0
    env.close()
    return o


def _same(a, b, what, lanes=slice(None), cut=False):
    """Every output, the final state, the counters and the tallies, bit for bit, on `lanes` of both runs.  cut: the launches are
    cut differently, so the two float64 return sums of a lane that finishes several episodes associate differently
    (test_gpu_safety_gate.py's bound: n * 2^-52 * sum |term|); every other row stays exact."""
    for k in OUT:
        assert np.array_equal(_bits(a[k][..., lanes] if k in PER_C else a[k][:, lanes]),
                              _bits(b[k][..., lanes] if k in PER_C else b[k][:, lanes])), (what, k)
    assert np.array_equal(_bits(a["state"][lanes]), _bits(b["state"][lanes])), (what, "state")
    assert np.array_equal(a["ctr"][lanes], b["ctr"][lanes]), (what, "ctr")
    ta, tb = a["tally"][:, lanes], b["tally"][:, lanes]
    if cut:
        from neorl_industrial_gym_amd import _lib as L
        n = ta[L.T_EPISODES]
        tol = n * 2.0 ** -52 * np.sqrt(n * np.maximum(ta[L.T_RET_SQ], tb[L.T_RET_SQ]))
        assert (np.abs(ta[L.T_RET_SUM] - tb[L.T_RET_SUM]) <= tol).all(), (what, "tally: sum of returns")
        assert (np.abs(ta[L.T_RET_SQ] - tb[L.T_RET_SQ]) <= n * 2.0 ** -52 * np.maximum(ta[L.T_RET_SQ], tb[L.T_RET_SQ])).all(), (what, "tally: sum of squares")
        rows = [r for r in range(ta.shape[0]) if r not in (L.T_RET_SUM, L.T_RET_SQ)]
        ta, tb = ta[rows], tb[rows]
    assert np.array_equal(_bits(ta), _bits(tb)), (what, "tally")


@functools.lru_cache(maxsize=None)
def _nets(ni, key, n_out):
    """A random actor and a random predictor whose state inputs are scaled by the observed magnitudes
    (test_gpu_safety_gate.py's construction), and the plain actor's run at B = 700 they were scaled on."""
    name = NAMES[key]
    probe = ni.make_batched(name, 1)
    S, A = probe.state_dim, probe.action_dim
    probe.close()
    ws = M.matrix_actor(ni, key, M.random_actor(S, A, 31), SEED)
    net = _random_predictor(S, A, n_out, 60 + n_out)
    o = _run(ni, name, True, ws, net, NEVER, 0.0, 1, 0.1, M.B_BIG, entry="mlp")
    sc = (1.0 / (1.0 + np.abs(o["obs"][o["live"]]).mean(axis=0))).astype(f32)
    net = [(np.concatenate([net[0][0][:S] * sc[:, None], net[0][0][S:]]).astype(f32), net[0][1]), net[1], net[2]]
    # The head biases are shifted so that the median over the lanes of a lane's largest logit is 0.3 on step 0.  A lane whose
    # logits are all <= 0 has d = 0 and a zero gradient: with a tolerance below 0 the lanes between it and 0 could never reach it,
    # and "stopped at the tolerance after some steps" would depend on a step that jumps over that band.
    z, _ = R.forward(net, o["obs"][0], o["act"][0])
    net[2] = (net[2][0], (net[2][1] + f32(0.3 - np.median(z.max(axis=1)))).astype(f32))
    return ws, net, S, A, o


@functools.lru_cache(maxsize=None)
def _limits(ni, oracle, key, n_out, mi):
    """Threshold, tolerance and step from the plain run's step 0, so that all four outcomes occur at B = 700: the threshold is the
    lower quartile of the lanes' largest p0 (a quarter kept), the tolerance the median of their largest logit (a quarter projected
    without a step), and the step moves the median walking lane's largest logit to the tolerance in about max_iters / 2 steps,
    by the first-order estimate -step |g|^2 per step: the lanes nearer than that finish early, the farther ones run out."""
    ws, net, S, A, plain = _nets(ni, key, n_out)
    obs = plain["obs"][0]
    z, g = R.forward(net, obs, oracle.mlp_actions(key, ws, obs))
    zmax = z.max(axis=1)
    thr = float(np.quantile(oracle.detmath_unary("sigmoidf", zmax), 0.25))
    tol = float(np.median(zmax))
    walking = zmax >= tol
    excess, g2 = np.median((zmax - tol)[walking]), np.median((g.astype(np.float64) ** 2).sum(axis=1)[walking])
    step = float(excess / (g2 * max(mi / 2.0, 0.5)))
    return thr, tol, step


@functools.lru_cache(maxsize=None)
def _mixed(ni, oracle, key, n_out, mi, B=M.B_BIG, autoreset=True, env_index0=0, t0=0, cuts=(T,)):
    ws, net, S, A, _ = _nets(ni, key, n_out)
    thr, tol, step = _limits(ni, oracle, key, n_out, mi)
    o = _run(ni, NAMES[key], autoreset, ws, net, thr, tol, mi, step, B, env_index0=env_index0, t0=t0, cuts=cuts)
    o["thr"], o["tol"], o["step"] = thr, tol, step
    return o


# ---- 1: never project ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,n_out,B", NEVER_MATRIX)
def test_at_a_threshold_nothing_reaches_it_is_the_plain_actor(ni, key, n_out, B):
    """Threshold 2: act, obs, reward, flags, final state, counters and tallies are nig_rollout_mlp's bit for bit; prob_out and
    viol_out are the gate's prob row with this predictor as its one member at T = 1; iters_out is -1 on every live lane-step and
    grad_out keeps its fill everywhere."""
    ws, net, S, A, _ = _nets(ni, key, n_out)
    plain = _run(ni, NAMES[key], True, ws, net, NEVER, 0.0, 1, 0.1, B, entry="mlp")
    gate = _run(ni, NAMES[key], True, ws, net, NEVER, 0.0, 1, 0.1, B, entry="gated")
    o = _run(ni, NAMES[key], True, ws, net, NEVER, 0.01, 10, 0.1, B)
    for k in ("act", "obs", "reward", "flags"):
        assert np.array_equal(_bits(o[k]), _bits(plain[k])), k
    assert np.array_equal(_bits(o["state"]), _bits(plain["state"])) and np.array_equal(o["ctr"], plain["ctr"])
    assert np.array_equal(_bits(o["tally"]), _bits(plain["tally"]))
    assert o["live"][0].all() and np.array_equal(_bits(o["prob"]), _bits(gate["prob"])) and np.array_equal(_bits(o["viol"]), _bits(o["prob"]))
    assert o["prob"][0].min() > 0 and (B < 100 or len(np.unique(o["prob"][0, 0])) > B // 2)
    assert (o["iters"][o["live"]] == -1).all() and (o["iters"][~o["live"]] == ITERS_FILL).all()
    assert (o["grad"] == f32(GRAD_FILL)).all() and not o["shielded"].any()


# ---- 2: the law ---------------------------------------------------------------------------------------------------------------
def _check_law(oracle, key, o, ws, net, mi):
    """p0, the first gradient, iters, viol, the action the env received and NIG_FLAG_SHIELDED on every live lane-step against the
    restatement on the device's own observation and the oracle's actor action; frozen lanes keep their fills."""
    live = o["live"]
    for k in range(live.shape[0]):
        lv = live[k]
        want = R.law(oracle, net, o["obs"][k], oracle.mlp_actions(key, ws, o["obs"][k]), o["thr"], o["tol"], mi, o["step"])
        assert _same_f32(o["prob"][k][:, lv], want["p0"].T[:, lv]), (k, "p0")
        assert np.array_equal(o["iters"][k][lv], want["iters"][lv]), (k, "iters")
        assert np.array_equal(o["shielded"][k][lv], want["projected"][lv]), (k, "NIG_FLAG_SHIELDED")
        assert _same_f32(o["viol"][k][:, lv], want["viol"].T[:, lv]), (k, "viol")
        assert _same_f32(o["act"][k][lv], want["act"][lv]), (k, "the action the env received")
        stepped = lv & (want["iters"] >= 1)
        assert _same_f32(o["grad"][k][stepped], want["grad"][stepped]), (k, "the first gradient")
        assert (o["grad"][k][~stepped] == f32(GRAD_FILL)).all(), (k, "grad_out is untouched where iters < 1")
        assert (o["iters"][k][~lv] == ITERS_FILL).all() and not o["prob"][k][:, ~lv].any() and not o["viol"][k][:, ~lv].any()
    assert not o["shielded"][~live].any()


@pytest.mark.parametrize("autoreset", [True, False])
@pytest.mark.parametrize("key,n_out,mi,B", MATRIX)
def test_the_law_bit_for_bit(ni, oracle, key, n_out, mi, B, autoreset):
    """All four outcomes occur on step 0 of the 700-lane runs -- kept, projected without a step, stopped at the tolerance after
    some steps, out of steps -- where max_iters leaves room for the third (max_iters = 1 has no count between 0 and 1).  The
    assertion is on step 0, where every lane is live on its own start state, so AdvancedPowerGrid's plant (an episode ends as
    soon as a projected action's voltage set-points leave 0.95 .. 1) takes nothing from it."""
    ws, net, S, A, _ = _nets(ni, key, n_out)
    o = _mixed(ni, oracle, key, n_out, mi, B, autoreset)
    live = o["live"]
    assert live[0].all() and (autoreset or not live[-1].any())
    _check_law(oracle, key, o, ws, net, mi)
    if B > 100:
        it = o["iters"][0]
        counts = [(it == -1).sum(), (it == 0).sum(), ((it > 0) & (it < mi)).sum(), (it == mi).sum()]
        print(f"{key} C={n_out} max_iters={mi}: kept {counts[0]}, no step {counts[1]}, stopped early {counts[2]}, out of steps {counts[3]}")
        assert counts[0] and counts[1] and counts[3] and (counts[2] or mi == 1), counts
        g = o["grad"][0][it >= 1]
        g = g[np.abs(g).max(axis=1) > 0]          # (a lane whose logits are all <= 0 but not below the tolerance has d = 0)
        # (the gradient is piecewise constant: lanes with the same ReLU pattern share it, and AdvancedChemicalReactor's start
        # states differ along little more than one direction -- 96 distinct rows of 350; more than a wave's 32 lanes is asked)
        assert len(g) > B // 4 and M.distinct_rows(g) > 32 and np.isfinite(g).all()
        moved = np.abs(o["act"][0] - oracle.mlp_actions(key, ws, o["obs"][0])).max(axis=1)
        assert (moved[it >= 1] > 0).sum() >= len(g) // 2 and not moved[it < 1].any()


# ---- 3: the step took that action ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("autoreset", [False, True])
@pytest.mark.parametrize("key,n_out,mi", CASES[:2])
def test_the_step_took_that_action(ni, oracle, key, n_out, mi, autoreset):
    """A second handle (same seed and env_index0) is teacher-forced per step with obs_out[k], the step counters of the flag words
    and the launch counter, and stepped on act_out[k]: its new state is obs_out[k + 1] bit for bit on lanes that did not finish;
    reward and flag word (without NIG_FLAG_SHIELDED) are the rollout's on every live lane."""
    o = _mixed(ni, oracle, key, n_out, mi, M.B_BIG, autoreset)
    L, B = ni._lib, M.B_BIG
    e2 = ni.make_batched(NAMES[key], B, autoreset=autoreset, tally=True, max_episode_steps=MAXS, seed=SEED)
    live, checked = o["live"], 0
    for k in range(T - 1):
        fl = o["flags"][k]
        step_after = (fl.astype(np.uint32) >> L.FLAG_STEP_SHIFT).astype(np.int64)
        ctr = np.where(live[k], step_after - 1, L.CTR_DONE).astype(np.int32)
        e2.state_soa.copy_(torch.from_numpy(np.ascontiguousarray(o["obs"][k].T)).to(e2.device))
        e2.ctr.copy_(torch.from_numpy(ctr).to(e2.device))
        e2.counter = o["t0"] + k
        nxt, rew, _, _, _ = e2.step(torch.from_numpy(np.ascontiguousarray(o["act"][k])).to(e2.device), layout="aos")
        torch.cuda.synchronize()
        nxt, rew, f2 = nxt.cpu().numpy(), rew.cpu().numpy(), e2.flags.cpu().numpy()
        cont = live[k] & live[k + 1] & ((fl & (L.FLAG_TERMINATED | L.FLAG_TRUNCATED | L.FLAG_DID_RESET)) == 0)
        checked += int(cont.sum())
        assert np.array_equal(_bits(o["obs"][k + 1])[cont], _bits(nxt)[cont]), k
        assert np.array_equal(_bits(o["reward"][k])[live[k]], _bits(rew)[live[k]]), k
        assert np.array_equal((fl & ~L.FLAG_SHIELDED)[live[k]], f2[live[k]]), k
    assert checked > B
    assert (o["iters"][live] >= 1).any() and (o["iters"][live] < 1).any()       # moved and untouched actions were both stepped on
    e2.close()


# ---- 4: a lane does not depend on its neighbours ------------------------------------------------------------------------------
@pytest.mark.parametrize("key,n_out,mi", [CASES[0], CASES[1]])
def test_a_lane_does_not_depend_on_its_neighbours(ni, oracle, key, n_out, mi):
    """One walking lane among kept ones (its block votes for passes that only it uses) and one kept lane among walking ones,
    against the runs in which every lane has the one state or the other: each lane's step-0 outputs are those of its own state,
    bit for bit.  B = 200: a full block and a partial one; the odd lanes sit in the full block's second wave and in the
    partial block."""
    ws, net, S, A, _ = _nets(ni, key, n_out)
    base = _mixed(ni, oracle, key, n_out, mi)
    it0 = base["iters"][0]
    kept, walking = base["obs"][0][np.argmax(it0 == -1)], base["obs"][0][np.argmax(it0 == mi)]
    B, odd = 200, [37, 150]
    run = lambda states: _run(ni, NAMES[key], False, ws, net, base["thr"], base["tol"], mi, base["step"], B, cuts=(1,), states=states)
    all_kept, all_walking = run(np.tile(kept, (B, 1))), run(np.tile(walking, (B, 1)))
    assert (all_kept["iters"][0] == -1).all() and (all_walking["iters"][0] == mi).all()
    for mostly, other, a, b in ((kept, walking, all_kept, all_walking), (walking, kept, all_walking, all_kept)):
        states = np.tile(mostly, (B, 1))
        states[odd] = other
        o = run(states)
        rest = np.setdiff1d(np.arange(B), odd)
        for k in ("prob", "viol"):
            assert np.array_equal(_bits(o[k][0][:, rest]), _bits(a[k][0][:, rest])) and np.array_equal(_bits(o[k][0][:, odd]), _bits(b[k][0][:, odd])), k
        for k in ("act", "grad", "iters"):
            assert np.array_equal(_bits(o[k][0][rest]), _bits(a[k][0][rest])) and np.array_equal(_bits(o[k][0][odd]), _bits(b[k][0][odd])), k
        assert np.array_equal(o["shielded"][0], o["iters"][0] >= 0)


# ---- 5: cuts and shards -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,n_out,mi", [CASES[0], CASES[2]])
def test_launch_cuts_and_shards(ni, oracle, key, n_out, mi):
    """One launch of T steps equals two launches of 3 + 4 from the same launch counter; two shards by env_index0 equal the
    unsharded run; B = 5 equals the first five lanes of B = 700: bit for bit in every output and in the final state."""
    one = _mixed(ni, oracle, key, n_out, mi, 700, True, 0, 37)
    two = _mixed(ni, oracle, key, n_out, mi, 700, True, 0, 37, (3, T - 3))
    assert one["shielded"].any() and not one["shielded"][one["live"]].all()
    _same(one, two, "one launch vs two", cut=True)
    whole = _mixed(ni, oracle, key, n_out, mi, 700, False)
    lo, hi = _mixed(ni, oracle, key, n_out, mi, 350, False, 0), _mixed(ni, oracle, key, n_out, mi, 350, False, 350)
    _same(whole, lo, "shard 0", lanes=slice(0, 350))
    for k in OUT:
        a = whole[k][..., 350:] if k in PER_C else whole[k][:, 350:]
        assert np.array_equal(_bits(a), _bits(hi[k])), ("shard 1", k)
    assert np.array_equal(_bits(whole["state"][350:]), _bits(hi["state"])) and np.array_equal(whole["ctr"][350:], hi["ctr"])
    _same(whole, _mixed(ni, oracle, key, n_out, mi, 5, False), "B = 700 vs B = 5", lanes=slice(0, 5))


# ---- 6: a non-finite head bias ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [-np.inf, np.inf])
@pytest.mark.parametrize("key,n_out,mi,c", [("cr", 3, 3, 1), ("pg", 4, 3, 3)])
def test_a_non_finite_head_bias_follows_the_arithmetic(ni, oracle, key, n_out, mi, c, value):
    """c3[c] = +-inf: the head's bias record meets B = 0 on lane half 1, so row c's logit is NaN on the device and in the
    restatement alike.  NaN < thr and NaN < tol are false: every live lane is projected and walks until the steps run out, on the
    gradient of the other rows (d_c = (NaN > 0) = 0).  Every output equals the restatement's (NaN = NaN); the other rows' p0 and
    viol are finite and the other rows' p0 are those of the finite predictor, bit for bit."""
    ws, net, S, A, _ = _nets(ni, key, n_out)
    thr, tol, step = _limits(ni, oracle, key, n_out, mi)
    c3 = net[2][1].copy()
    c3[c] = value
    bad = [net[0], net[1], (net[2][0], c3)]
    o = _run(ni, NAMES[key], False, ws, bad, thr, tol, mi, step, M.B_BIG)
    o["thr"], o["tol"], o["step"] = thr, tol, step
    live = o["live"]
    assert live[0].all() and not live[-1].any()
    _check_law(oracle, key, o, ws, bad, mi)
    assert np.isnan(o["prob"][:, c][live]).all() and np.isnan(o["viol"][:, c][live]).all()
    others = [r for r in range(n_out) if r != c]
    lv = np.broadcast_to(live[:, None], (T, len(others), M.B_BIG))
    assert np.isfinite(o["prob"][:, others][lv]).all() and np.isfinite(o["viol"][:, others][lv]).all()
    assert (o["iters"][live] == mi).all() and o["shielded"][live].all()
    good = _mixed(ni, oracle, key, n_out, mi, M.B_BIG, False)
    assert np.array_equal(_bits(o["prob"][0][others]), _bits(good["prob"][0][others]))


# ---- 7: refusals and footprint ------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(ni):
    L, lib = ni._lib, ni._lib.lib()
    key, n_out = "cr", 3
    ws, net, S, A, _ = _nets(ni, key, n_out)
    B, n = 200, 3
    INVALID, UNSUPPORTED = 1, 4           # NIG_ERR_INVALID, NIG_ERR_UNSUPPORTED
    assert lib.nig_rollout_mlp_projected(None, n, 3, 0.1, None, None, 0, None, 0, None, 0, 0, None, None, None, None, 0, 0, None) == INVALID

    def install(env, hidden=256, Cn=None, thr=0.5, tol=0.01, null=False):
        W = [np.ascontiguousarray(x, dtype=f32) for pair in net for x in pair]
        ptrs = [C.c_void_p(w.ctypes.data) for w in W]
        if null:
            ptrs[4] = None
        return lib.nig_set_mlp_constraint(env._h, hidden, n_out if Cn is None else Cn, *ptrs, thr, tol, env._stream())

    def attempt(env, want, what, mi=3, step=0.1, ld_c=None, c_step=None, n_steps=n, out_stride=None, ld_act=None, act=True):
        ld = env.ld
        bufs = dict(rw=torch.full((n, ld), 7.5, device=env.device), fl=torch.full((n, ld), 0x5A5A5A5B, dtype=torch.int32, device=env.device),
                    obs=torch.full((n, B, S), 7.5, device=env.device), act=torch.full((n, A, ld), 7.5, device=env.device),
                    pr=torch.full((n, n_out, ld), 7.5, device=env.device), vi=torch.full((n, n_out, ld), 7.5, device=env.device),
                    it=torch.full((n, ld), 0x5A5A5A5B, dtype=torch.int32, device=env.device), gr=torch.full((n, A, ld), 7.5, device=env.device))
        before = {k: v.clone() for k, v in bufs.items()}
        state, ctr, t = env.get_state().clone(), env.ctr.clone(), env.counter
        p = lambda x: C.c_void_p(x.data_ptr())
        rc = lib.nig_rollout_mlp_projected(env._h, n_steps, mi, step, p(bufs["rw"]), p(bufs["fl"]), ld if out_stride is None else out_stride,
                                           p(bufs["obs"]), B * S, p(bufs["act"]) if act else None, ld if ld_act is None else ld_act, A * ld,
                                           p(bufs["pr"]), p(bufs["vi"]), p(bufs["it"]), p(bufs["gr"]), ld if ld_c is None else ld_c,
                                           n_out * ld if c_step is None else c_step, env._stream())
        torch.cuda.synchronize()
        assert rc == want, (what, rc, lib.nig_last_error())
        if want != 0:
            for k in bufs:
                assert torch.equal(bufs[k], before[k]), (what, k)
            assert torch.equal(env.get_state(), state) and torch.equal(env.ctr, ctr) and env.counter == t, what

    env = ni.make_batched(NAMES[key], B, max_episode_steps=MAXS)
    env.reset()
    attempt(env, INVALID, "neither actor nor predictor")
    env.set_mlp_policy(ws)
    attempt(env, INVALID, "no predictor installed")
    with pytest.raises(L.NigError):
        env.rollout_mlp_projected(n)
    # refused installations leave "no predictor installed"
    for rc, what, kw in [(INVALID, "C = 0", dict(Cn=0)), (INVALID, "C = 5", dict(Cn=5)), (INVALID, "a NULL array", dict(null=True)),
                         (INVALID, "threshold = NaN", dict(thr=float("nan"))), (INVALID, "threshold = inf", dict(thr=float("inf"))),
                         (INVALID, "tolerance = NaN", dict(tol=float("nan"))), (INVALID, "tolerance = -inf", dict(tol=float("-inf"))),
                         (UNSUPPORTED, "hidden 128", dict(hidden=128))]:
        assert install(env, **kw) == rc, (what, lib.nig_last_error())
        attempt(env, INVALID, what + ": still no predictor")
    assert install(env) == 0
    env.set_mlp_constraint(net, 0.5, 0.01)
    for what, kw in [("max_iters 0", dict(mi=0)), ("max_iters 17", dict(mi=L.MAX_PROJECT_ITERS + 1)), ("max_iters -1", dict(mi=-1)),
                     ("step NaN", dict(step=float("nan"))), ("step inf", dict(step=float("inf"))), ("ld_c < B", dict(ld_c=B - 1)),
                     ("c_step_stride < C * ld_c", dict(c_step=n_out * env.ld - 1)), ("n_steps 0", dict(n_steps=0)),
                     ("out_stride < B", dict(out_stride=B - 1)), ("ld_act < B", dict(ld_act=B - 1)),
                     ("ld_act < B with grad_out alone", dict(ld_act=B - 1, act=False))]:
        attempt(env, INVALID, what, **kw)
    # a refused installation keeps the installed predictor; the largest step count runs
    assert install(env, thr=float("nan")) == INVALID
    attempt(env, 0, "the installed projection runs", mi=L.MAX_PROJECT_ITERS)
    env.close()
    # a predictor without an actor
    env = ni.make_batched(NAMES[key], B, max_episode_steps=MAXS)
    env.reset()
    env.set_mlp_constraint(net, 0.5, 0.01)
    attempt(env, INVALID, "no actor installed")
    env.close()


@pytest.mark.parametrize("pitch", ["B", "B + odd", "beyond ld"])
def test_footprint_of_the_projection_outputs(ni, oracle, pitch):
    """prob_out, viol_out, iters_out and grad_out beside act / obs / reward / flags in canary arenas, lanes freezing inside the
    launch (no auto-reset, episodes of at most 5 steps): no pad column, stride gap, row >= C of a block, frozen-lane or red-zone
    word changes, every documented word is written, and grad_out's words are written exactly where iters >= 1.  The step stride
    leaves room for a fourth row, which C = 3 must not touch."""
    key, n_out, mi, B = "pg", 3, 3, 200
    ws, net, S, A, _ = _nets(ni, key, n_out)
    thr, tol, step = _limits(ni, oracle, key, n_out, mi)
    env = ni.make_batched(NAMES[key], B, seed=SEED, autoreset=False, tally=True, max_episode_steps=MAXS)
    env.set_mlp_policy(ws)
    env.set_mlp_constraint(net, thr, tol)
    ld, lda, ostep = B + 3, B + 5, (B * S + 3) // 4 * 4 + 8
    ld_c = {"B": B, "B + odd": B + 7, "beyond ld": env.ld + 65}[pitch]
    c_step = 4 * ld_c + 5
    a = Arena("cuda")
    rew = a.add("reward_out", "f32", Layout(T, ld, 1, ld, B))
    fl = a.add("flags_out", "flags", Layout(T, ld, 1, ld, B))
    it = a.add("iters_out", "i32", Layout(T, ld, 1, ld, B))
    pr = a.add("prob_out", "f32", Layout(T, c_step, n_out, ld_c, B))
    vi = a.add("viol_out", "f32", Layout(T, c_step, n_out, ld_c, B))
    obs = a.add("obs_out", "f32", Layout(T, ostep, 1, B * S, B * S, lane_width=S), align=16)
    act = a.add("act_out", "f32", Layout(T, A * lda + 7, A, lda, B))
    gr = a.add("grad_out", "f32", Layout(T, A * lda + 7, A, lda, B))
    a.build()
    env.reset()
    p = lambda b: C.c_void_p(b.ptr)
    rc = ni._lib.lib().nig_rollout_mlp_projected(env._h, T, mi, step, p(rew), p(fl), ld, p(obs), ostep, p(act), lda, A * lda + 7, p(pr), p(vi), p(it),
                                                 p(gr), ld_c, c_step, env._stream())
    assert rc == 0, ni._lib.lib().nig_last_error()
    torch.cuda.synchronize()
    f = fl.rows(T)[:, 0]
    live = (f & ni._lib.FLAG_INACTIVE) == 0
    assert bool(live[0].all()) and not bool(live[-1].any())
    stepped = live & (it.rows(T)[:, 0] >= 1)
    assert bool(stepped.any()) and bool((live & ~stepped).any())
    written = {b.name: dict(n_outer=T, live=live if b in (it, pr, vi, obs, act) else None) for b in (rew, fl, it, pr, vi, obs, act)}
    written[gr.name] = dict(n_outer=T, live=stepped)
    findings = [str(x) for x in a.check(written)]
    assert not findings, "\n  ".join(findings)
    env.close()


# ---- 8: evaluate_with_safety --------------------------------------------------------------------------------------------------
def test_evaluate_with_safety_runs_the_fused_projection(ni, oracle, monkeypatch):
    """evaluate_with_safety(ConstraintProjectionPolicy, env) reaches rollout_mlp_projected without a host step or predict.  At a
    threshold nothing reaches, its 13 metrics are the plain actor's, value for value; at the mixed limits lanes are projected and
    the lengths and violations are those of the rows of the same rollout on a second handle."""
    from neorl_industrial_gym_amd.episodes import episodes_from_rows
    key, n_out, mi, n_ep = "cr", 3, 10, 256
    ws, net, S, A, _ = _nets(ni, key, n_out)
    thr, tol, step = _limits(ni, oracle, key, n_out, mi)
    L = ni._lib
    mk = lambda: ni.make_batched(NAMES[key], n_ep, autoreset=False, tally=True, max_episode_steps=24)
    a, b = mk(), mk()
    want = ni.evaluate_with_safety(ni.MLPPolicy(ws), b, n_episodes=n_ep)
    sp = ni.ConstraintProjectionPolicy(ws, net, threshold=NEVER, tolerance=tol, max_iters=mi, step=step)
    assert sp.fusable

    def boom(*_a, **_k):
        raise AssertionError("the fused projection must not step or predict on the host")
    monkeypatch.setattr(a, "step", boom)
    monkeypatch.setattr(sp, "predict", boom)
    monkeypatch.setattr(sp, "predict_device", boom)
    calls = []
    real = a.rollout_mlp_projected
    monkeypatch.setattr(a, "rollout_mlp_projected", lambda *x, **k: (calls.append(x), real(*x, **k)))
    got = ni.evaluate_with_safety(sp, a, n_episodes=n_ep)
    assert calls and all(c[1:3] == (mi, step) for c in calls)
    assert len(got) == 13 and set(got) == set(want)
    for k in want:
        assert got[k] == want[k], k
    a.close(); b.close()
    sp = ni.ConstraintProjectionPolicy(ws, net, threshold=thr, tolerance=tol, max_iters=mi, step=step)
    a, b = mk(), mk()
    got = ni.evaluate_with_safety(sp, a, n_episodes=n_ep)
    sp.install(b)
    b.ctr.fill_(L.CTR_DONE)
    b.reset(mask=torch.ones(n_ep, dtype=torch.uint8, device=b.device))
    rw = torch.zeros(24, b.ld, dtype=torch.float32, device=b.device)
    fl = torch.zeros(24, b.ld, dtype=torch.int32, device=b.device)
    b.rollout_mlp_projected(24, mi, step, rw, fl)
    torch.cuda.synchronize()
    rw, fl = rw[:, :n_ep].cpu().numpy(), fl[:, :n_ep].cpu().numpy()
    live = (fl & L.FLAG_INACTIVE) == 0
    sh = ((fl & L.FLAG_SHIELDED) != 0)[live]
    assert sh.any() and not sh.all()
    rec = episodes_from_rows(rw, fl, bool(b.spec.reward_is_f32), 1)
    ret, w0 = rec["ret"][0], rec["w"][0, 0]
    lens, viol = (w0 & L.CTR_STEP_MASK).astype(np.int64), (w0 >> L.CTR_VIOL_SHIFT).astype(np.int64)
    assert np.array_equal(lens, live.sum(axis=0))
    assert got["length_mean"] == np.mean(lens) and got["safety_violations"] == viol.sum()
    assert got["return_min"] == ret.min() and got["return_max"] == ret.max()
    a.close(); b.close()
    # under a Disturbed wrapper the policy takes the host loop, as the search does
    from neorl_industrial_gym_amd.utils import _install_agent
    e = mk()
    wrapped = ni.Disturbed(sp, ni.Disturbance(obs_noise=0.01))
    assert _install_agent(wrapped, e)[1] is None
    assert _install_agent(sp, e)[1] is not None
    e.close()


# ---- 9: the module's own guard ------------------------------------------------------------------------------------------------
def test_the_matrix_tests_cover_the_family_and_the_odd_env_is_refused(ni):
    """The two matrix tests run on every env of M.MFMA_ENVS at both batch sizes with C = 1, 3, 4 and max_iters = 1, 3, 10 among
    them; WaterTreatment (S = 15) has no MFMA actor: installation and launch return NIG_ERR_UNSUPPORTED and every output keeps
    its fill."""
    keys = {k for k, _ in M.MFMA_ENVS}
    for rows in (MATRIX, NEVER_MATRIX):
        assert {(r[0], r[-1]) for r in rows} == {(k, B) for k in keys for B in (M.B_BIG, M.B_SMALL)}
    assert {c for _, c, _ in CASES} == {1, 3, 4} and {mi for _, _, mi in CASES} == {1, 3, 10}
    for fn, rows in ((test_the_law_bit_for_bit, MATRIX), (test_at_a_threshold_nothing_reaches_it_is_the_plain_actor, NEVER_MATRIX)):
        marks = [m for m in fn.pytestmark if m.name == "parametrize" and "B" in m.args[0]]
        assert len(marks) == 1 and list(marks[0].args[1]) == rows, inspect.getsource(fn)[:80]
    lib = ni._lib.lib()
    water = ni.make_batched("WaterTreatment-v0", 64)
    water.reset()
    Sw, Aw, ld, n = water.state_dim, water.action_dim, water.ld, 2
    net = _random_predictor(Sw, Aw, 3, 5)
    W = [np.ascontiguousarray(x, dtype=f32) for pair in net for x in pair]
    assert lib.nig_set_mlp_constraint(water._h, 256, 3, *[C.c_void_p(w.ctypes.data) for w in W], 0.5, 0.01, water._stream()) == 4
    bufs = dict(rw=torch.full((n, ld), 7.5, device=water.device), fl=torch.full((n, ld), 0x5A5A5A5B, dtype=torch.int32, device=water.device),
                obs=torch.full((n, 64, Sw + 1), 7.5, device=water.device), act=torch.full((n, Aw, ld), 7.5, device=water.device),
                pr=torch.full((n, 3, ld), 7.5, device=water.device), vi=torch.full((n, 3, ld), 7.5, device=water.device),
                it=torch.full((n, ld), 0x5A5A5A5B, dtype=torch.int32, device=water.device), gr=torch.full((n, Aw, ld), 7.5, device=water.device))
    before = {k: v.clone() for k, v in bufs.items()}
    p = lambda x: C.c_void_p(x.data_ptr())
    rc = lib.nig_rollout_mlp_projected(water._h, n, 3, 0.1, p(bufs["rw"]), p(bufs["fl"]), ld, p(bufs["obs"]), 64 * (Sw + 1), p(bufs["act"]), ld, Aw * ld,
                                       p(bufs["pr"]), p(bufs["vi"]), p(bufs["it"]), p(bufs["gr"]), ld, 3 * ld, water._stream())
    torch.cuda.synchronize()
    assert rc == 4, lib.nig_last_error()
    for k in bufs:
        assert torch.equal(bufs[k], before[k]), k
    water.close()
