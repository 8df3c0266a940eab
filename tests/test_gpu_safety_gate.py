"""-m gpu: the fused safety-ensemble gate (nig_set_mlp_safety_ensemble / nig_rollout_mlp_gated, BatchedIndustrialEnv.rollout_mlp_gated;
"nig-gate-v1" in include/nig.h) -- the reference's SafeEnsembleAgent.get_safe_action (agents/safety_critical.py:391-532) in the MFMA
actor kernel -- against the law restated on the host.

The restatement: row c of a member is, bit for bit, a one-output critic with C3[:, c:c+1] and c3[c], so oracle.mlp_critic gives
sigmoid(z_m[c]) and pins the logit to the resolution of the sigmoid; everything after the logits is the law in NumPy float32 with
the oracle's det_sigmoidf, applied to the device's own logit_out.

Shapes are small on purpose: T steps with max_episode_steps 5 (lanes freeze or reset inside the launch), B = 700 (five full
128-env blocks and a partial one) and B = 5 (one partial wave)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import closed_loop_matrix as M
from footprint import Arena, Layout

pytestmark = pytest.mark.gpu

# ChemicalReactor: A = 3, one-chunk critic layer 1, odd S + A; PowerGrid: two-chunk layer 1, 16x16x1 actor head;
# RobotAssembly: A = 7; HVACControl: a build-specified plant; SteelAnnealing and AdvancedChemicalReactor: A = 6, an even
# one-chunk layer 1 (width 26: no zero-padded k-step); SupplyChain: A = 10 (actor head rows 8 and 9 from the third source-lane
# group), layer-1 width 38 (two chunks, 20 records, no padding record); AdvancedPowerGrid: PowerGrid's shapes.  The two Advanced
# envs draw nothing, so their lanes start from closed_loop_matrix.start_states (from reset() they would all be clones).
NAMES = dict(M.MFMA_ENVS)                          # every env the family is compiled for (tests/closed_loop_matrix.py)
T, MAXS, SEED = 7, 5, 0x5EED
KMAX = 8
HEAD_STD = 0.04          # independent members then differ by a few tenths in their logits (the spread limit of the law is 0.2)
BIG = 1.0e30             # a spread limit no finite spread reaches
f32 = np.float32


@pytest.fixture(scope="module")
def ni():
    import neorl_industrial_gym_amd as ni
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return ni


def _random_actor(S, A, seed):       # the style of test_gpu_safe_action_search.py
    rng = np.random.default_rng(seed)
    return [(rng.normal(0, 1.0 / np.sqrt(S), (S, 256)).astype(f32) * f32(0.05), rng.normal(0, 0.05, 256).astype(f32)),
            (rng.normal(0, 1.0 / 16, (256, 256)).astype(f32), rng.normal(0, 0.05, 256).astype(f32)),
            (rng.normal(0, 1.0 / 8, (256, A)).astype(f32), rng.normal(0, 0.1, A).astype(f32))]


def _random_member(S, A, n_out, seed, h=256):
    rng = np.random.default_rng(seed)
    D = S + A
    return [(rng.normal(0, 1.0 / np.sqrt(D), (D, h)).astype(f32) * f32(0.05), rng.normal(0, 0.05, h).astype(f32)),
            (rng.normal(0, 1.0 / np.sqrt(h), (h, h)).astype(f32), rng.normal(0, 0.05, h).astype(f32)),
            (rng.normal(0, HEAD_STD, (h, n_out)).astype(f32), rng.normal(0, 0.1, n_out).astype(f32))]


def _column(member, c):
    """Row c of a member as the one-output critic the oracle evaluates."""
    return [member[0], member[1], (np.ascontiguousarray(member[2][0][:, c:c + 1]), member[2][1][c:c + 1].copy())]


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32) if x.dtype == np.float32 else (np.ascontiguousarray(x).view(np.uint64) if x.dtype == np.float64 else x)


OUT = ("act", "obs", "reward", "flags", "prob", "unc", "logit")


def _run(ni, name, autoreset, ws, ms, Tm, thr, umax, B, entry="gated", env_index0=0, t0=0, cuts=(T,)):
    """One rollout of sum(cuts) steps, cut into len(cuts) launches, through rollout_mlp_gated (or rollout_mlp: its prob / unc /
    logit rows stay zero).  Returns the outputs as host arrays: act [n, B, A], obs [n, B, S], prob / unc [n, C, B],
    logit [n, K, C, B]."""
    env = ni.make_batched(name, B, seed=SEED, env_index0=env_index0, autoreset=autoreset, tally=True, max_episode_steps=MAXS)
    env.set_mlp_policy(ws)
    K, Cn = len(ms), ms[0][2][1].size
    if entry == "gated":
        env.set_mlp_safety_ensemble(ms, Tm, thr, umax)
    dev, n = env.device, sum(cuts)
    S, A, ld = env.state_dim, env.action_dim, env.ld
    ostep = (B * S + 3) // 4 * 4      # (an observation step is a multiple of 4 floats: padded where B * S is none)
    act = torch.zeros(n, A, ld, dtype=torch.float32, device=dev)
    obs = torch.zeros(n, ostep, dtype=torch.float32, device=dev)
    fl = torch.zeros(n, ld, dtype=torch.int32, device=dev)
    rw = torch.zeros(n, ld, dtype=torch.float32, device=dev)
    pr, un = (torch.zeros(n, Cn, ld, dtype=torch.float32, device=dev) for _ in range(2))
    lg = torch.zeros(n, K, Cn, ld, dtype=torch.float32, device=dev)
    p = lambda x: C.c_void_p(x.data_ptr())
    env.counter = t0
    env.reset()
    assert env_index0 == 0 or M.KEY_OF[name] not in M.CLONED
    M.install_start(ni, env, M.KEY_OF[name], SEED)
    k = 0
    for m in cuts:
        s = slice(k, k + m)
        if entry == "mlp":
            L = ni._lib.lib()
            with torch.cuda.device(dev):
                ni._lib.check(L.nig_rollout_mlp(env._h, m, p(rw[s]), p(fl[s]), ld, p(obs[s]), ostep, p(act[s]), ld, A * ld, env._stream()))
        elif ostep != B * S:
            L = ni._lib.lib()
            with torch.cuda.device(dev):
                ni._lib.check(L.nig_rollout_mlp_gated(env._h, m, p(rw[s]), p(fl[s]), ld, p(obs[s]), ostep, p(act[s]), ld, A * ld,
                                                      p(pr[s]), p(un[s]), p(lg[s]), ld, Cn * ld, env._stream()))
        else:
            env.rollout_mlp_gated(m, rw[s], fl[s], obs[s].view(m, B, S), act[s], pr[s], un[s], lg[s])
        k += m
    torch.cuda.synchronize()
    assert env.counter == t0 + n
    o = dict(act=act[:, :, :B].permute(0, 2, 1).cpu().numpy(), obs=obs[:, :B * S].reshape(n, B, S).cpu().numpy(), flags=fl[:, :B].cpu().numpy(),
             reward=rw[:, :B].cpu().numpy(), prob=pr[..., :B].cpu().numpy(), unc=un[..., :B].cpu().numpy(), logit=lg[..., :B].cpu().numpy())
    o["live"] = (o["flags"] & ni._lib.FLAG_INACTIVE) == 0
    o["shielded"] = (o["flags"] & ni._lib.FLAG_SHIELDED) != 0
    o["uncertain"] = (o["flags"] & ni._lib.FLAG_UNCERTAIN) != 0
    o["state"] = env.get_state().cpu().numpy()
    o["ctr"] = env.ctr.cpu().numpy()
    o["tally"] = env.tally.cpu().numpy()
    o["t0"], o["env0"] = t0, env_index0
    env.close()
    return o


def _same(a, b, what, lanes=slice(None), cut=False):
    """Every output, the final state, the counters and the tallies, bit for bit, on `lanes` of both runs.  cut: the runs cut
    their launches differently.  A launch sums the returns (and their squares) of the episodes it finishes in registers and adds
    the sum to the handle's tally at its end -- every closed-loop kernel does -- so two cuts associate those two float64 sums
    differently where a lane finishes several episodes: for them the bound is that of reassociating n terms, n * 2^-52 * sum |term|
    (the squares: their sum itself; the returns: sum |r| <= sqrt(n * sum r^2)); every other row stays exact."""
    for k in OUT:
        assert np.array_equal(_bits(a[k][..., lanes] if k in ("prob", "unc", "logit") else a[k][:, lanes]),
                              _bits(b[k][..., lanes] if k in ("prob", "unc", "logit") else b[k][:, lanes])), (what, k)
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
    """A random actor and KMAX independent random members whose state inputs are scaled by the observed magnitudes
    (test_gpu_safe_action_search.py's construction: state columns of the order of 100 would saturate the first layer), and
    the ungated run at B = 700 they were scaled on."""
    name = NAMES[key]
    probe = ni.make_batched(name, 1)
    S, A = probe.state_dim, probe.action_dim
    probe.close()
    ws = M.matrix_actor(ni, key, _random_actor(S, A, 31), SEED)
    ms = [_random_member(S, A, n_out, 40 + m) for m in range(KMAX)]
    o = _run(ni, name, True, ws, ms[:1], 1.0, 2.0, BIG, 700, entry="mlp")
    sc = (1.0 / (1.0 + np.abs(o["obs"][o["live"]]).mean(axis=0))).astype(f32)
    ms = [[(np.concatenate([m[0][0][:S] * f32(20.0) * sc[:, None], m[0][0][S:] * f32(20.0)]).astype(f32), m[0][1]), m[1], m[2]] for m in ms]
    return ws, ms, S, A, o


@functools.lru_cache(maxsize=None)
def _accept_all(ni, key, n_out, K, Tm, B=700, autoreset=True):
    """The first run: limits nothing reaches.  Its step-0 medians give the limits of the mixed runs."""
    ws, ms, S, A, _ = _nets(ni, key, n_out)
    return _run(ni, NAMES[key], autoreset, ws, ms[:K], Tm, 2.0, BIG, B)


def _medians(o, q=0.5):
    """(quantile q -- the median -- over the lanes of the largest p of a lane, median of its largest sd) on step 0."""
    return float(np.quantile(o["prob"][0].max(axis=0), q)), float(np.median(o["unc"][0].max(axis=0)))


@functools.lru_cache(maxsize=None)
def _mixed(ni, key, n_out, K, Tm, B=700, autoreset=True, env_index0=0, t0=0, cuts=(T,)):
    """The run at the median limits of the accept-all run at B = 700: both branches of both comparisons share waves."""
    ws, ms, S, A, _ = _nets(ni, key, n_out)
    # AdvancedChemicalReactor's start states differ along little more than one direction (one step from one state, half of the
    # action ranges clipped away), and a lane's largest p and largest sd rise together along it: at the two medians the lanes
    # rejected for their probability ARE the lanes rejected for their spread, and "rejected for its probability alone" never
    # occurs.  Its probability limit is therefore the lower quartile: the quarter of the lanes between it and the median has it.
    thr, umax = _medians(_accept_all(ni, key, n_out, K, Tm), 0.25 if key == "acr" else 0.5)
    if K == 1:
        umax = 0.2
    o = _run(ni, NAMES[key], autoreset, ws, ms[:K], Tm, thr, umax, B, env_index0=env_index0, t0=t0, cuts=cuts)
    o["thr"], o["umax"] = thr, umax
    return o


def _law(oracle, z, Tm, thr, umax):
    """Section "nig-gate-v1" of include/nig.h in NumPy float32 on the members' logits z [K, C, n]: (p [C, n], sd [C, n],
    safe [n], certain [n])."""
    K = z.shape[0]
    kf = f32(K)
    with np.errstate(all="ignore"):
        acc, s1, s2 = z[0].copy(), np.zeros_like(z[0]), np.zeros_like(z[0])
        for m in range(1, K):
            acc = acc + z[m]
            d = z[m] - z[0]
            s1 = s1 + d
            s2 = s2 + d * d
        v = s2 - (s1 * s1) / kf
        v = np.where(v < 0, f32(0), v).astype(f32)
        sd = np.sqrt(v / kf)
        pen = np.where(sd > 1, f32(1), sd).astype(f32)
        p = oracle.detmath_unary("sigmoidf", (acc / kf) / f32(Tm)) + f32(0.5) * pen
        p = np.where(p < 0, f32(0), np.where(p > 1, f32(1), p)).astype(f32)
        safe, certain = (p < f32(thr)).all(axis=0), (sd < f32(umax)).all(axis=0)
    assert p.dtype == f32 and sd.dtype == f32
    return p, sd, safe, certain


def _check_law(ni, oracle, key, o, ws, Tm, thr, umax):
    """prob, unc, both flag bits and the action the env received on every live lane-step, bit for bit from the device's own
    logit_out; the raw action is the oracle's actor on the device's own observation."""
    live = o["live"]
    accepted = np.zeros_like(live)
    for k in range(live.shape[0]):
        lv = live[k]
        p, sd, safe, certain = _law(oracle, o["logit"][k], Tm, thr, umax)
        assert np.array_equal(_bits(o["prob"][k])[:, lv], _bits(p)[:, lv]), (k, "prob")
        assert np.array_equal(_bits(o["unc"][k])[:, lv], _bits(sd)[:, lv]), (k, "unc")
        ok = safe & certain
        assert np.array_equal(o["shielded"][k][lv], ~ok[lv]), (k, "NIG_FLAG_SHIELDED")
        assert np.array_equal(o["uncertain"][k][lv], ~certain[lv]), (k, "NIG_FLAG_UNCERTAIN")
        raw = oracle.mlp_actions(key, ws, o["obs"][k])
        want = np.where(ok[:, None], raw, f32(0.0)).astype(f32)
        assert np.array_equal(_bits(o["act"][k])[lv], _bits(want)[lv]), (k, "the action the env received")
        accepted[k] = lv & ok
    assert not (o["shielded"] | o["uncertain"])[~live].any()
    return accepted


# ---- 1: one member anchors to the oracle -----------------------------------------------------------------------------------
@pytest.mark.parametrize("key,n_out,B,autoreset", [("cr", 3, 700, True), ("cr", 1, 5, False), ("pg", 1, 700, False), ("ra", 4, 700, True),
                                                     ("hvac", 1, 700, True), ("pg", 4, 5, True),
                                                     ("ra", 1, 5, False), ("hvac", 3, 5, True), ("acr", 3, 700, True), ("acr", 1, 5, False),
                                                     ("apg", 4, 700, False), ("apg", 1, 5, True), ("steel", 1, 700, True), ("steel", 3, 5, False),
                                                     ("supply", 4, 700, True), ("supply", 4, 5, False), ("supply", 1, 700, False)])
def test_one_member_is_the_oracles_critic_row_by_row(ni, oracle, key, n_out, B, autoreset):
    """K = 1, T = 1: unc is exactly 0 and prob[c] is oracle.mlp_critic of column c, bit for bit, on the device's own
    observation and the oracle's raw action; the env received the raw action where every p is below the limit and zero elsewhere.
    The limit is the median of the lanes' largest p, so both outcomes occur."""
    ws, ms, S, A, _ = _nets(ni, key, n_out)
    o = _mixed(ni, key, n_out, 1, 1.0, B, autoreset)
    live, thr = o["live"], f32(o["thr"])
    assert live[0].all() and (autoreset or not live[-1].any())
    assert not o["unc"].any() and not np.signbit(o["unc"]).any()
    for k in range(T):
        lv = live[k]
        raw = oracle.mlp_actions(key, ws, o["obs"][k])
        p = np.stack([oracle.mlp_critic(key, _column(ms[0], c), o["obs"][k], raw) for c in range(n_out)])
        assert np.array_equal(_bits(o["prob"][k])[:, lv], _bits(p)[:, lv]), k
        ok = (p < thr).all(axis=0)
        assert np.array_equal(o["shielded"][k][lv], ~ok[lv]) and not o["uncertain"][k].any(), k
        assert np.array_equal(_bits(o["act"][k])[lv & ok], _bits(raw)[lv & ok]), k
        assert not _bits(o["act"][k])[lv & ~ok].any(), k
        if k == 0 and key in M.FLOAT64_KEYS:       # the shapes only these envs bring, against the networks in NumPy float64
            raw64 = M.actor64(ws, o["obs"][0])
            assert M.worst(f"{key} B={B}: the actor's action of step 0 against float64", raw, raw64, M.ACT_ATOL) <= 1.0
            p64 = np.stack([M.critic64(_column(ms[0], c), o["obs"][0], raw64) for c in range(n_out)])
            assert M.worst(f"{key} B={B} C={n_out}: prob of step 0 against float64", o["prob"][0], p64, M.PROB_ATOL) <= 1.0
    if B > 100:
        assert o["shielded"][0].any() and not o["shielded"][0].all()
        if key in M.CLONED:
            assert M.distinct_rows(oracle.mlp_actions(key, ws, o["obs"][0])) >= 600, "step 0: the lanes are no clones of each other"


@pytest.mark.parametrize("key", ["cr", "pg", "hvac"])
def test_one_member_one_row_is_the_shields_decision_and_the_plain_actor(ni, key):
    """C = 1, K = 1, T = 1.  At limits nothing reaches the gate is rollout_mlp: act, obs, reward, flags, final state, counters and
    tallies bit for bit.  At the median limit its SHIELDED set and prob row on step 0 are rollout_mlp_safe's at the same
    threshold (from step 1 on the two loops differ by design: the shield halves the action, the gate commands zero)."""
    ws, ms, S, A, plain = _nets(ni, key, 1)
    o = _accept_all(ni, key, 1, 1, 1.0)
    for k in ("act", "obs", "reward", "flags"):
        assert np.array_equal(_bits(o[k]), _bits(plain[k])), k
    assert np.array_equal(_bits(o["state"]), _bits(plain["state"])) and np.array_equal(o["ctr"], plain["ctr"])
    assert np.array_equal(_bits(o["tally"]), _bits(plain["tally"]))
    g = _mixed(ni, key, 1, 1, 1.0)
    env = ni.make_batched(NAMES[key], 700, seed=SEED, autoreset=True, tally=True, max_episode_steps=MAXS)
    env.set_mlp_policy(ws)
    env.set_mlp_safety(ms[0], g["thr"])
    fl = torch.zeros(1, env.ld, dtype=torch.int32, device=env.device)
    pr = torch.zeros(1, env.ld, dtype=torch.float32, device=env.device)
    env.reset()
    env.rollout_mlp_safe(1, None, fl, None, None, pr)
    torch.cuda.synchronize()
    shield = (fl[0, :700].cpu().numpy() & ni._lib.FLAG_SHIELDED) != 0
    assert np.array_equal(shield, g["shielded"][0]) and shield.any() and not shield.all()
    assert np.array_equal(_bits(pr[0, :700].cpu().numpy()), _bits(g["prob"][0, 0]))
    env.close()


# ---- 2, 3, 4: logits, the law, the reference's formula ------------------------------------------------------------------------
CASES = [("cr", 3, 5, 1.0), ("pg", 4, 8, 1.5), ("ra", 1, 2, 1.5), ("hvac", 3, 2, 1.0), ("cr", 4, 8, 1.5), ("pg", 1, 5, 1.0),
         ("acr", 3, 5, 1.0), ("apg", 4, 2, 1.5), ("steel", 1, 3, 1.0), ("supply", 4, 8, 1.5)]
assert {c[0] for c in CASES} == set(NAMES)


@pytest.mark.parametrize("key,n_out,K,Tm", CASES[:4] + CASES[6:])
def test_every_logit_is_the_oracles_critic_on_that_column(ni, oracle, key, n_out, K, Tm):
    """sigmoidf(logit_out) of every member and row equals oracle.mlp_critic of that column, bit for bit, on lanes of full blocks
    and of the partial last block."""
    ws, ms, S, A, _ = _nets(ni, key, n_out)
    o = _mixed(ni, key, n_out, K, Tm)
    lanes = np.r_[0:160, 640:700]
    for k in range(T):
        lv = o["live"][k][lanes]
        obs = o["obs"][k][lanes]
        raw = oracle.mlp_actions(key, ws, obs)
        for m in range(K):
            for c in range(n_out):
                want = oracle.mlp_critic(key, _column(ms[m], c), obs, raw)
                got = oracle.detmath_unary("sigmoidf", o["logit"][k, m, c][lanes])
                assert np.array_equal(_bits(got)[lv], _bits(want)[lv]), (k, m, c)
                if k == 0 and key in M.FLOAT64_KEYS and m in (0, K - 1):      # and against the member in NumPy float64
                    p64 = M.critic64(_column(ms[m], c), obs, M.actor64(ws, obs))
                    assert M.worst(f"{key} member {m} row {c}: sigmoid(logit) of step 0 against float64", got, p64, M.PROB_ATOL) <= 1.0
    z = o["logit"][0]
    assert len(np.unique(z[0, 0])) > 350, "the members do not spread their logits over the lanes"


@pytest.mark.parametrize("B,autoreset", [(700, True), (700, False), (5, False)])
@pytest.mark.parametrize("key,n_out,K,Tm", CASES)
def test_the_law_bit_for_bit_from_the_logits(ni, oracle, key, n_out, K, Tm, B, autoreset):
    """prob, unc, NIG_FLAG_SHIELDED, NIG_FLAG_UNCERTAIN and act_out from logit_out by the NumPy float32 restatement, at limits
    set to the medians of a first run: accepted lanes, lanes rejected for their probability alone and lanes rejected for their
    spread all occur on step 0 of the 700-lane runs."""
    ws, ms, S, A, _ = _nets(ni, key, n_out)
    o = _mixed(ni, key, n_out, K, Tm, B, autoreset)
    live = o["live"]
    assert live[0].all() and (autoreset or not live[-1].any())
    accepted = _check_law(ni, oracle, key, o, ws, Tm, o["thr"], o["umax"])
    if B > 100:
        sh, un = o["shielded"][0], o["uncertain"][0]
        assert accepted[0].any() and (sh & ~un).any() and un.any(), (accepted[0].sum(), (sh & ~un).sum(), un.sum())
        spread = o["unc"][0]
        assert 0.03 < np.median(spread) < 1.0, "independent members should differ by a few tenths in their logits"


@pytest.mark.parametrize("key,n_out,K,Tm", [c for c in CASES if c[2] > 1])
def test_prob_and_unc_against_the_references_formula(ni, key, n_out, K, Tm):
    """The reference's arithmetic in float64 on the device's logit_out -- np.mean, two-pass np.std, 1 / (1 + exp(-x / T)),
    minimum, clip -- within the project's bar: 1e-5 relative with an absolute floor of 1e-6, on every live lane-step."""
    o = _mixed(ni, key, n_out, K, Tm)
    z = o["logit"].astype(np.float64)                                       # [n, K, C, B]
    mean, sd = np.mean(z, axis=1), np.std(z, axis=1)
    p = np.clip(1.0 / (1.0 + np.exp(-mean / Tm)) + 0.5 * np.minimum(sd, 1.0), 0.0, 1.0)
    lv = np.broadcast_to(o["live"][:, None, :], p.shape)
    for got, want, what in ((o["prob"], p, "prob"), (o["unc"], sd, "unc")):
        err = np.abs(got.astype(np.float64) - want)[lv]
        bound = np.maximum(1e-6, 1e-5 * np.abs(want[lv]))
        print(f"{key} K={K} {what}: worst error / bound = {(err / bound).max():.3g}")
        assert (err <= bound).all(), what


# ---- 5: the step took that action ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("autoreset", [False, True])
@pytest.mark.parametrize("key,n_out,K,Tm", CASES[:2])
def test_the_step_took_that_action(ni, key, n_out, K, Tm, autoreset):
    """A second handle (same seed and env_index0) is teacher-forced per step with obs_out[k], the step counters of the flag
    words and the launch counter, and stepped on act_out[k]: its new state is obs_out[k + 1] bit for bit on lanes that did not
    finish; reward and flag word (without the gate's two bits) are the rollout's on every live lane."""
    o = _mixed(ni, key, n_out, K, Tm, 700, autoreset)
    L, B = ni._lib, 700
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
        assert np.array_equal((fl & ~(L.FLAG_SHIELDED | L.FLAG_UNCERTAIN))[live[k]], f2[live[k]]), k
    assert checked > B
    assert o["shielded"][live].any() and not o["shielded"][live].all()      # zeroed and untouched actions were both stepped on
    e2.close()


# ---- 6, 7: identical members, non-finite members ------------------------------------------------------------------------------
@pytest.mark.parametrize("key,n_out", [("cr", 3), ("pg", 4)])
def test_identical_members_have_no_spread(ni, oracle, key, n_out):
    ws, ms, S, A, _ = _nets(ni, key, n_out)
    o = _run(ni, NAMES[key], True, ws, [ms[2]] * 5, 1.5, 0.6, 0.2, 700)
    assert o["live"].all() and not _bits(o["unc"]).any() and not o["uncertain"].any()
    assert np.array_equal(_bits(o["logit"][:, 0]), _bits(o["logit"][:, 4]))
    _check_law(ni, oracle, key, o, ws, 1.5, 0.6, 0.2)


@pytest.mark.parametrize("value", [-np.inf, np.inf])
@pytest.mark.parametrize("key,n_out,K,bad,c", [("cr", 3, 5, 2, 1), ("pg", 4, 2, 0, 3)])
def test_a_non_finite_member_rejects(ni, key, n_out, K, bad, c, value):
    """One member's c3[c] = -inf: its logit is not finite (the head's bias record meets B = 0 on lane half 1, so the device's
    own logit is NaN where the reference's is -inf), the spread of row c is NaN (the law's clamp keeps it), NaN < umax is false:
    every live lane is rejected with both flag bits and the env received zero -- at limits every finite value meets.  + inf
    rejects too."""
    ws, ms, S, A, _ = _nets(ni, key, n_out)
    ms = [list(m) for m in ms[:K]]
    c3 = ms[bad][2][1].copy()
    c3[c] = value
    ms[bad][2] = (ms[bad][2][0], c3)
    o = _run(ni, NAMES[key], False, ws, ms, 1.0, 2.0, BIG, 700)
    live = o["live"]
    assert live[0].all() and not live[-1].any()
    assert not np.isfinite(o["logit"][:, bad, c][live]).any()
    assert np.isfinite(np.delete(o["logit"], bad, axis=1)[:, :, c][np.broadcast_to(live[:, None], (T, K - 1, 700))]).all()
    assert np.isnan(o["unc"][:, c][live]).all()
    others = [r for r in range(n_out) if r != c]
    assert np.isfinite(o["unc"][:, others][np.broadcast_to(live[:, None], (T, len(others), 700))]).all()
    assert o["shielded"][live].all() and o["uncertain"][live].all()
    assert not _bits(o["act"])[live].any()


# ---- 8: cuts and shards --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,n_out,K,Tm", [CASES[0], CASES[2]])
def test_launch_cuts_and_shards(ni, key, n_out, K, Tm):
    """One launch of T steps equals two launches of 3 + 4 from the same launch counter; two shards by env_index0 equal the
    unsharded run; B = 5 equals the first five lanes of B = 700: bit for bit in every output and in the final state."""
    one = _mixed(ni, key, n_out, K, Tm, 700, True, 0, 37)
    two = _mixed(ni, key, n_out, K, Tm, 700, True, 0, 37, (3, T - 3))
    assert one["shielded"].any() and not one["shielded"][one["live"]].all()
    _same(one, two, "one launch vs two", cut=True)
    whole = _mixed(ni, key, n_out, K, Tm, 700, False)
    lo, hi = _mixed(ni, key, n_out, K, Tm, 350, False, 0), _mixed(ni, key, n_out, K, Tm, 350, False, 350)
    _same(whole, lo, "shard 0", lanes=slice(0, 350))
    for k in OUT:
        a = whole[k][..., 350:] if k in ("prob", "unc", "logit") else whole[k][:, 350:]
        assert np.array_equal(_bits(a), _bits(hi[k])), ("shard 1", k)
    assert np.array_equal(_bits(whole["state"][350:]), _bits(hi["state"])) and np.array_equal(whole["ctr"][350:], hi["ctr"])
    _same(whole, _mixed(ni, key, n_out, K, Tm, 5, False), "B = 700 vs B = 5", lanes=slice(0, 5))


# ---- 9: a 128-wide member ------------------------------------------------------------------------------------------------------
def test_128_wide_members_run_through_the_padding_helper(ni, oracle):
    """The reference's SafetyEnsembleMember width: on pad_safety_member's 256-wide networks the device's logits are, through the
    sigmoid, bit for bit oracle.mlp_critic on the PADDED columns, and within 1e-5 (floor 1e-6) of a float64 host network on the
    UNPADDED weights."""
    from neorl_industrial_gym_amd.policies import pad_safety_member
    key, n_out, h = "cr", 3, 128
    ws, ms, S, A, _ = _nets(ni, key, n_out)
    rng = np.random.default_rng(91)
    narrow = [[(m[0][0][:, :h].copy(), m[0][1][:h].copy()), (rng.normal(0, 1.0 / np.sqrt(h), (h, h)).astype(f32), rng.normal(0, 0.05, h).astype(f32)),
               (rng.normal(0, HEAD_STD * 2, (h, n_out)).astype(f32), rng.normal(0, 0.1, n_out).astype(f32))] for m in ms[:2]]
    padded = [pad_safety_member(m) for m in narrow]
    o = _run(ni, NAMES[key], True, ws, padded, 1.0, 2.0, BIG, 700)
    assert o["live"].all() and len(np.unique(o["logit"][0, 0, 0])) > 100
    x = np.concatenate([o["obs"], o["act"]], axis=-1).astype(np.float64)
    for m in range(2):
        z = x
        for i, (W, b) in enumerate(narrow[m]):
            z = z @ W.astype(np.float64) + b.astype(np.float64)
            if i < 2:
                z = np.maximum(z, 0)
        got = o["logit"][:, m].transpose(0, 2, 1).astype(np.float64)          # [n, B, C]
        assert (np.abs(got - z) <= np.maximum(1e-6, 1e-5 * np.abs(z))).all(), m
    for k in (0, T - 1):
        for m in range(2):
            for c in range(n_out):
                want = oracle.mlp_critic(key, _column(padded[m], c), o["obs"][k], o["act"][k])
                assert np.array_equal(_bits(oracle.detmath_unary("sigmoidf", o["logit"][k, m, c])), _bits(want)), (k, m, c)


# ---- 10: refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(ni):
    L, lib = ni._lib, ni._lib.lib()
    key, n_out, K = "cr", 3, 2
    ws, ms, S, A, _ = _nets(ni, key, n_out)
    B, n = 200, 3
    INVALID, UNSUPPORTED = 1, 4           # NIG_ERR_INVALID, NIG_ERR_UNSUPPORTED
    assert lib.nig_rollout_mlp_gated(None, n, None, None, 0, None, 0, None, 0, 0, None, None, None, 0, 0, None) == INVALID

    def install(env, members, hidden=256, Cn=None, Tm=1.0, thr=0.5, umax=0.2, K_=None, null=None):
        W = [[np.ascontiguousarray(x, dtype=f32) for pair in m for x in pair] for m in members]
        Kn = len(members) if K_ is None else K_
        cols = [(C.c_void_p * max(len(W), 1))(*[w[j].ctypes.data for w in W]) for j in range(6)]
        if null == "array":
            cols[4] = None
        if null == "member":
            cols[2][len(W) - 1] = None
        return lib.nig_set_mlp_safety_ensemble(env._h, Kn, hidden, n_out if Cn is None else Cn, *cols, Tm, thr, umax, env._stream())

    def attempt(env, want, what, ld_c=None, c_step=None, n_steps=n, out_stride=None, ld_act=None):
        ld = env.ld
        bufs = dict(rw=torch.full((n, ld), 7.5, device=env.device), fl=torch.full((n, ld), 0x5A5A5A5B, dtype=torch.int32, device=env.device),
                    obs=torch.full((n, B, S), 7.5, device=env.device), act=torch.full((n, A, ld), 7.5, device=env.device),
                    pr=torch.full((n, n_out, ld), 7.5, device=env.device), un=torch.full((n, n_out, ld), 7.5, device=env.device),
                    lg=torch.full((n, KMAX, n_out, ld), 7.5, device=env.device))
        before = {k: v.clone() for k, v in bufs.items()}
        state, ctr, t = env.get_state().clone(), env.ctr.clone(), env.counter
        p = lambda x: C.c_void_p(x.data_ptr())
        rc = lib.nig_rollout_mlp_gated(env._h, n_steps, p(bufs["rw"]), p(bufs["fl"]), ld if out_stride is None else out_stride, p(bufs["obs"]), B * S,
                                       p(bufs["act"]), ld if ld_act is None else ld_act, A * ld, p(bufs["pr"]), p(bufs["un"]), p(bufs["lg"]),
                                       ld if ld_c is None else ld_c, n_out * ld if c_step is None else c_step, env._stream())
        torch.cuda.synchronize()
        assert rc == want, (what, rc, lib.nig_last_error())
        if want != 0:
            for k in bufs:
                assert torch.equal(bufs[k], before[k]), (what, k)
            assert torch.equal(env.get_state(), state) and torch.equal(env.ctr, ctr) and env.counter == t, what

    env = ni.make_batched(NAMES[key], B, max_episode_steps=MAXS)
    env.reset()
    attempt(env, INVALID, "neither actor nor members")
    env.set_mlp_policy(ws)
    attempt(env, INVALID, "no members installed")
    with pytest.raises(L.NigError):
        env.rollout_mlp_gated(n)
    # refused installations leave "no members installed"
    for rc, what, kw in [(INVALID, "K = 0", dict(K_=0)), (INVALID, "K = NIG_MAX_ENSEMBLE + 1", dict(K_=L.MAX_ENSEMBLE + 1)), (INVALID, "K = -1", dict(K_=-1)),
                         (INVALID, "C = 0", dict(Cn=0)), (INVALID, "C = 5", dict(Cn=5)), (INVALID, "a NULL array", dict(null="array")),
                         (INVALID, "a NULL member pointer", dict(null="member")), (INVALID, "T = 0", dict(Tm=0.0)), (INVALID, "T < 0", dict(Tm=-1.0)),
                         (INVALID, "T = inf", dict(Tm=float("inf"))), (INVALID, "T = NaN", dict(Tm=float("nan"))),
                         (INVALID, "NaN probability limit", dict(thr=float("nan"))), (INVALID, "NaN spread limit", dict(umax=float("nan"))),
                         (UNSUPPORTED, "hidden 128", dict(hidden=128))]:
        assert install(env, ms[:K], **kw) == rc, (what, lib.nig_last_error())
        attempt(env, INVALID, what + ": still no members")
    with pytest.raises(L.NigError):
        env.set_mlp_safety_ensemble([], 1.0, 0.5, 0.2)
    assert install(env, ms[:K]) == 0
    env.set_mlp_safety_ensemble(ms[:K], 1.0, 0.5, 0.2)
    attempt(env, INVALID, "ld_c < B", ld_c=B - 1)
    attempt(env, INVALID, "c_step_stride < C * ld_c", c_step=n_out * env.ld - 1)
    attempt(env, INVALID, "n_steps 0", n_steps=0)
    attempt(env, INVALID, "out_stride < B", out_stride=B - 1)
    attempt(env, INVALID, "ld_act < B", ld_act=B - 1)
    # a refused installation keeps the installed members; the largest ensemble and the widest head install and run
    assert install(env, ms[:K], Tm=0.0) == INVALID
    attempt(env, 0, "the installed gate runs")
    env.set_mlp_safety_ensemble(_nets(ni, key, 4)[1][:KMAX], 1.0, 0.5, 0.2)
    env.rollout_mlp_gated(n)
    torch.cuda.synchronize()
    env.close()
    # members without an actor
    env = ni.make_batched(NAMES[key], B, max_episode_steps=MAXS)
    env.reset()
    env.set_mlp_safety_ensemble(ms[:K], 1.0, 0.5, 0.2)
    attempt(env, INVALID, "no actor installed")
    env.close()
    # an env shape without the MFMA actor (S = 15)
    water = ni.make_batched("WaterTreatment-v0", 64)
    water.reset()
    Sw, Aw = water.state_dim, water.action_dim
    assert install(water, [_random_member(Sw, Aw, n_out, 5)]) == UNSUPPORTED
    assert lib.nig_rollout_mlp_gated(water._h, n, None, None, 0, None, 0, None, 0, 0, None, None, None, 0, 0, water._stream()) == UNSUPPORTED
    water.close()


# ---- 11: footprint -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pitch", ["B", "B + odd", "beyond ld"])
def test_footprint_of_the_gate_outputs(ni, pitch):
    """prob_out, unc_out and logit_out beside act / obs / reward / flags in canary arenas, lanes freezing inside the launch (no
    auto-reset, episodes of at most 5 steps): no pad column, stride gap, row >= C of a block, frozen-lane or red-zone word changes
    and every documented word is written.  The step stride leaves room for a fourth row, which C = 3 must not touch."""
    key, n_out, K, B = "pg", 3, 5, 200
    ws, ms, S, A, _ = _nets(ni, key, n_out)
    env = ni.make_batched(NAMES[key], B, seed=SEED, autoreset=False, tally=True, max_episode_steps=MAXS)
    env.set_mlp_policy(ws)
    thr, umax = _medians(_accept_all(ni, key, n_out, K, 1.0))
    env.set_mlp_safety_ensemble(ms[:K], 1.0, thr, umax)
    ld, lda, ostep = B + 3, B + 5, (B * S + 3) // 4 * 4 + 8
    ld_c = {"B": B, "B + odd": B + 7, "beyond ld": env.ld + 65}[pitch]
    c_step = 4 * ld_c + 5
    a = Arena("cuda")
    rew = a.add("reward_out", "f32", Layout(T, ld, 1, ld, B))
    fl = a.add("flags_out", "flags", Layout(T, ld, 1, ld, B))
    pr = a.add("prob_out", "f32", Layout(T, c_step, n_out, ld_c, B))
    un = a.add("unc_out", "f32", Layout(T, c_step, n_out, ld_c, B))
    lg = a.add("logit_out", "f32", Layout(T * K, c_step, n_out, ld_c, B))
    obs = a.add("obs_out", "f32", Layout(T, ostep, 1, B * S, B * S, lane_width=S), align=16)
    act = a.add("act_out", "f32", Layout(T, A * lda + 7, A, lda, B))
    a.build()
    env.reset()
    p = lambda b: C.c_void_p(b.ptr)
    rc = ni._lib.lib().nig_rollout_mlp_gated(env._h, T, p(rew), p(fl), ld, p(obs), ostep, p(act), lda, A * lda + 7, p(pr), p(un), p(lg), ld_c, c_step,
                                             env._stream())
    assert rc == 0, ni._lib.lib().nig_last_error()
    torch.cuda.synchronize()
    f = fl.rows(T)[:, 0]
    live = (f & ni._lib.FLAG_INACTIVE) == 0
    assert bool(live[0].all()) and not bool(live[-1].any())
    assert bool((f & ni._lib.FLAG_SHIELDED)[live].bool().any()) and bool((f & ni._lib.FLAG_UNCERTAIN)[live].bool().any())
    written = {b.name: dict(n_outer=T, live=live if b in (pr, un, obs, act) else None) for b in (rew, fl, pr, un, obs, act)}
    written[lg.name] = dict(n_outer=T * K, live=live.repeat_interleave(K, dim=0))
    findings = [str(x) for x in a.check(written)]
    assert not findings, "\n  ".join(findings)
    env.close()


# ---- 12: evaluate_with_safety ---------------------------------------------------------------------------------------------------
def test_evaluate_with_safety_runs_the_fused_gate(ni, monkeypatch):
    """evaluate_with_safety(SafetyEnsemblePolicy, env) reaches rollout_mlp_gated without a host step or predict.  At limits nothing
    reaches, its 13 metrics are the plain actor's, value for value; at the median limits they are those reduced from the reward /
    flag rows of the same rollout on a second handle (returns: the float64 mean of 256 terms, to reassociation error)."""
    from neorl_industrial_gym_amd.episodes import episodes_from_rows
    key, n_out, K, n_ep = "cr", 3, 5, 256
    ws, ms, S, A, _ = _nets(ni, key, n_out)
    L = ni._lib
    mk = lambda: ni.make_batched(NAMES[key], n_ep, autoreset=False, tally=True, max_episode_steps=24)
    a, b = mk(), mk()
    want = ni.evaluate_with_safety(ni.MLPPolicy(ws), b, n_episodes=n_ep)
    sp = ni.SafetyEnsemblePolicy(ws, ms[:K], temperature=1.0, threshold=2.0, max_uncertainty=BIG)
    assert sp.fusable

    def boom(*_a, **_k):
        raise AssertionError("the fused gate must not step or predict on the host")
    monkeypatch.setattr(a, "step", boom)
    monkeypatch.setattr(sp, "predict", boom)
    monkeypatch.setattr(sp, "predict_device", boom)
    calls = []
    real = a.rollout_mlp_gated
    monkeypatch.setattr(a, "rollout_mlp_gated", lambda *x, **k: (calls.append(x), real(*x, **k)))
    got = ni.evaluate_with_safety(sp, a, n_episodes=n_ep)
    assert calls
    assert len(got) == 13 and set(got) == set(want)
    for k in want:
        assert got[k] == want[k], k
    a.close(); b.close()
    # the median limits: both outcomes occur, and the metrics are those of the rows
    thr, umax = _medians(_accept_all(ni, key, n_out, K, 1.0))
    sp = ni.SafetyEnsemblePolicy(ws, ms[:K], temperature=1.0, threshold=thr, max_uncertainty=umax)
    a, b = mk(), mk()
    got = ni.evaluate_with_safety(sp, a, n_episodes=n_ep)
    sp.install(b)
    b.ctr.fill_(L.CTR_DONE)
    b.reset(mask=torch.ones(n_ep, dtype=torch.uint8, device=b.device))
    rw = torch.zeros(24, b.ld, dtype=torch.float32, device=b.device)
    fl = torch.zeros(24, b.ld, dtype=torch.int32, device=b.device)
    b.rollout_mlp_gated(24, rw, fl)
    torch.cuda.synchronize()
    rw, fl = rw[:, :n_ep].cpu().numpy(), fl[:, :n_ep].cpu().numpy()
    live = (fl & L.FLAG_INACTIVE) == 0
    sh = ((fl & L.FLAG_SHIELDED) != 0)[live]
    assert sh.any() and not sh.all()
    rec = episodes_from_rows(rw, fl, bool(b.spec.reward_is_f32), 1)
    assert (rec["count"] == 1).all()
    ret, w0 = rec["ret"][0], rec["w"][0, 0]
    lens, viol = (w0 & L.CTR_STEP_MASK).astype(np.int64), (w0 >> L.CTR_VIOL_SHIFT).astype(np.int64)
    assert np.array_equal(lens, live.sum(axis=0))
    assert got["length_mean"] == np.mean(lens) and got["safety_violations"] == viol.sum()
    assert got["return_min"] == ret.min() and got["return_max"] == ret.max()
    assert got["successful_episodes"] == int((ret > 0).sum())
    assert abs(got["return_mean"] - np.mean(ret)) <= n_ep * 2.0 ** -52 * np.abs(ret).sum() / n_ep
    a.close(); b.close()
