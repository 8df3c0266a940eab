"""-m gpu: the fused safe-action search (nig_rollout_mlp_search, BatchedIndustrialEnv.rollout_mlp_search; "nig-search-v1" in
include/nig.h) -- the safety-critical agents' get_safe_action (agents/safety_critical.py:173-208) in the MFMA actor kernel --
against the law restated on the host: the CPU oracle's actor, critic and env step, and policies.search_candidates' draws.

Shapes are small on purpose: T steps with max_episode_steps 5 (lanes freeze or reset inside the launch), B = 700 (five full
128-env blocks and a partial one) and B = 5 (one partial wave); the host restatement costs T * B * N oracle critic passes."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import closed_loop_matrix as M
from footprint import Arena, Layout

pytestmark = pytest.mark.gpu

# ChemicalReactor: A = 3, 4x4x1 head, one-chunk critic layer 1; PowerGrid: A = 8, 16x16x1 head, two-chunk critic layer 1;
# RobotAssembly: A = 7, a candidate spans two generator blocks with an unused word; HVACControl: a build-specified plant;
# SteelAnnealing and AdvancedChemicalReactor: A = 6, an even one-chunk critic layer 1 (width 26, no zero-padded k-step);
# SupplyChain: A = 10, head rows 8 and 9 from the third source-lane group, a candidate spans three generator blocks, critic
# width 38 (two chunks, 20 records, no padding record); AdvancedPowerGrid: PowerGrid's shapes.  The two Advanced envs draw
# nothing, so their lanes start from closed_loop_matrix.start_states (from reset() they would all be clones).
ENVS = M.MFMA_ENVS                                 # every env the family is compiled for (tests/closed_loop_matrix.py)
T, MAXS, SEED = 7, 5, 0x5EED
SHAPES = [(700, 5), (5, 1)]                        # (B, n_candidates)
f32 = np.float32


@pytest.fixture(scope="module")
def ni():
    import neorl_industrial_gym_amd as ni
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return ni


def _random_actor(S, A, seed):       # the style of test_gpu_safety_shield.py
    rng = np.random.default_rng(seed)
    return [(rng.normal(0, 1.0 / np.sqrt(S), (S, 256)).astype(f32) * f32(0.05), rng.normal(0, 0.05, 256).astype(f32)),
            (rng.normal(0, 1.0 / 16, (256, 256)).astype(f32), rng.normal(0, 0.05, 256).astype(f32)),
            (rng.normal(0, 1.0 / 8, (256, A)).astype(f32), rng.normal(0, 0.1, A).astype(f32))]


def _random_critic(S, A, seed, h=256):
    rng = np.random.default_rng(seed)
    D = S + A
    return [(rng.normal(0, 1.0 / np.sqrt(D), (D, h)).astype(f32) * f32(0.05), rng.normal(0, 0.05, h).astype(f32)),
            (rng.normal(0, 1.0 / np.sqrt(h), (h, h)).astype(f32), rng.normal(0, 0.05, h).astype(f32)),
            (rng.normal(0, 1.0 / 2, (h, 1)).astype(f32), rng.normal(0, 0.1, 1).astype(f32))]


OUT = ("act", "obs", "reward", "flags", "prob", "risk", "choice")


def _run(ni, name, autoreset, ws, cw, thr, N, B, entry="search", env_index0=0, t0=0, cuts=(T,)):
    """One rollout of sum(cuts) steps, cut into len(cuts) launches, through rollout_mlp_search (or rollout_mlp_safe: its
    risk / choice rows stay zero).  Returns (env, outputs as host arrays + the launch counter of step 0's noise - 1)."""
    env = ni.make_batched(name, B, seed=SEED, env_index0=env_index0, autoreset=autoreset, tally=True, max_episode_steps=MAXS)
    env.set_mlp_policy(ws)
    env.set_mlp_safety(cw, thr)
    dev, n = env.device, sum(cuts)
    act = torch.zeros(n, env.action_dim, env.ld, dtype=torch.float32, device=dev)
    # (an observation step is a multiple of 4 floats: where B * S is none, the rows are padded and the C entry points are called
    # directly -- the Python methods take contiguous [n, B, S] tensors)
    S, ostep = env.state_dim, (B * env.state_dim + 3) // 4 * 4
    obs = torch.zeros(n, ostep, dtype=torch.float32, device=dev)
    p = lambda x: C.c_void_p(x.data_ptr())
    fl = torch.zeros(n, env.ld, dtype=torch.int32, device=dev)
    rw, pr, rk = (torch.zeros(n, env.ld, dtype=torch.float32, device=dev) for _ in range(3))
    ch = torch.zeros(n, env.ld, dtype=torch.int32, device=dev)
    env.counter = t0
    env.reset()
    assert env_index0 == 0 or M.KEY_OF[name] not in M.CLONED
    M.install_start(ni, env, M.KEY_OF[name], SEED)
    k = 0
    for m in cuts:
        s = slice(k, k + m)
        if ostep != B * S:
            common = (p(rw[s]), p(fl[s]), env.ld, p(obs[s]), ostep, p(act[s]), env.ld, env.action_dim * env.ld, p(pr[s]))
            L = ni._lib.lib()
            with torch.cuda.device(dev):
                ni._lib.check(L.nig_rollout_mlp_search(env._h, m, N, *common, p(rk[s]), p(ch[s]), env._stream()) if entry == "search"
                              else L.nig_rollout_mlp_safe(env._h, m, *common, env._stream()))
        elif entry == "search":
            env.rollout_mlp_search(m, N, rw[s], fl[s], obs[s].view(m, B, S), act[s], pr[s], rk[s], ch[s])
        else:
            env.rollout_mlp_safe(m, rw[s], fl[s], obs[s].view(m, B, S), act[s], pr[s])
        k += m
    torch.cuda.synchronize()
    assert env.counter == t0 + n
    o = dict(act=act[:, :, :B].permute(0, 2, 1).cpu().numpy(), obs=obs[:, :B * S].reshape(n, B, S).cpu().numpy(), flags=fl[:, :B].cpu().numpy(),
             reward=rw[:, :B].cpu().numpy(), prob=pr[:, :B].cpu().numpy(), risk=rk[:, :B].cpu().numpy(), choice=ch[:, :B].cpu().numpy())
    o["live"] = (o["flags"] & ni._lib.FLAG_INACTIVE) == 0
    o["shielded"] = (o["flags"] & ni._lib.FLAG_SHIELDED) != 0
    o["state"] = env.get_state().cpu().numpy()
    o["ctr"] = env.ctr.cpu().numpy()
    o["tally"] = env.tally.cpu().numpy()
    o["t0"], o["env0"] = t0, env_index0
    return env, o


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32) if x.dtype == np.float32 else (np.ascontiguousarray(x).view(np.uint64) if x.dtype == np.float64 else x)


def _same(a, b, what, lanes=slice(None), cut=False):
    """Every output, the final state, the counters and the tallies, bit for bit, on `lanes` of both runs.  cut: the runs cut
    their launches differently.  A launch sums the returns (and their squares) of the episodes it finishes in registers and adds
    the sum to the handle's tally at its end -- every closed-loop kernel does -- so two cuts associate those two float64 sums
    differently where a lane finishes several episodes: for them the bound is that of reassociating n terms, n * 2^-52 * sum |term|
    (the squares: their sum itself; the returns: sum |r| <= sqrt(n * sum r^2)); every other row stays exact."""
    for k in OUT:
        assert np.array_equal(_bits(a[k][:, lanes]), _bits(b[k][:, lanes])), (what, k)
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
def _nets(ni, key, name):
    """A random actor and a random critic whose state inputs are scaled by the observed magnitudes, so that p spreads over the
    lanes and over the candidates (test_gpu_safety_shield.py's construction: state columns of the order of 100 saturate the
    unscaled critic at p == 1.0); and the never-search run at B = 700 they were scaled on."""
    probe = ni.make_batched(name, 1)
    S, A = probe.state_dim, probe.action_dim
    probe.close()
    ws, cw = M.matrix_actor(ni, key, _random_actor(S, A, 31), SEED), _random_critic(S, A, 32)
    env, o = _run(ni, name, True, ws, cw, 2.0, 1, 700, entry="safe")
    env.close()
    sc = (1.0 / (1.0 + np.abs(o["obs"][o["live"]]).mean(axis=0))).astype(f32)
    cw = [(np.concatenate([cw[0][0][:S] * f32(20.0) * sc[:, None], cw[0][0][S:] * f32(20.0)]).astype(f32), cw[0][1]), cw[1], cw[2]]
    return ws, cw, S, A


def _first_min(p):
    """The law's choice over p [n, N]: c = 0, then every c with p_c < p_best in order; a NaN gives way to the first number."""
    best = np.zeros(p.shape[0], dtype=np.int64)
    pb = p[:, 0].copy()
    for c in range(1, p.shape[1]):
        with np.errstate(invalid="ignore"):
            take = (p[:, c] < pb) | (np.isnan(pb) & ~np.isnan(p[:, c]))
        pb = np.where(take, p[:, c], pb)
        best = np.where(take, c, best)
    return best, pb


def _check_law(ni, oracle, key, o, ws, cw, thr, N, candidates_only=False):
    """Every live step of the run against "nig-search-v1" restated on the host from the recorded observations.  Returns the
    per-step masks of searched lanes."""
    from neorl_industrial_gym_amd.policies import search_candidates
    live, B = o["live"], o["obs"].shape[1]
    thr = f32(thr)
    searched = np.zeros_like(live)
    for k in range(o["obs"].shape[0]):
        lv = live[k]
        raw = oracle.mlp_actions(key, ws, o["obs"][k])
        p0 = oracle.mlp_critic(key, cw, o["obs"][k], raw)
        assert np.array_equal(_bits(o["prob"][k])[lv], _bits(p0)[lv]), (k, "prob")
        if k == 0 and key in M.FLOAT64_KEYS:       # the shapes only these envs bring, against the networks in NumPy float64
            raw64 = M.actor64(ws, o["obs"][0])
            assert M.worst(f"{key} B={B}: the actor's action of step 0 against float64", raw, raw64, M.ACT_ATOL) <= 1.0
            assert M.worst(f"{key} B={B}: prob of step 0 against float64", o["prob"][0], M.critic64(cw, o["obs"][0], raw64), M.PROB_ATOL) <= 1.0
            if not candidates_only:
                assert M.worst(f"{key} B={B}: risk of step 0 against float64", o["risk"][0], M.critic64(cw, o["obs"][0], o["act"][0]), M.PROB_ATOL) <= 1.0
        with np.errstate(invalid="ignore"):
            want = lv & ~(p0 < thr)
        searched[k] = want
        keep = lv & ~want
        assert np.array_equal(_bits(o["act"][k])[keep], _bits(raw)[keep]), (k, "kept action")
        assert np.array_equal(_bits(o["risk"][k])[keep], _bits(p0)[keep]) and (o["choice"][k][keep] == -1).all(), (k, "kept risk / choice")
        idx = np.nonzero(want)[0]
        if idx.size == 0:
            continue
        cand = np.stack([search_candidates(SEED, o["env0"] + int(i), o["t0"] + k + 1, N, raw.shape[1]) for i in idx])     # [n, N, A]
        if candidates_only:
            best, pb = np.zeros(idx.size, dtype=np.int64), None
        else:
            pc = oracle.mlp_critic(key, cw, np.repeat(o["obs"][k][idx], N, axis=0), cand.reshape(idx.size * N, -1)).reshape(idx.size, N)
            best, pb = _first_min(pc)
            assert np.array_equal(_bits(o["risk"][k][idx]), _bits(pb.astype(f32))), (k, "risk")
        assert np.array_equal(o["choice"][k][idx], best), (k, "choice")
        assert np.array_equal(_bits(o["act"][k][idx]), _bits(cand[np.arange(idx.size), best])), (k, "searched action")
    assert np.array_equal(o["shielded"], searched), "FLAG_SHIELDED on exactly the searched live steps"
    return searched


# ---- 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N", SHAPES)
@pytest.mark.parametrize("autoreset", [False, True])
@pytest.mark.parametrize("key,name", ENVS)
def test_never_search_is_the_shield_kernel_at_the_same_threshold(ni, key, name, autoreset, B, N):
    """Threshold 2.0 (p < 2 always): act, obs, reward, flags, prob, final state, counters and tallies bit for bit
    rollout_mlp_safe's; choice == -1 on live steps and risk bit-equal to prob (frozen lanes: the words stay as they were)."""
    ws, cw, S, A = _nets(ni, key, name)
    env, o = _run(ni, name, autoreset, ws, cw, 2.0, N, B)
    env.close()
    env, r = _run(ni, name, autoreset, ws, cw, 2.0, N, B, entry="safe")
    env.close()
    live = o["live"]
    assert live[0].all() and (autoreset or not live[-1].any())          # (lanes freeze inside the launch without auto-reset)
    assert (o["choice"][live] == -1).all() and (o["choice"][~live] == 0).all()
    assert np.array_equal(_bits(o["risk"]), _bits(o["prob"]))
    assert not o["shielded"].any()
    r["risk"], r["choice"] = o["risk"], o["choice"]                     # (rollout_mlp_safe has neither)
    _same(o, r, "search at 2.0 vs shield at 2.0")


# ---- 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,autoreset", [(700, 5, True), (700, 1, False), (5, 1, False), (5, 5, True)])
@pytest.mark.parametrize("key,name", ENVS)
def test_always_search_takes_the_first_least_risky_candidate(ni, oracle, key, name, B, N, autoreset):
    """Threshold 0.0 (p is never below 0): on every live step act is search_candidates(...)[best] bit for bit, best the first
    minimum of oracle.mlp_critic over the candidates on the recorded observation; choice == best; risk the oracle's p_best
    and prob the oracle's p0, bit for bit; FLAG_SHIELDED on exactly the live steps; the next observation is the oracle's env
    step on that action."""
    ws, cw, S, A = _nets(ni, key, name)
    env, o = _run(ni, name, autoreset, ws, cw, 0.0, N, B)
    env.close()
    live, L = o["live"], ni._lib
    searched = _check_law(ni, oracle, key, o, ws, cw, 0.0, N)
    assert np.array_equal(searched, live) and np.array_equal(o["shielded"], live)
    if N > 1 and B > 100:
        assert len(np.unique(o["choice"][live])) == N                   # (the critic tells the candidates apart: every c wins somewhere)
    # teacher-forced env step: obs[k+1] = step(obs[k], act[k]) where the lane neither finished nor reset
    n, checked = min(B, 400), 0
    for k in range(T - 1):
        fl = o["flags"][k, :n]
        step_after = (fl.astype(np.uint32) >> L.FLAG_STEP_SHIFT).astype(np.int32)
        nz = np.stack([oracle.gen_step_noise(key, SEED, i, k + 1) for i in range(n)]) if oracle.spec(key).k_step else None
        r = oracle.step(key, o["obs"][k, :n], o["act"][k, :n], nz, step_after - 1, max_steps=MAXS, flavor=oracle.MATH_POLY)
        cont = live[k, :n] & live[k + 1, :n] & ((fl & (L.FLAG_TERMINATED | L.FLAG_TRUNCATED | L.FLAG_DID_RESET)) == 0)
        checked += int(cont.sum())
        assert np.array_equal(_bits(o["obs"][k + 1, :n][cont]), _bits(r["state_next"][cont])), k
    if key == "apg":
        # the plant: an AdvancedPowerGrid episode ends whenever a[4] or a[5] is below 0.95, which a uniform candidate of [-1, 1)
        # almost always is, so (almost) no searched lane continues.  What holds instead: every live step's TERMINATED bit is the
        # oracle's on that candidate, and step 0 -- the only step whose lanes are distinct -- is checked above lane by lane
        M.check_env_steps(oracle, L, key, o["obs"], o["act"], o["flags"], SEED, MAXS)
        assert ((o["flags"][0] & L.FLAG_TERMINATED) != 0).mean() > 0.9
    else:
        assert checked > 0                                              # (the loop compared something)
    if B > 100 and key in M.CLONED:
        assert M.distinct_rows(oracle.mlp_actions(key, ws, o["obs"][0])) >= 600, "step 0: the lanes are no clones of each other"


# ---- 3 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,name", ENVS[:2])
def test_equal_risks_take_candidate_zero(ni, oracle, key, name):
    """A critic with C3 = 0 gives every candidate p = sigmoid(c3): at threshold 0 the first-minimum rule must choose c = 0
    everywhere, and the action is candidate 0."""
    ws, cw, S, A = _nets(ni, key, name)
    flat = [cw[0], cw[1], (np.zeros_like(cw[2][0]), cw[2][1])]
    env, o = _run(ni, name, True, ws, flat, 0.0, 5, 700)
    env.close()
    live = o["live"]
    assert live.all() and (o["choice"] == 0).all()
    assert len(np.unique(_bits(o["risk"]))) == 1 and np.array_equal(_bits(o["risk"]), _bits(o["prob"]))
    _check_law(ni, oracle, key, o, ws, flat, 0.0, 5, candidates_only=True)


# ---- 4, 5, 6 ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _median_threshold(ni, key, name):
    """The median of step 0's p over the 700 lanes of the never-search run (test 1's): lanes on both sides of it."""
    ws, cw, S, A = _nets(ni, key, name)
    env, o = _run(ni, name, True, ws, cw, 2.0, 1, 700)
    env.close()
    p = o["prob"][0]
    assert len(np.unique(p)) > 350, "the critic does not spread p over the lanes"
    return float(np.median(p))


@pytest.mark.parametrize("autoreset", [False, True])
@pytest.mark.parametrize("key,name", ENVS)
def test_mixed_lanes_keep_or_search_per_lane(ni, oracle, key, name, autoreset):
    """A threshold at the median of step 0's p: both classes occur on step 0; kept lanes carry the actor's action (risk == p0,
    choice -1, no flag), searched lanes the law of the always-search test, lane by lane."""
    ws, cw, S, A = _nets(ni, key, name)
    thr = _median_threshold(ni, key, name)
    env, o = _run(ni, name, autoreset, ws, cw, thr, 5, 700)
    env.close()
    searched = _check_law(ni, oracle, key, o, ws, cw, thr, 5)
    assert searched[0].any() and (o["live"][0] & ~searched[0]).any()
    with np.errstate(invalid="ignore"):
        assert np.array_equal(o["shielded"][o["live"]], ~(o["prob"][o["live"]] < f32(thr)))


@pytest.mark.parametrize("spread", ["median", "sparse"])
@pytest.mark.parametrize("key,name", ENVS[:2])
def test_a_lane_does_not_depend_on_its_neighbours(ni, key, name, spread):
    """Lanes [0, 100) of the B = 700 run equal a B = 100 env with the same seed and env_index0, bit for bit in every output:
    at the mixed threshold, and at one only a lane in two hundred exceeds on step 0 -- so the runs differ in which lanes share
    a block, and block-steps with and without candidate passes both occur."""
    ws, cw, S, A = _nets(ni, key, name)
    thr = _median_threshold(ni, key, name)
    if spread == "sparse":
        env, o = _run(ni, name, False, ws, cw, 2.0, 1, 700)
        env.close()
        thr = float(np.sort(o["prob"][0])[-4])
    env, big = _run(ni, name, False, ws, cw, thr, 5, 700)
    env.close()
    env, small = _run(ni, name, False, ws, cw, thr, 5, 100)
    env.close()
    sh, live = big["shielded"], big["live"]
    assert sh.any() and (live & ~sh).any()
    block_steps = np.stack([sh[:, b:b + 128].any(axis=1) for b in range(0, 700, 128)], axis=1)[live.any(axis=1)]
    assert block_steps.any() and (spread == "median" or not block_steps.all())
    _same(big, small, "B = 700 vs B = 100", lanes=slice(0, 100))


@pytest.mark.parametrize("key,name", [ENVS[0], ENVS[2]])
def test_launch_cuts(ni, key, name):
    """One launch of T steps equals two launches of T1 + T2 from the same launch counter, in every output and final state."""
    ws, cw, S, A = _nets(ni, key, name)
    thr = _median_threshold(ni, key, name)
    env, one = _run(ni, name, True, ws, cw, thr, 5, 700, t0=37)
    env.close()
    env, two = _run(ni, name, True, ws, cw, thr, 5, 700, t0=37, cuts=(3, T - 3))
    env.close()
    assert one["shielded"].any() and not one["shielded"][one["live"]].all()
    _same(one, two, "one launch vs two", cut=True)


# ---- 7 ---------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(ni):
    L, lib = ni._lib, ni._lib.lib()
    ws, cw, S, A = _nets(ni, "cr", "ChemicalReactor-v0")
    B, n = 200, 3

    def attempt(env, N, what):
        bufs = dict(rw=torch.full((n, env.ld), 7.5, device=env.device), fl=torch.full((n, env.ld), 0x5A5A5A5B, dtype=torch.int32, device=env.device),
                    obs=torch.full((n, B, S), 7.5, device=env.device), act=torch.full((n, A, env.ld), 7.5, device=env.device),
                    pr=torch.full((n, env.ld), 7.5, device=env.device), rk=torch.full((n, env.ld), 7.5, device=env.device),
                    ch=torch.full((n, env.ld), 0x5A5A5A5B, dtype=torch.int32, device=env.device))
        before = {k: v.clone() for k, v in bufs.items()}
        state, ctr, t = env.get_state().clone(), env.ctr.clone(), env.counter
        p = lambda x: C.c_void_p(x.data_ptr())
        rc = lib.nig_rollout_mlp_search(env._h, n, N, p(bufs["rw"]), p(bufs["fl"]), env.ld, p(bufs["obs"]), B * S, p(bufs["act"]), env.ld,
                                        A * env.ld, p(bufs["pr"]), p(bufs["rk"]), p(bufs["ch"]), env._stream())
        torch.cuda.synchronize()
        assert rc == 1, (what, rc)                                      # NIG_ERR_INVALID
        for k in bufs:
            assert torch.equal(bufs[k], before[k]), (what, k)
        assert torch.equal(env.get_state(), state) and torch.equal(env.ctr, ctr) and env.counter == t, what
    env = ni.make_batched("ChemicalReactor-v0", B, max_episode_steps=MAXS)
    env.reset()
    env.set_mlp_policy(ws)
    attempt(env, 5, "no critic installed")
    with pytest.raises(L.NigError):
        env.rollout_mlp_search(n, 5)
    env.set_mlp_safety(cw, 0.0)
    attempt(env, 0, "n_candidates 0")
    attempt(env, L.MAX_CANDIDATES + 1, "n_candidates NIG_MAX_CANDIDATES + 1")
    attempt(env, -1, "n_candidates -1")
    env.rollout_mlp_search(n, L.MAX_CANDIDATES)                         # the largest search runs
    torch.cuda.synchronize()
    env.close()
    env = ni.make_batched("ChemicalReactor-v0", B, max_episode_steps=MAXS)
    env.reset()
    env.set_mlp_safety(cw, 0.0)
    attempt(env, 5, "no actor installed")
    env.close()


# ---- 8 ---------------------------------------------------------------------------------------------------------------------
def test_footprint_of_the_row_outputs(ni):
    """prob_out, risk_out and choice_out beside act / obs / reward / flags in canary arenas, pitch > B, lanes freezing inside
    the launch (no auto-reset, episodes of at most 5 steps): no pad column, stride gap, frozen-lane or red-zone word changes
    and every documented word is written."""
    name, B = "PowerGrid-v0", 200
    ws, cw, S, A = _nets(ni, "pg", name)
    env = ni.make_batched(name, B, seed=SEED, autoreset=False, tally=True, max_episode_steps=MAXS)
    env.set_mlp_policy(ws)
    env.set_mlp_safety(cw, _median_threshold(ni, "pg", name))
    ld, lda, ostep = B + 3, B + 5, (B * S + 3) // 4 * 4 + 8
    a = Arena("cuda")
    rew = a.add("reward_out", "f32", Layout(T, ld, 1, ld, B))
    fl = a.add("flags_out", "flags", Layout(T, ld, 1, ld, B))
    pr = a.add("prob_out", "f32", Layout(T, ld, 1, ld, B))
    rk = a.add("risk_out", "f32", Layout(T, ld, 1, ld, B))
    ch = a.add("choice_out", "i32", Layout(T, ld, 1, ld, B))
    obs = a.add("obs_out", "f32", Layout(T, ostep, 1, B * S, B * S, lane_width=S), align=16)
    act = a.add("act_out", "f32", Layout(T, A * lda + 7, A, lda, B))
    a.build()
    env.reset()
    p = lambda b: C.c_void_p(b.ptr)
    rc = ni._lib.lib().nig_rollout_mlp_search(env._h, T, 5, p(rew), p(fl), ld, p(obs), ostep, p(act), lda, A * lda + 7, p(pr), p(rk), p(ch),
                                              env._stream())
    assert rc == 0, ni._lib.lib().nig_last_error()
    torch.cuda.synchronize()
    f = fl.rows(T)[:, 0]
    live = (f & ni._lib.FLAG_INACTIVE) == 0
    assert bool(live[0].all()) and not bool(live[-1].any()) and bool((f & ni._lib.FLAG_SHIELDED)[live].bool().any())
    written = {b.name: dict(n_outer=T, live=live if b in (pr, rk, ch, obs, act) else None) for b in (rew, fl, pr, rk, ch, obs, act)}
    findings = [str(x) for x in a.check(written)]
    assert not findings, "\n  ".join(findings)
    env.close()


# ---- 9 ---------------------------------------------------------------------------------------------------------------------
def test_evaluate_with_safety_runs_the_fused_search(ni, monkeypatch):
    """evaluate_with_safety(policy.searching(5, 2.0), env) reaches rollout_mlp_search and, at a threshold no p reaches, returns
    the 13-key dict of policy.shielded(2.0), value for value (the two kernels agree bit for bit there)."""
    ws, cw, S, A = _nets(ni, "cr", "ChemicalReactor-v0")
    pol = ni.MLPPolicy(ws, safety_weights=cw)
    a = ni.make_batched("ChemicalReactor-v0", 256, autoreset=False, tally=True, max_episode_steps=24)
    b = ni.make_batched("ChemicalReactor-v0", 256, autoreset=False, tally=True, max_episode_steps=24)
    want = ni.evaluate_with_safety(pol.shielded(2.0), b, n_episodes=256)
    sp = pol.searching(5, 2.0)
    assert sp.fusable

    def boom(*_a, **_k):
        raise AssertionError("the fused search must not step or predict on the host")
    monkeypatch.setattr(a, "step", boom)
    monkeypatch.setattr(sp, "predict", boom)
    monkeypatch.setattr(sp, "predict_device", boom)
    calls = []
    real = a.rollout_mlp_search
    monkeypatch.setattr(a, "rollout_mlp_search", lambda *x, **k: (calls.append(x), real(*x, **k)))
    got = ni.evaluate_with_safety(sp, a, n_episodes=256)
    assert calls and all(c[1] == 5 for c in calls)
    assert len(got) == 13 and set(got) == set(want)
    for k in want:
        assert got[k] == want[k], k
    a.close(); b.close()


def test_a_128_wide_critic_runs_through_the_padding_helper(ni, oracle):
    """The reference's RiskEstimator width: pad_critic's 256-wide network gives, on the device, p within 1e-5 of a float64
    host critic on the UNPADDED weights, and bit for bit oracle.mlp_critic on the padded ones."""
    from neorl_industrial_gym_amd.policies import pad_critic
    ws, cw256, S, A = _nets(ni, "cr", "ChemicalReactor-v0")
    rng = np.random.default_rng(91)
    h = 128
    narrow = [(cw256[0][0][:, :h].copy(), cw256[0][1][:h].copy()), (rng.normal(0, 1.0 / np.sqrt(h), (h, h)).astype(f32), rng.normal(0, 0.05, h).astype(f32)),
              (rng.normal(0, 1.0 / 2, (h, 1)).astype(f32), rng.normal(0, 0.1, 1).astype(f32))]
    padded = pad_critic(narrow)
    env, o = _run(ni, "ChemicalReactor-v0", True, ws, padded, 2.0, 1, 700)
    env.close()
    z = np.concatenate([o["obs"], o["act"]], axis=-1).astype(np.float64)
    for i, (W, b) in enumerate(narrow):
        z = z @ W.astype(np.float64) + b.astype(np.float64)
        if i < 2:
            z = np.maximum(z, 0)
    p64 = 1.0 / (1.0 + np.exp(-z[..., 0]))
    assert o["live"].all() and np.abs(o["prob"] - p64).max() <= 1e-5
    assert len(np.unique(o["prob"][0])) > 100
    for k in range(T):
        assert np.array_equal(_bits(o["prob"][k]), _bits(oracle.mlp_critic("cr", padded, o["obs"][k], o["act"][k]))), k
