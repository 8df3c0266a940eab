"""-m gpu: the fused safety-critic shield (nig_rollout_mlp_safe, BatchedIndustrialEnv.rollout_mlp_safe) -- the
reference agents' predict_with_safety (agents/cql.py:354-394) in the MFMA actor kernel -- against the CPU oracle's
actor and env step and a float64 host critic, and evaluate_with_safety's fused shielded path against its host form."""
import numpy as np
import pytest
import torch

import closed_loop_matrix as M

pytestmark = pytest.mark.gpu

ENVS = M.MFMA_ENVS        # which env brings which kernel shape: tests/closed_loop_matrix.py
# AdvancedPowerGrid resets every lane to the same state, draws no noise, and ends an episode whenever a voltage set-point
# action (a[4], a[5]) lies below 0.95 -- which a halved tanh output always does.  So its lanes never spread p and never
# continue an always-halved episode: the two tests that need that take the envs below, and
# test_always_shield_ends_advanced_power_grid_episodes_like_the_oracle covers its always-shield case.  AdvancedChemicalReactor
# resets every lane to one state too.  test_shield_matrix below runs both from per-lane distinct start states (never, always and
# mixed), so that a p or an action row that reaches the wrong lane shows.
ENVS_SPREAD = [e for e in ENVS if e[0] != "apg"]
B, T, MAXS, SEED = 3000, 14, 9, 0x5EED        # B not a multiple of 128: a partial last block


@pytest.fixture(scope="module")
def ni():
    import neorl_industrial_gym_amd as ni
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return ni


def _random_actor(S, A, seed):       # the style of test_gpu_parity.py's MFMA-actor test
    rng = np.random.default_rng(seed)
    return [(rng.normal(0, 1.0 / np.sqrt(S), (S, 256)).astype(np.float32) * np.float32(0.05), rng.normal(0, 0.05, 256).astype(np.float32)),
            (rng.normal(0, 1.0 / 16, (256, 256)).astype(np.float32), rng.normal(0, 0.05, 256).astype(np.float32)),
            (rng.normal(0, 1.0 / 8, (256, A)).astype(np.float32), rng.normal(0, 0.1, A).astype(np.float32))]


def _random_critic(S, A, seed):
    rng = np.random.default_rng(seed)
    D = S + A
    return [(rng.normal(0, 1.0 / np.sqrt(D), (D, 256)).astype(np.float32) * np.float32(0.05), rng.normal(0, 0.05, 256).astype(np.float32)),
            (rng.normal(0, 1.0 / 16, (256, 256)).astype(np.float32), rng.normal(0, 0.05, 256).astype(np.float32)),
            (rng.normal(0, 1.0 / 2, (256, 1)).astype(np.float32), rng.normal(0, 0.1, 1).astype(np.float32))]


def _critic64(cw, obs, act):
    z = np.concatenate([obs.astype(np.float64), act.astype(np.float64)], axis=-1)
    for i, (W, b) in enumerate(cw):
        z = z @ W.astype(np.float64) + b.astype(np.float64)
        if i < 2:
            z = np.maximum(z, 0)
    return 1.0 / (1.0 + np.exp(-z[..., 0]))


def _run(ni, name, autoreset, ws, cw, thr, B=B):
    env = ni.make_batched(name, B, autoreset=autoreset, tally=True, max_episode_steps=MAXS)
    env.set_mlp_policy(ws)
    env.set_mlp_safety(cw, thr)
    dev = env.device
    act = torch.zeros(T, env.action_dim, env.ld, dtype=torch.float32, device=dev)
    obs = torch.zeros(T, B, env.state_dim, dtype=torch.float32, device=dev)
    fl = torch.zeros(T, env.ld, dtype=torch.int32, device=dev)
    rw = torch.zeros(T, env.ld, dtype=torch.float32, device=dev)
    pr = torch.zeros(T, env.ld, dtype=torch.float32, device=dev)
    env.reset()
    env.rollout_mlp_safe(T, rw, fl, obs, act, pr)
    torch.cuda.synchronize()
    out = dict(act=act[:, :, :B].permute(0, 2, 1).cpu().numpy(), obs=obs.cpu().numpy(), flags=fl[:, :B].cpu().numpy(),
               prob=pr[:, :B].cpu().numpy())
    out["live"] = (out["flags"] & ni._lib.FLAG_INACTIVE) == 0
    out["shielded"] = (out["flags"] & ni._lib.FLAG_SHIELDED) != 0
    return env, out


@pytest.mark.parametrize("key,name", ENVS)
@pytest.mark.parametrize("autoreset", [False, True])
def test_never_shield_is_the_plain_actor(ni, oracle, key, name, autoreset):
    """Threshold 2.0 (p < 2 always): every action, the final state, step, done and tallies bit for bit the oracle's
    MFMA-actor rollout; p within 1e-5 of a float64 critic on the recorded (obs, act); no shield flag."""
    probe = ni.make_batched(name, 1)
    S, A = probe.state_dim, probe.action_dim
    probe.close()
    ws, cw = _random_actor(S, A, 11), _random_critic(S, A, 12)
    env, o = _run(ni, name, autoreset, ws, cw, 2.0)
    r = oracle.rollout_mlp(key, B, T, ws, max_steps=MAXS, autoreset=autoreset, nthreads=8, trajectories=True)
    live = o["live"]
    assert np.array_equal(o["act"].view(np.uint32)[live], r["act"].view(np.uint32)[live])
    assert np.array_equal(env.get_state().cpu().numpy().view(np.uint32), r["state"].view(np.uint32))
    assert np.array_equal(env.current_step.cpu().numpy(), r["step"]) and np.array_equal(env.done.cpu().numpy(), r["done"] != 0)
    assert np.array_equal(env.tally[ni._lib.T_EPISODES].cpu().numpy(), [t.episodes for t in r["tallies"]])
    assert np.array_equal(env.total_violations.cpu().numpy(), [t.violations for t in r["tallies"]])
    p64 = _critic64(cw, o["obs"], o["act"])
    assert np.allclose(o["prob"][live], p64[live], atol=1e-5, rtol=0)
    for k in range(T):                  # and bit for bit the oracle's restatement of the critic in the device's order
        pk = oracle.mlp_critic(key, cw, o["obs"][k], o["act"][k])
        assert np.array_equal(o["prob"][k].view(np.uint32)[live[k]], pk.view(np.uint32)[live[k]]), k
    assert not o["shielded"].any()
    env.close()


@pytest.mark.parametrize("key,name", ENVS_SPREAD)
@pytest.mark.parametrize("autoreset", [False, True])
def test_always_shield_halves_and_steps_with_the_halved_action(ni, oracle, key, name, autoreset):
    """Threshold 0.0 (p is never below 0): every live action is 0.5 x the oracle's actor on the recorded observation,
    bit for bit, with the flag set; the next observation is the oracle's env step on that halved action."""
    probe = ni.make_batched(name, 1)
    S, A = probe.state_dim, probe.action_dim
    probe.close()
    ws, cw = _random_actor(S, A, 21), _random_critic(S, A, 22)
    env, o = _run(ni, name, autoreset, ws, cw, 0.0)
    live, L = o["live"], ni._lib
    assert np.array_equal(o["shielded"], live)
    for k in range(T):
        raw = oracle.mlp_actions(key, ws, o["obs"][k])
        want = (raw * np.float32(0.5)).astype(np.float32)
        assert np.array_equal(o["act"][k].view(np.uint32)[live[k]], want.view(np.uint32)[live[k]]), k
    # teacher-forced env step on the first lanes: obs[k+1] = step(obs[k], act[k]) where the lane neither finished nor reset
    n, checked = 400, 0
    for k in range(T - 1):
        fl = o["flags"][k, :n]
        step_after = (fl.astype(np.uint32) >> L.FLAG_STEP_SHIFT).astype(np.int32)
        nz = np.stack([oracle.gen_step_noise(key, SEED, i, k + 1) for i in range(n)]) if oracle.spec(key).k_step else None
        r = oracle.step(key, o["obs"][k, :n], o["act"][k, :n], nz, step_after - 1, max_steps=MAXS, flavor=oracle.MATH_POLY)
        cont = live[k, :n] & live[k + 1, :n] & ((fl & (L.FLAG_TERMINATED | L.FLAG_TRUNCATED | L.FLAG_DID_RESET)) == 0)
        checked += int(cont.sum())
        assert np.array_equal(o["obs"][k + 1, :n][cont].view(np.uint32), r["state_next"][cont].view(np.uint32)), k
    assert checked > n
    env.close()


def test_always_shield_ends_advanced_power_grid_episodes_like_the_oracle(ni, oracle):
    """AdvancedPowerGrid at threshold 0.0, no auto-reset: every action of step 0 is 0.5 x the oracle's actor bit for bit
    and flagged; the halved step ends every episode exactly where the oracle's step does, and the state each lane keeps
    is that step's next state, bit for bit."""
    key, name = "apg", "AdvancedPowerGrid-v0"
    probe = ni.make_batched(name, 1)
    S, A = probe.state_dim, probe.action_dim
    probe.close()
    ws, cw = _random_actor(S, A, 21), _random_critic(S, A, 22)
    env, o = _run(ni, name, False, ws, cw, 0.0)
    live, L = o["live"], ni._lib
    assert np.array_equal(o["shielded"], live) and live[0].all()
    raw = oracle.mlp_actions(key, ws, o["obs"][0])
    assert np.array_equal(o["act"][0].view(np.uint32), (raw * np.float32(0.5)).astype(np.float32).view(np.uint32))
    r = oracle.step(key, o["obs"][0], o["act"][0], None, np.zeros(B, dtype=np.int32), max_steps=MAXS, flavor=oracle.MATH_POLY)
    ended = (o["flags"][0] & L.FLAG_TERMINATED) != 0
    assert np.array_equal(ended, r["terminated"] != 0) and ended.all()
    assert not live[1:].any()
    assert np.array_equal(env.get_state().cpu().numpy().view(np.uint32), r["state_next"].view(np.uint32))
    env.close()


@pytest.mark.parametrize("key,name", ENVS_SPREAD)
@pytest.mark.parametrize("autoreset", [False, True])
def test_mixed_shield_decisions(ni, oracle, key, name, autoreset):
    """A threshold inside the range of p: every live action is exactly raw or 0.5 raw (raw = the oracle's actor), the
    choice agrees with the flag, with p < thr on the kernel's own p, and with a float64 critic away from the threshold."""
    probe = ni.make_batched(name, 1)
    S, A = probe.state_dim, probe.action_dim
    probe.close()
    ws, cw = _random_actor(S, A, 31), _random_critic(S, A, 32)
    env0, o0 = _run(ni, name, autoreset, ws, cw, 2.0)
    env0.close()
    # state columns of the order of 100 (ChemicalReactor's temperatures) saturate the critic (p == 1.0 everywhere): scale
    # its state inputs by the observed magnitudes so that p spreads, then put the threshold at the median of p
    sc = (1.0 / (1.0 + np.abs(o0["obs"][o0["live"]]).mean(axis=0))).astype(np.float32)
    cw = [(np.concatenate([cw[0][0][:S] * np.float32(20.0) * sc[:, None], cw[0][0][S:]]).astype(np.float32), cw[0][1]), cw[1], cw[2]]
    env0, o0 = _run(ni, name, autoreset, ws, cw, 2.0)
    env0.close()
    thr = float(np.median(o0["prob"][o0["live"]]))
    env, o = _run(ni, name, autoreset, ws, cw, thr)
    live = o["live"]
    kept = np.zeros_like(live)
    halved = np.zeros_like(live)
    for k in range(T):
        raw = oracle.mlp_actions(key, ws, o["obs"][k])
        kept[k] = (o["act"][k].view(np.uint32) == raw.view(np.uint32)).all(axis=1)
        halved[k] = (o["act"][k].view(np.uint32) == (raw * np.float32(0.5)).view(np.uint32)).all(axis=1)
        p64 = _critic64(cw, o["obs"][k], raw)
        pk = oracle.mlp_critic(key, cw, o["obs"][k], raw)
        assert np.array_equal(o["prob"][k].view(np.uint32)[live[k]], pk.view(np.uint32)[live[k]]), k
        far = live[k] & (np.abs(p64 - thr) > 1e-4)
        assert np.array_equal(o["shielded"][k][far], (p64 >= thr)[far]), k
    sh = o["shielded"]
    assert ((kept | halved) | ~live).all()
    assert halved[live & sh].all() and kept[live & ~sh].all()
    assert np.array_equal(sh[live], ~(o["prob"][live] < np.float32(thr)))
    assert not sh[~live].any()
    frac = sh[live].mean()
    assert 0.1 <= frac <= 0.9, frac
    env.close()


# ---- the closed-loop matrix's shapes (tests/closed_loop_matrix.py) ------------------------------------------------------------
def _run_matrix(ni, key, autoreset, ws, cw, thr, B):
    """rollout_mlp_safe at the matrix's T and episode cap through the C entry point (observation rows padded to a multiple of 4
    floats where B * S is none); AdvancedChemicalReactor and AdvancedPowerGrid start from per-lane distinct states."""
    import ctypes as C
    T_, name = M.T_NEW, M.NAMES[key]
    env = ni.make_batched(name, B, autoreset=autoreset, tally=True, max_episode_steps=M.MAXS_NEW, seed=SEED)
    env.set_mlp_policy(ws)
    env.set_mlp_safety(cw, thr)
    dev, S, A, ld = env.device, env.state_dim, env.action_dim, env.ld
    ostep = (B * S + 3) // 4 * 4
    act = torch.zeros(T_, A, ld, dtype=torch.float32, device=dev)
    obs = torch.zeros(T_, ostep, dtype=torch.float32, device=dev)
    fl = torch.zeros(T_, ld, dtype=torch.int32, device=dev)
    rw, pr = (torch.zeros(T_, ld, dtype=torch.float32, device=dev) for _ in range(2))
    env.reset()
    M.install_start(ni, env, key, SEED)
    p = lambda x: C.c_void_p(x.data_ptr())
    with torch.cuda.device(dev):
        ni._lib.check(ni._lib.lib().nig_rollout_mlp_safe(env._h, T_, p(rw), p(fl), ld, p(obs), ostep, p(act), ld, A * ld, p(pr), env._stream()))
    torch.cuda.synchronize()
    o = dict(act=act[:, :, :B].permute(0, 2, 1).cpu().numpy(), obs=obs[:, :B * S].reshape(T_, B, S).cpu().numpy(), flags=fl[:, :B].cpu().numpy(),
             prob=pr[:, :B].cpu().numpy())
    o["live"] = (o["flags"] & ni._lib.FLAG_INACTIVE) == 0
    o["shielded"] = (o["flags"] & ni._lib.FLAG_SHIELDED) != 0
    env.close()
    return o


_MATRIX_NETS = {}


def _matrix_nets(ni, key):
    """(actor, critic whose state rows are scaled by the observed magnitudes so that p spreads, the median of step 0's p over
    700 lanes)."""
    if key not in _MATRIX_NETS:
        probe = ni.make_batched(M.NAMES[key], 1)
        S, A = probe.state_dim, probe.action_dim
        probe.close()
        ws, cw = M.matrix_actor(ni, key, _random_actor(S, A, 31), SEED), _random_critic(S, A, 32)
        sc = M.state_scale(ni, key, SEED)
        cw = [(np.concatenate([cw[0][0][:S] * np.float32(20.0) * sc[:, None], cw[0][0][S:]]).astype(np.float32), cw[0][1]), cw[1], cw[2]]
        p0 = _run_matrix(ni, key, True, ws, cw, 2.0, M.B_BIG)["prob"][0]
        assert len(np.unique(p0)) > 350, "the critic does not spread p over the lanes"
        _MATRIX_NETS[key] = (ws, cw, float(np.median(p0)))
    return _MATRIX_NETS[key]


@pytest.mark.parametrize("mode", ["never", "always", "mixed"])
@pytest.mark.parametrize("B,autoreset", [(M.B_BIG, True), (M.B_BIG, False), (M.B_SMALL, True)])
@pytest.mark.parametrize("key,name", M.MFMA_ENVS)
def test_shield_matrix(ni, oracle, key, name, B, autoreset, mode):
    """The shield on every MFMA env at the matrix's shapes, on the device's own obs_out: p is oracle.mlp_critic of the oracle's
    raw action, bit for bit; the action is the raw action where p < threshold and 0.5 x it elsewhere, with the flag; the next
    observation is the oracle's step on that action.  AdvancedChemicalReactor and AdvancedPowerGrid start from per-lane distinct
    states (from reset() their lanes are clones: a p or an action row stored to the wrong lane would pass).  Step 0 is also held
    to the actor and the critic in NumPy float64."""
    ws, cw, median = _matrix_nets(ni, key)
    thr = {"never": 2.0, "always": 0.0, "mixed": median}[mode]
    o = _run_matrix(ni, key, autoreset, ws, cw, thr, B)
    live, sh = o["live"], o["shielded"]
    assert live[0].all() and (autoreset or not live[-1].any())
    for k in range(M.T_NEW):
        lv = live[k]
        raw = oracle.mlp_actions(key, ws, o["obs"][k])
        pk = oracle.mlp_critic(key, cw, o["obs"][k], raw)
        assert np.array_equal(o["prob"][k].view(np.uint32)[lv], pk.view(np.uint32)[lv]), k
        want_sh = lv & ~(pk < np.float32(thr))
        assert np.array_equal(sh[k], want_sh), k
        want = np.where(want_sh[:, None], raw * np.float32(0.5), raw).astype(np.float32)
        assert np.array_equal(o["act"][k].view(np.uint32)[lv], want.view(np.uint32)[lv]), k
    checked = M.check_env_steps(oracle, ni._lib, key, o["obs"], o["act"], o["flags"], SEED, M.MAXS_NEW)
    if key == "apg" and mode == "always":
        # the plant: a halved set-point action is below 0.95, so every AdvancedPowerGrid episode ends on its first step (the
        # oracle agrees, check_env_steps) and no lane ever continues
        assert checked == 0 and ((o["flags"] & ni._lib.FLAG_TERMINATED) != 0)[live].all()
    elif key != "apg" or B == M.B_BIG:
        assert checked > 0
    raw0 = M.actor64(ws, o["obs"][0])
    if B == M.B_BIG:
        assert key not in M.CLONED or M.distinct_rows(o["act"][0]) >= 600, M.distinct_rows(o["act"][0])
        if mode == "mixed":
            assert sh[0].any() and not sh[0].all()
    if key not in M.FLOAT64_KEYS:
        return
    scale = np.where(sh[0][:, None], 0.5, 1.0)
    assert M.worst(f"{key} {mode} B={B}: actions of step 0 against float64", o["act"][0], raw0 * scale, M.ACT_ATOL) <= 1.0
    assert M.worst(f"{key} {mode} B={B}: p of step 0 against float64", o["prob"][0], M.critic64(cw, o["obs"][0], raw0), M.PROB_ATOL) <= 1.0


def _spread_critic(ni, name, autoreset, ws, cw, S):
    """The critic with its state inputs scaled by the observed magnitudes, so that p spreads (test_mixed_shield_decisions)."""
    env0, o0 = _run(ni, name, autoreset, ws, cw, 2.0)
    env0.close()
    sc = (1.0 / (1.0 + np.abs(o0["obs"][o0["live"]]).mean(axis=0))).astype(np.float32)
    return [(np.concatenate([cw[0][0][:S] * np.float32(20.0) * sc[:, None], cw[0][0][S:]]).astype(np.float32), cw[0][1]), cw[1], cw[2]]


@pytest.mark.parametrize("key,name", ENVS)
def test_threshold_equal_to_an_occurring_p_is_shielded(ni, oracle, key, name):
    """The threshold is a p that occurs at step 0 of the shielded run itself (step 0 acts on the reset states, so its p is
    that of the never-shield run bit for bit): the lanes with p == threshold must be shielded (the shield is !(p < thr),
    not p > thr), those below it must not, and p is the oracle critic's bit for bit."""
    probe = ni.make_batched(name, 1)
    S, A = probe.state_dim, probe.action_dim
    probe.close()
    ws, cw = _random_actor(S, A, 61), _random_critic(S, A, 62)
    cw = _spread_critic(ni, name, True, ws, cw, S)
    env0, o0 = _run(ni, name, True, ws, cw, 2.0)
    env0.close()
    p0 = np.sort(o0["prob"][0][o0["live"][0]])
    thr = p0[len(p0) // 2]                                  # a float32 p of step 0, not a mean of two
    env, o = _run(ni, name, True, ws, cw, float(thr))
    live = o["live"]
    assert np.array_equal(o["prob"][0].view(np.uint32), o0["prob"][0].view(np.uint32))
    at = live[0] & (o["prob"][0] == thr)
    assert at.any()
    assert o["shielded"][0][at].all()
    assert not o["shielded"][0][live[0] & (o["prob"][0] < thr)].any()
    assert np.array_equal(o["shielded"][live], ~(o["prob"][live] < thr))
    for k in range(T):
        raw = oracle.mlp_actions(key, ws, o["obs"][k])
        pk = oracle.mlp_critic(key, cw, o["obs"][k], raw)
        assert np.array_equal(o["prob"][k].view(np.uint32)[live[k]], pk.view(np.uint32)[live[k]]), k
    env.close()


@pytest.mark.parametrize("key,name", [("cr", "ChemicalReactor-v0"), ("pg", "PowerGrid-v0"), ("apg", "AdvancedPowerGrid-v0")])
@pytest.mark.parametrize("b", [1, 33, 129])
def test_small_batches(ni, oracle, key, name, b):
    """Batches of one lane, of part of a wave and of one block plus one lane: actions, p and the final state against the
    oracle (threshold 2.0: the plain actor) and, at a threshold inside the range of p, the shield decision."""
    probe = ni.make_batched(name, 1)
    S, A = probe.state_dim, probe.action_dim
    probe.close()
    ws, cw = _random_actor(S, A, 71), _random_critic(S, A, 72)
    env, o = _run(ni, name, True, ws, cw, 2.0, B=b)
    r = oracle.rollout_mlp(key, b, T, ws, max_steps=MAXS, autoreset=True, nthreads=8, trajectories=True)
    live = o["live"]
    assert np.array_equal(o["act"].view(np.uint32)[live], r["act"].view(np.uint32)[live])
    assert np.array_equal(env.get_state().cpu().numpy().view(np.uint32), r["state"].view(np.uint32))
    for k in range(T):
        pk = oracle.mlp_critic(key, cw, o["obs"][k], o["act"][k])
        assert np.array_equal(o["prob"][k].view(np.uint32)[live[k]], pk.view(np.uint32)[live[k]]), k
    env.close()
    thr = float(o["prob"][0][0])
    env, o = _run(ni, name, True, ws, cw, thr, B=b)
    assert o["shielded"][0][0]
    assert np.array_equal(o["shielded"][o["live"]], ~(o["prob"][o["live"]] < np.float32(thr)))
    env.close()


@pytest.mark.parametrize("key,name", [("cr", "ChemicalReactor-v0"), ("apg", "AdvancedPowerGrid-v0")])
def test_two_launches_continue_one_rollout(ni, oracle, key, name):
    """A shielded rollout in two launches from launch counter t0 (threshold 2.0) is the oracle's single rollout from t0:
    the second launch takes up the counter, the states and the episode steps where the first left them."""
    probe = ni.make_batched(name, 1)
    S, A = probe.state_dim, probe.action_dim
    probe.close()
    ws, cw = _random_actor(S, A, 81), _random_critic(S, A, 82)
    b, t0, T1, T2 = 700, 37, 5, 8
    env = ni.make_batched(name, b, autoreset=True, tally=True, max_episode_steps=MAXS)
    env.set_mlp_policy(ws)
    env.set_mlp_safety(cw, 2.0)
    env.counter = t0
    env.reset()
    acts = []
    for n in (T1, T2):
        act = torch.zeros(n, env.action_dim, env.ld, dtype=torch.float32, device=env.device)
        fl = torch.zeros(n, env.ld, dtype=torch.int32, device=env.device)
        rw = torch.zeros(n, env.ld, dtype=torch.float32, device=env.device)
        env.rollout_mlp_safe(n, rw, fl, None, act, None)
        torch.cuda.synchronize()
        acts.append(act[:, :, :b].permute(0, 2, 1).cpu().numpy())
    assert env.counter == t0 + T1 + T2
    r = oracle.rollout_mlp(key, b, T1 + T2, ws, t0=t0, max_steps=MAXS, autoreset=True, nthreads=8, trajectories=True)
    assert np.array_equal(np.concatenate(acts).view(np.uint32), r["act"].view(np.uint32))
    assert np.array_equal(env.get_state().cpu().numpy().view(np.uint32), r["state"].view(np.uint32))
    assert np.array_equal(env.current_step.cpu().numpy(), r["step"])
    env.close()


@pytest.mark.parametrize("thr", [2.0, 1e-6])
def test_evaluate_with_safety_runs_the_fused_shield(ni, monkeypatch, thr):
    """evaluate_with_safety(MLPPolicy.from_agent(agent).shielded(thr), batched env) takes the fused kernel and gives the
    dict of the host loop around predict_with_safety (same nets, different float32 summation order)."""
    import types
    S, A = 12, 3
    ws, cw = _random_actor(S, A, 41), _random_critic(S, A, 42)
    flax = lambda layers: {"params": {"MLP_0": {f"Dense_{i}": {"kernel": W, "bias": b} for i, (W, b) in enumerate(layers)}}}
    agent = types.SimpleNamespace(state={"actor": types.SimpleNamespace(params=flax(ws)),
                                         "safety": types.SimpleNamespace(params=flax(cw))},
                                  constraint_threshold=0.1, is_trained=True)
    pol = ni.MLPPolicy.from_agent(agent).shielded(thr)
    assert pol.fusable
    a = ni.make_batched("ChemicalReactor-v0", 256, autoreset=False, tally=True, max_episode_steps=48)
    b = ni.make_batched("ChemicalReactor-v0", 256, autoreset=False, tally=True, max_episode_steps=48)

    class HostOnly:
        is_trained = True

        def predict(self, obs, deterministic=True):
            return pol.predict(obs)
    want = ni.evaluate_with_safety(HostOnly(), b, n_episodes=256)

    def boom(*_a, **_k):
        raise AssertionError("the fused shielded path must not step or predict on the host")
    monkeypatch.setattr(a, "step", boom)
    monkeypatch.setattr(pol, "predict", boom)
    monkeypatch.setattr(pol, "predict_device", boom)
    calls = []
    real = a.rollout_mlp_safe
    monkeypatch.setattr(a, "rollout_mlp_safe", lambda *x, **k: (calls.append(x), real(*x, **k)))
    got = ni.evaluate_with_safety(pol, a, n_episodes=256)
    assert calls
    assert len(got) == 13 and set(got) == set(want)
    for k in want:
        assert got[k] == pytest.approx(want[k], rel=2e-3, abs=1e-6), k
    a.close(); b.close()


def test_shield_errors(ni):
    S, A = 12, 3
    ws, cw = _random_actor(S, A, 51), _random_critic(S, A, 52)
    env = ni.make_batched("ChemicalReactor-v0", 256)
    env.reset()
    with pytest.raises(ni._lib.NigError):          # no actor, no critic
        env.rollout_mlp_safe(2)
    env.set_mlp_safety(cw, 0.5)
    with pytest.raises(ni._lib.NigError):          # critic but no actor
        env.rollout_mlp_safe(2)
    env.close()
    env = ni.make_batched("ChemicalReactor-v0", 256)
    env.reset()
    env.set_mlp_policy(ws)
    with pytest.raises(ni._lib.NigError):          # actor but no critic
        env.rollout_mlp_safe(2)
    with pytest.raises(AssertionError):            # critic on S inputs instead of S + A
        env.set_mlp_safety([(cw[0][0][:S], cw[0][1]), cw[1], cw[2]], 0.5)
    with pytest.raises(AssertionError):            # two outputs
        env.set_mlp_safety([cw[0], cw[1], (np.zeros((256, 2), np.float32), np.zeros(2, np.float32))], 0.5)
    env.set_mlp_safety(cw, 0.5)
    env.set_mlp_policy(ws)                          # replacing the actor keeps the critic
    env.rollout_mlp_safe(2)
    torch.cuda.synchronize()
    env.close()
