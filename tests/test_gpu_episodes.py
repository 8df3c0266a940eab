"""-m gpu: per-episode records on the device (include/nig.h nig_episode_log_*, nig_collect_episodes, nig_reduce_episodes;
csrc/nig_episodes.hpp) and ni.evaluate_episodes.

Shapes: batch 100 (a ragged wave) and 257 (two blocks, the second nearly empty); the log's pitch at its default (batch rounded
up to 64) and at batch + 37 (no multiple of 64); max_episode_steps = 12, so lanes finish several episodes in 40 steps; capacity
3, so lanes overflow.  The reference of every comparison is episodes.episodes_from_rows (pinned against the library's own
state machine on the host by tests/test_episodes_host.py) on the rows copied back, or the kernels' own tally."""
import ctypes as C

import numpy as np
import pytest
import torch

from footprint import Arena, Layout

pytestmark = pytest.mark.gpu

NAME = {"cr": "ChemicalReactor-v0", "pg": "PowerGrid-v0", "ra": "RobotAssembly-v0", "hvac": "HVACControl-v0"}
T, CAP, MAX_STEPS = 40, 3, 12


@pytest.fixture(scope="module")
def ni():
    import neorl_industrial_gym_amd as ni
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return ni


def _actor(S, A, seed):
    rng = np.random.default_rng(seed)
    return [(rng.normal(0, 1.0 / np.sqrt(S), (S, 256)).astype(np.float32) * np.float32(0.05), rng.normal(0, 0.05, 256).astype(np.float32)),
            (rng.normal(0, 1.0 / 16, (256, 256)).astype(np.float32), rng.normal(0, 0.05, 256).astype(np.float32)),
            (rng.normal(0, 1.0 / 8, (256, A)).astype(np.float32), rng.normal(0, 0.1, A).astype(np.float32))]


def _play(ni, env, source, n, rew, fl):
    """n steps of `source` into the rows rew / fl [>= n, pitch]"""
    if source == "ring":
        ring = torch.stack([env.fill_actions(900 + env.counter + s) for s in range(n)])
        env.rollout(n, ring, rew, fl)
    elif source == "sampled":
        env.rollout_sampled(n, rew, fl)
    elif source == "mlp":
        env.rollout_mlp(n, rew, fl)
    elif source == "mlp_bf16":
        env.rollout_mlp_bf16(n, rew, fl)
    else:
        env.rollout_policy(n, rew, fl)


def _make(ni, key, B, source, autoreset, tally=False, seed=0xE915):
    env = ni.make_batched(NAME[key], B, seed=seed, autoreset=autoreset, tally=tally, max_episode_steps=MAX_STEPS)
    if source == "mpc":
        env.set_policy(ni.mpc_agent(env.state_dim, env.action_dim))
    elif source == "pid":
        env.set_policy(ni.pid_agent(env.state_dim, env.action_dim))
    elif source == "mlp":
        env.set_mlp_policy(_actor(env.state_dim, env.action_dim, 11))
    elif source == "mlp_bf16":
        env.set_mlp_policy_bf16(_actor(env.state_dim, env.action_dim, 11))
    env.reset()
    return env


def _rows(env, pitch):
    return (torch.zeros(T, pitch, dtype=torch.float32, device=env.device), torch.zeros(T, pitch, dtype=torch.int32, device=env.device))


def _host(ni, env, rew, fl, n=T, carry=None):
    B = env.batch
    return ni.episodes_from_rows(rew[:n, :B].cpu().numpy(), fl[:n, :B].cpu().numpy().view(np.uint32), bool(env.spec.reward_is_f32), CAP, carry)


def _assert_log_equals(log, want):
    """count, carry and every record a lane has: the same bits"""
    torch.cuda.synchronize()
    count = log.count.cpu().numpy().view(np.uint32)
    assert np.array_equal(count, want["count"])
    assert np.array_equal(log.carry_ret.cpu().numpy().view(np.uint64), want["carry_ret"].view(np.uint64))
    assert np.array_equal(log.carry_w.cpu().numpy().view(np.uint32), want["carry_w"])
    have = np.arange(log.capacity)[:, None] < np.minimum(count.astype(np.int64), log.capacity)[None, :]
    assert np.array_equal(log.returns.cpu().numpy().view(np.uint64)[have], want["ret"].view(np.uint64)[have])
    words = log.words.cpu().numpy().view(np.uint32)
    for j in range(5):
        assert np.array_equal(words[j][have], want["w"][j][have]), f"record word {j}"
    return count, have


CASES = [
    # (env, source of the rows, auto-reset, batch, extra log pitch)
    ("cr", "ring", True, 100, 0), ("cr", "ring", False, 100, 37), ("pg", "sampled", True, 257, 0), ("ra", "sampled", True, 100, 37),
    ("ra", "mpc", True, 257, 37), ("pg", "mpc", False, 100, 0), ("cr", "pid", True, 100, 0), ("cr", "mlp", True, 257, 0),
    ("cr", "mlp", False, 100, 37), ("hvac", "mpc", True, 100, 37), ("cr", "mlp_bf16", True, 257, 0), ("pg", "mlp_bf16", False, 100, 37),
]


@pytest.mark.parametrize("key,source,autoreset,B,extra", CASES, ids=["-".join(map(str, c)) for c in CASES])
def test_kernel_equals_host_restatement(ni, key, source, autoreset, B, extra):
    L = ni._lib
    env = _make(ni, key, B, source, autoreset)
    rew, fl = _rows(env, env.ld + 5)                       # row pitch of the inputs: beyond the batch, no multiple of 64 either
    _play(ni, env, source, T, rew, fl)
    log = env.episode_log(CAP, ld=(B + extra) if extra else None)
    assert log.ld == (B + extra if extra else -(-B // 64) * 64)
    env.collect_episodes(log, T, rew, fl)
    want = _host(ni, env, rew, fl)
    count, have = _assert_log_equals(log, want)
    f = fl[:, :B].cpu().numpy().view(np.uint32)
    if autoreset:
        assert count.min() >= T // MAX_STEPS and not (f & L.FLAG_INACTIVE).any()
    else:
        assert count.max() == 1 and (f & L.FLAG_INACTIVE).any()            # frozen lanes' rows were written and skipped
    if key == "ra" and autoreset:
        assert count.max() > CAP                                                # lanes overflow: count goes on, records stop
    # the decoded views say what the words say
    w = want["w"]
    assert np.array_equal(log.length.cpu().numpy()[have], (w[0] & L.CTR_STEP_MASK)[have])
    assert np.array_equal(log.violations.cpu().numpy()[have], (w[0] >> 16)[have])
    assert np.array_equal(log.critical.cpu().numpy()[have], ((w[1] >> L.FLAG_NCRIT_SHIFT) & 3)[have])
    assert np.array_equal(log.terminated.cpu().numpy()[have], ((w[1] & 1) != 0)[have])
    assert np.array_equal(log.truncated.cpu().numpy()[have], ((w[1] & 2) != 0)[have])
    assert np.array_equal(log.constraint_steps.cpu().numpy()[1][have], (w[2] >> 16)[have])
    assert (log.length.cpu().numpy()[have] <= MAX_STEPS).all() and (log.length.cpu().numpy()[have] >= 1).all()
    env.close()


@pytest.mark.parametrize("key,B", [("cr", 100), ("hvac", 257), ("pg", 257), ("ra", 100)])
def test_reduce_episodes_equals_the_kernels_own_tally(ni, key, B):
    """One episode per lane on a tally=True, autoreset=False handle, one fused closed-loop launch of max_episode_steps steps:
    nig_reduce_episodes(n_episodes = B) against nig_reduce_tally."""
    L = ni._lib
    env = _make(ni, key, B, "mpc", False, tally=True)
    rew, fl = _rows(env, env.ld)
    env.rollout_policy(MAX_STEPS, rew, fl)
    log = env.episode_log(1)
    env.collect_episodes(log, MAX_STEPS, rew, fl)
    got, want = log.reduce(B).cpu().numpy(), env.reduce_tally().cpu().numpy()
    assert np.all(log.count.cpu().numpy() == 1) and got[L.T_EPISODES] == B
    lane_ret = env.tally[L.T_RET_SUM].cpu().numpy()                     # one episode per lane: its return as the kernel summed it
    mine = log.returns[0].cpu().numpy()
    assert got[L.T_ROWS] == int((log.violations[0] > 0).sum().item())
    if env.spec.reward_is_f32:
        assert np.array_equal(got[:L.T_ROWS].view(np.uint64), want.view(np.uint64)), (got, want)
        assert np.array_equal(mine.view(np.uint64), lane_ret.view(np.uint64))
    else:
        integer_rows = [L.T_EPISODES, L.T_LEN_SUM, L.T_LEN_SQ, L.T_VIOL, L.T_CRIT, L.T_SHUTDOWN, L.T_SATISFIED, L.T_CONSTRAINTS]
        assert np.array_equal(got[integer_rows], want[integer_rows])
        # reward_out is the float64 reward rounded to float32: half an ulp, 2^-24 relative, per stored reward; twice that also
        # covers the float64 summation of at most 12 terms (derived, not measured)
        live = (fl[:MAX_STEPS, :B].cpu().numpy().view(np.uint32) & L.FLAG_INACTIVE) == 0
        bound = (np.abs(rew[:MAX_STEPS, :B].cpu().numpy().astype(np.float64)) * live).sum(0) * 2.0 ** -23
        err = np.abs(mine - lane_ret)
        print(f"{key}: max |return - kernel's| = {err.max():.3e}, bound min {bound.min():.3e}, worst ratio {np.max(err / np.maximum(bound, 1e-300)):.3f}")
        assert np.all(err <= bound)
        if np.all(np.abs(lane_ret) > bound):                             # no return close enough to zero for its sign to turn
            assert got[L.T_SUCCESS] == want[L.T_SUCCESS]
    env.close()


def test_chunk_invariance_on_the_device(ni):
    logs = []
    for cuts in ((T,), (13, 27)):
        env = _make(ni, "pg", 257, "sampled", True)
        rew, fl = _rows(env, env.ld)
        log = env.episode_log(CAP, ld=257 + 37)
        for n in cuts:
            env.rollout_sampled(n, rew, fl)
            env.collect_episodes(log, n, rew, fl)
        torch.cuda.synchronize()
        count = log.count.cpu().numpy()
        have = torch.from_numpy(np.arange(CAP)[:, None] < np.minimum(count, CAP)[None, :]).to(env.device)
        logs.append((count, log.carry_ret.cpu().numpy().view(np.uint64), log.carry_w.cpu().numpy(),
                     log.returns[have].cpu().numpy().view(np.uint64), log.words[:, have].cpu().numpy()))
        env.close()
    assert logs[0][0].max() > CAP and logs[0][0].min() >= 3
    for a, b in zip(*logs):
        assert np.array_equal(a, b)


def _mark(mask, byte_off, rows, pitch, B, words_per_elem, row_cols=None):
    """set the words of columns [0, B) (or of the (row, col) pairs in row_cols) of a [rows][pitch] array at byte_off"""
    base = byte_off // 4
    if row_cols is None:
        r, c = np.meshgrid(np.arange(rows), np.arange(B), indexing="ij")
        r, c = r.reshape(-1), c.reshape(-1)
    else:
        r, c = row_cols
    for k in range(words_per_elem):
        mask[base + (r * pitch + c) * words_per_elem + k] = True


@pytest.mark.parametrize("B,extra", [(100, 37), (257, 0)])
def test_where_the_log_entry_points_write(ni, B, extra):
    L = ni._lib
    env = _make(ni, "ra", B, "sampled", True)
    rew0, fl0 = _rows(env, env.ld)
    env.rollout_sampled(T, rew0, fl0)
    lay = L.episode_log_query(B, CAP, B + extra if extra else 0)
    pitch, n = int(lay.ld), int(lay.bytes) // 4
    in_pitch = B + 3
    a = Arena("cuda")
    logb = a.add("log", "i32", Layout(1, n, 1, n, n), align=16, extra_outer=0)
    rw = a.add("reward", "f32", Layout(T, in_pitch, 1, in_pitch, B), role="in", extra_outer=0)
    fw = a.add("flags", "flags", Layout(T, in_pitch, 1, in_pitch, B), role="in", extra_outer=0)
    part = a.add("partial_out", "f64", Layout(1, L.T_ROWS + 1, 1, L.T_ROWS + 1, L.T_ROWS + 1), extra_outer=0)
    a.build()
    rw.rows()[:, 0, :] = rew0[:, :B].view(torch.int32)           # pad columns and stride gaps of the inputs keep the canary (a NaN)
    fw.rows()[:, 0, :] = fl0[:, :B]
    a.freeze_inputs()
    lib, h, st = env._L, env._h, env._stream()
    ld_arg = B + extra if extra else 0
    mask = np.zeros(n, bool)

    def check(stage, partial_written):
        torch.cuda.synchronize()
        found = [str(f) for f in a.check({"log": dict(n_outer=1, mask=torch.from_numpy(mask).to("cuda")),
                                          "partial_out": dict(n_outer=1) if partial_written else None})]
        assert not found, (stage, found)

    assert lib.nig_episode_log_init(h, logb.ptr, CAP, ld_arg, st) == 0
    _mark(mask, lay.off_count, 1, pitch, B, 1)
    _mark(mask, lay.off_carry_ret, 1, pitch, B, 2)
    _mark(mask, lay.off_carry_w, 4, pitch, B, 1)
    check("init", False)
    assert lib.nig_collect_episodes(h, T, rw.ptr, fw.ptr, in_pitch, logb.ptr, CAP, ld_arg, st) == 0
    want = ni.episodes_from_rows(rew0[:, :B].cpu().numpy(), fl0[:, :B].cpu().numpy().view(np.uint32), False, CAP)
    assert want["count"].max() > CAP and want["count"].min() >= 3
    have = np.nonzero(np.arange(CAP)[:, None] < np.minimum(want["count"].astype(np.int64), CAP)[None, :])
    _mark(mask, lay.off_ret, CAP, pitch, B, 2, have)
    for j in range(5):
        _mark(mask, lay.off_w[j], CAP, pitch, B, 1, have)
    check("collect", False)              # record rows at or beyond a lane's count / capacity, pad columns, red zones: canary
    words = logb.ints.cpu().numpy()
    count = words[lay.off_count // 4:lay.off_count // 4 + B].view(np.uint32)
    assert np.array_equal(count, want["count"])
    assert lib.nig_reduce_episodes(h, logb.ptr, CAP, ld_arg, B * CAP, part.ptr, st) == 0
    _mark(mask, lay.off_tally, L.T_ROWS + 1, pitch, B, 2)
    nblk = -(-B // 256)
    mask[lay.off_scratch // 4:lay.off_scratch // 4 + nblk * L.T_ROWS * 2] = True
    check("reduce", True)
    got = part.data.cpu().numpy()
    assert got[L.T_EPISODES] == np.minimum(want["count"], CAP).sum()
    env.close()


def test_refusals_launch_nothing(ni):
    L = ni._lib
    env = _make(ni, "cr", 100, "sampled", True)
    B = env.batch
    lay = L.episode_log_query(B, CAP, 0)
    mem = torch.full((int(lay.bytes) // 4,), 0x5A5A5A5B, dtype=torch.int32, device=env.device)
    rew, fl = _rows(env, env.ld)
    part = torch.full((L.T_ROWS + 1,), 7.0, dtype=torch.float64, device=env.device)
    lib, h, st = env._L, env._h, env._stream()
    p, r, f, o = mem.data_ptr(), rew.data_ptr(), fl.data_ptr(), part.data_ptr()
    refused = [
        lib.nig_episode_log_init(h, p, 0, 0, st),                              # capacity below 1
        lib.nig_episode_log_init(h, p, CAP, B - 1, st),                        # ld < batch
        lib.nig_episode_log_init(h, None, CAP, 0, st),
        lib.nig_episode_log_init(h, p + 4, CAP, 0, st),                        # not 8-byte aligned
        lib.nig_episode_log_init(None, p, CAP, 0, st),
        lib.nig_collect_episodes(h, 0, r, f, env.ld, p, CAP, 0, st),           # n_steps < 1
        lib.nig_collect_episodes(h, T, None, f, env.ld, p, CAP, 0, st),        # NULL reward with flags
        lib.nig_collect_episodes(h, T, r, None, env.ld, p, CAP, 0, st),
        lib.nig_collect_episodes(h, T, r, f, B - 1, p, CAP, 0, st),            # out_stride < batch
        lib.nig_collect_episodes(h, T, r, f, 0, p, CAP, 0, st),                # stride 0 with more than one step
        lib.nig_collect_episodes(h, T, r, f, env.ld, p, 0, 0, st),
        lib.nig_collect_episodes(h, T, r, f, env.ld, p, CAP, B - 1, st),
        lib.nig_reduce_episodes(h, p, CAP, 0, 0, o, st),                       # n_episodes < 1
        lib.nig_reduce_episodes(h, p, CAP, 0, CAP * B + 1, o, st),
        lib.nig_reduce_episodes(h, p, CAP, 0, B, None, st),
        lib.nig_reduce_episodes(h, p, 0, 0, B, o, st),
    ]
    torch.cuda.synchronize()
    assert refused == [1] * len(refused)
    assert b"nig_reduce_episodes" in lib.nig_last_error()
    assert bool((mem == 0x5A5A5A5B).all().item()) and bool((part == 7.0).all().item())
    with pytest.raises(L.NigError, match="capacity"):
        env.episode_log(0)
    env.close()


class HostAgent:
    """an agent that only has predict(): the per-step host loop"""
    is_trained = True

    def __init__(self, A):
        self.A = A

    def predict(self, obs, deterministic=True):
        obs = np.asarray(obs, dtype=np.float32)
        return np.clip(obs[:, :self.A] * np.float32(0.01) - np.float32(0.1), -1, 1).astype(np.float32)


KEYS13 = ["return_mean", "return_std", "return_min", "return_max", "length_mean", "length_std", "safety_violations",
          "safety_violations_per_episode", "critical_violations", "emergency_shutdowns", "constraint_satisfaction_rate",
          "successful_episodes", "success_rate"]


def _counted(env, calls, name):
    inner = getattr(env, name)

    def call(*a, **k):
        calls[name] += 1
        return inner(*a, **k)

    setattr(env, name, call)


@pytest.mark.parametrize("key,agent", [("cr", "mpc"), ("hvac", "mpc"), ("cr", "host"), ("pg", "mpc"), ("cr", "bf16"), ("pg", "bf16")])
def test_evaluate_episodes_rounds_mode_equals_evaluate_with_safety(ni, key, agent):
    B, n = 100, 250                                                   # three rounds, the last one half full
    out = []
    for fn in (ni.evaluate_with_safety, lambda a, e, n_episodes: ni.evaluate_episodes(a, e, n_episodes, chunk=5)):
        env = ni.make_batched(NAME[key], B, seed=0xE915, autoreset=False, tally=True, max_episode_steps=MAX_STEPS)
        calls = {"rollout_mlp_bf16": 0, "rollout_mlp": 0}
        if agent == "bf16":                                               # the bf16 actor: both evaluations reach its own kernel
            ag = ni.MLPPolicy(_actor(env.state_dim, env.action_dim, 11)).bf16()
            _counted(env, calls, "rollout_mlp_bf16")
            _counted(env, calls, "rollout_mlp")
        else:
            ag = ni.mpc_agent(env.state_dim, env.action_dim) if agent == "mpc" else HostAgent(env.action_dim)
        out.append(fn(ag, env, n_episodes=n))
        if agent == "bf16":
            assert calls["rollout_mlp_bf16"] >= 1 and calls["rollout_mlp"] == 0, calls
        env.close()
    ref, got = out
    assert got["mode"] == "rounds" and got["n_episodes"] == n and got["returns"].shape == (n,)
    exact = KEYS13 if key != "pg" else ["length_mean", "length_std", "safety_violations", "safety_violations_per_episode",
                                        "critical_violations", "emergency_shutdowns", "constraint_satisfaction_rate"]
    for k in exact:
        assert got[k] == ref[k], (k, got[k], ref[k])
    r = got["returns"].cpu().numpy()
    assert got["return_min"] == r.min() and got["return_max"] == r.max()
    assert int(got["lengths"].sum().item()) == round(got["length_mean"] * n)
    assert int(got["violations"].sum().item()) == got["safety_violations"]


def test_evaluate_episodes_quota_mode(ni):
    B, n = 100, 250
    env = ni.make_batched(NAME["ra"], B, seed=0xE915, autoreset=True, max_episode_steps=MAX_STEPS)
    agent = ni.mpc_agent(env.state_dim, env.action_dim)
    got = ni.evaluate_episodes(agent, env, n, chunk=10)
    assert got["mode"] == "quota" and got["n_episodes"] == n
    r, ln, v = got["returns"].cpu().numpy(), got["lengths"].cpu().numpy(), got["violations"].cpu().numpy()
    assert r.shape == ln.shape == v.shape == (n,) and r.dtype == np.float64
    assert got["return_median"] == float(np.median(r))
    assert got["violation_rate"] == float(np.mean(v > 0))
    assert got["return_sem"] == float(np.std(r, ddof=1) / np.sqrt(n))
    assert got["safety_violations"] == int(v.sum()) and got["length_mean"] == ln.sum() / n
    assert abs(got["return_mean"] - r.mean()) <= 1e-12 * max(1.0, np.abs(r).sum() / n)
    assert got["sample_efficiency"] == got["return_mean"] / got["length_mean"]
    assert got["return_min"] == r.min() and got["return_max"] == r.max()
    assert (ln >= 1).all() and (ln <= MAX_STEPS).all()
    assert np.array_equal(got["terminated"].cpu().numpy() | got["truncated"].cpu().numpy(), np.ones(n, bool))
    try:
        import scipy.stats  # noqa: F401
        lo, hi = got["confidence_interval"]
        assert lo < got["return_mean"] < hi
    except ImportError:
        assert got["confidence_interval"] is None
    # every lane played its quota; exactly n episodes were counted, in the order k * B + i
    log = env.episode_log(3)
    rew, fl = _rows(env, env.ld)
    env.reset()
    env.rollout_policy(T, rew, fl)
    env.collect_episodes(log, T, rew, fl)
    assert int(log.count.min().item()) >= 3
    part = log.reduce(n).cpu().numpy()
    assert part[ni._lib.T_EPISODES] == n
    eps = log.episodes(n)
    assert np.array_equal(eps["returns"].cpu().numpy(), np.concatenate([log.returns[0].cpu().numpy(), log.returns[1].cpu().numpy(),
                                                                        log.returns[2, :50].cpu().numpy()]))
    with pytest.raises(ValueError, match="runs in the kernel"):
        ni.evaluate_episodes(HostAgent(env.action_dim), env, n)
    env.close()
