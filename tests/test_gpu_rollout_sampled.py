"""-m gpu: nig_rollout_sampled -- the fused rollout that draws every step's uniform action in the kernel (include/nig.h).

The contract is bit-identity: the step with launch counter t takes the action nig_fill_actions(t) writes, so a sampled call
equals nig_rollout on a ring of n_steps slots filled that way -- in every kernel form the host can select (one-wave with whole
blocks and a ragged tail, three-wave, PowerGrid wide 512 / wide 256 / paired), every output mode, across chained launches
(odd and even starting counters), on handles whose lanes freeze, under a constraint mask -- and equals the CPU oracle, which
draws oracle_gen_actions(env, seed, lane, t) on every step and has no ring at all.  Then: sharding independence, no ring-sized
allocation, the refusals of nig_rollout, and the reference's statistics on the sampled path."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import refstats
from conftest import ENV_NAME

pytestmark = pytest.mark.gpu

NEVER = 1 << 30
CANARY_F, CANARY_I = -12345.5, 0x5A5A5A5A
MODES = ("none", "min", "soa", "aos")          # no outputs / reward + flags / + [S][ld] rows / + row-major [B][S] trajectory


@pytest.fixture(scope="module")
def ni():
    import neorl_industrial_gym_amd as ni
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    yield ni
    ni.tune(split_blocks=-1, wide_min_blocks=-1)


def _bufs(env, n, mode):
    """canary-filled output buffers of one call: (reward, flags, obs) or Nones"""
    dev, ld, B, S = env.device, env.ld, env.batch, env.state_dim
    if mode == "none":
        return None, None, None
    rew = torch.full((n, ld), CANARY_F, dtype=torch.float32, device=dev)
    fl = torch.full((n, ld), CANARY_I, dtype=torch.int32, device=dev)
    obs = None
    if mode == "soa":
        obs = torch.full((n, S, ld), CANARY_F, dtype=torch.float32, device=dev)
    if mode == "aos":
        obs = torch.full((n, B, S), CANARY_F, dtype=torch.float32, device=dev)
    return rew, fl, obs


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else (t.view(torch.int64) if t.dtype == torch.float64 else t)


def _same_handles(ni, a, b, what):
    L = ni._lib
    assert a.counter == b.counter, what
    assert torch.equal(_bits(a.state_soa), _bits(b.state_soa)), f"{what}: state words"
    assert torch.equal(a.ctr, b.ctr), f"{what}: ctr"
    assert torch.equal(a.life_viol, b.life_viol), f"{what}: life_viol"
    assert torch.equal(_bits(a.ep_return), _bits(b.ep_return)), f"{what}: ep_return"
    fp_rows = [L.T_RET_SUM, L.T_RET_SQ]            # several episodes of one launch are merged as one fp64 partial
    int_rows = [r for r in range(L.T_ROWS) if r not in fp_rows]
    assert torch.equal(a.tally[int_rows], b.tally[int_rows]), f"{what}: integer tally rows"
    assert torch.allclose(a.tally[fp_rows], b.tally[fp_rows], rtol=1e-14, atol=0.0), f"{what}: fp64 tally rows"


def _ring_vs_sampled(ni, env_id, B, chunks, modes, autoreset=True, max_steps=6, cmask=None, seed=0xC0FFEE, env0=12345):
    """Handle A: rollout(n, ring) with ring[s] = fill_actions(t0 + 1 + s), one slot per step; handle B: rollout_sampled(n).
    Same seed, same env_index0, the same chain of calls.  Everything observable must be equal, pad columns (canaries) included.
    Returns the number of episodes that finished."""
    kw = dict(seed=seed, env_index0=env0, autoreset=autoreset, tally=True, max_episode_steps=max_steps)
    a, b = ni.make_batched(env_id, B, **kw), ni.make_batched(env_id, B, **kw)
    if cmask is not None:
        a.set_constraint_mask(cmask); b.set_constraint_mask(cmask)
    a.reset(); b.reset()
    for i, (n, mode) in enumerate(zip(chunks, modes)):
        t0 = a.counter
        assert b.counter == t0
        ring = torch.empty(n, a.action_dim, a.ld, dtype=torch.float32, device=a.device)
        for s in range(n):
            a.fill_actions(t0 + 1 + s, ring[s])
        oa, ob = _bufs(a, n, mode), _bufs(b, n, mode)
        a.rollout(n, ring, *oa)
        b.rollout_sampled(n, *ob)
        torch.cuda.synchronize()
        what = f"{env_id} B={B} call {i} ({n} steps from counter {t0}, outputs {mode})"
        assert a.counter == b.counter == t0 + n, what
        for name, x, y in zip(("reward rows", "flag rows", "observations"), oa, ob):
            if x is not None:
                assert torch.equal(_bits(x), _bits(y)), f"{what}: {name}"
        if mode != "none":                           # the call wrote what it had to, and the rows are not trivially equal
            assert not bool((oa[1][:, :B] == CANARY_I).any()), what
        _same_handles(ni, a, b, what)
    episodes = int(a.tally[ni._lib.T_EPISODES].sum().item())
    if not autoreset:
        assert bool(a.done.all()) and bool(b.done.all()), "the lanes were meant to freeze inside the launch"
    a.close(); b.close()
    return episodes


def _kernel(ni, key, B, outputs):
    import bench
    return bench.rollout_kernel_name(types.SimpleNamespace(key=key, B=B, outputs=outputs, ni=ni))


# ----------------------------------------------------------------------------------------- 1. sampled == ring-fed
ALL_ENVS = ["ChemicalReactor-v0", "PowerGrid-v0", "RobotAssembly-v0", "AdvancedChemicalReactor-v0", "AdvancedPowerGrid-v0",
            "HVACControl-v0", "WaterTreatment-v0", "SteelAnnealing-v0", "SupplyChain-v0"]


def test_all_envs_are_covered(ni):
    assert sorted(ALL_ENVS) == sorted(ni.batched.ENV_IDS)


@pytest.mark.parametrize("env_id", ALL_ENVS)
def test_one_wave_form_whole_blocks_and_ragged_tail(ni, env_id):
    """every env id the library knows, knobs set so that nothing but rollout_kernel / rollout_sampled_kernel runs: 1000 lanes =
    three whole 256-lane blocks (FULL) + a ragged block of 232; four chained calls, one per output mode, starting on counters
    1, 8, 14, 18 (ChemicalReactor and the spec plants peel the first step of a call that starts on an even counter)."""
    ni.tune(split_blocks=0, wide_min_blocks=NEVER)
    key = {v: k for k, v in ENV_NAME.items()}.get(env_id)
    if key:                                        # (bench.rollout_kernel_name names the three reference envs only)
        assert _kernel(ni, key, 1000, "full") == "rollout_kernel<%s,3>" % env_id.split("-")[0]
    episodes = _ring_vs_sampled(ni, env_id, 1000, chunks=(7, 6, 4, 3), modes=("aos", "soa", "min", "none"))
    assert episodes > 0


@pytest.mark.parametrize("key", ["cr", "ra"])
@pytest.mark.parametrize("rounds", [1, 2])
def test_three_wave_form(ni, key, rounds):
    """ChemicalReactor and RobotAssembly, four whole blocks: one round (knob 256) and two rounds of two blocks (knob 2: only
    ChemicalReactor, and only with an observation trajectory, runs rounds -- the host's rule, shared by both entry points)."""
    ni.tune(split_blocks=256 if rounds == 1 else 2, wide_min_blocks=-1)
    B, name = 1024, {"cr": "ChemicalReactor", "ra": "RobotAssembly"}[key]
    split = "split_rollout_kernel<%s,%%d,4>" % name
    one_wave = "rollout_kernel<%s,%%d>" % name
    if rounds == 1:
        assert _kernel(ni, key, B, "full") == split % 3 and _kernel(ni, key, B, "min") == split % 1 and _kernel(ni, key, B, "none") == split % 0
    else:
        assert _kernel(ni, key, B, "full") == (split if key == "cr" else one_wave) % 3
        assert _kernel(ni, key, B, "min") == one_wave % 1
    episodes = _ring_vs_sampled(ni, ENV_NAME[key], B, chunks=(9, 6, 5, 4, 3), modes=("aos", "soa", "min", "none", "aos"), max_steps=7)
    assert episodes > 0
    # ... and with a ragged tail behind the whole blocks (a one-wave launch of its own)
    _ring_vs_sampled(ni, ENV_NAME[key], B + 100, chunks=(5, 4), modes=("aos", "min"), max_steps=7)


@pytest.mark.parametrize("form,B,split_blocks,wide_min,kernel", [
    ("wide512", 2048 + 256, 0, 1, "rollout_wide_kernel<PowerGrid,%d,512>"),      # four wide blocks + one 256-lane block (two launches)
    ("wide256", 1024, 0, 256, "rollout_wide_kernel<PowerGrid,%d,256>"),
    ("paired", 768, 256, 256, "rollout_pg_pair_kernel<%d>")])                  # register stepper (none / min), LDS stepper (trajectories)
def test_powergrid_lds_forms(ni, form, B, split_blocks, wide_min, kernel):
    ni.tune(split_blocks=split_blocks, wide_min_blocks=wide_min)
    for outputs, out in (("full", 3), ("min", 1), ("none", 0)):
        assert _kernel(ni, "pg", B, outputs) == kernel % out
    episodes = _ring_vs_sampled(ni, "PowerGrid-v0", B, chunks=(9, 6, 5, 4, 3), modes=("aos", "soa", "min", "none", "aos"), max_steps=7)
    assert episodes > 0


@pytest.mark.parametrize("key", ["cr", "pg", "ra"])
def test_lanes_that_freeze_inside_the_launch(ni, key):
    """a handle WITHOUT auto-reset: every lane ends its episode (5-step cap) inside the first call and is frozen from then on --
    the host keeps such handles on the one-wave form, for both entry points; the frozen lanes' rows (NIG_FLAG_INACTIVE, reward 0,
    the held state) are written in every later step of both calls."""
    ni.tune(split_blocks=-1, wide_min_blocks=-1)
    _ring_vs_sampled(ni, ENV_NAME[key], 1024 + 77, chunks=(9, 4), modes=("aos", "soa"), autoreset=False, max_steps=5)


@pytest.mark.parametrize("key,B,knobs", [("cr", 1024, (256, -1)), ("pg", 2048, (0, 1)), ("ra", 1000, (0, NEVER))])
def test_constraint_mask_variant(ni, key, B, knobs):
    """nig_set_constraint_mask(0b101): constraint 1 switched off on both handles (three-wave, wide and one-wave forms)"""
    ni.tune(split_blocks=knobs[0], wide_min_blocks=knobs[1])
    _ring_vs_sampled(ni, ENV_NAME[key], B, chunks=(7, 6), modes=("aos", "min"), cmask=0b101, max_steps=9)


def test_default_episode_length_with_many_steps(ni):
    """no shortened episodes: ChemicalReactor three-wave, 300 steps in two calls (151 + 149: both counter parities), the
    producer's draw at every position of its unrolled loop and in its tail"""
    ni.tune(split_blocks=-1, wide_min_blocks=-1)
    _ring_vs_sampled(ni, "ChemicalReactor-v0", 2048, chunks=(151, 149), modes=("aos", "min"), max_steps=None)


# ----------------------------------------------------------------------------------------- 2. sampled == oracle
@pytest.mark.parametrize("key,B", [("cr", 65536), ("pg", 262144), ("ra", 65536)])
def test_sampled_rollout_bit_identical_to_oracle_at_baseline_sizes(ni, oracle, key, B):
    """BASELINE sizes x 200 fused steps against the CPU oracle (oracle_rollout draws oracle_gen_actions on every step).  No
    action ring exists anywhere in this test."""
    ni.tune(split_blocks=-1, wide_min_blocks=-1)
    T = 200
    env = ni.make_batched(ENV_NAME[key], B, autoreset=True, tally=True)
    fl = torch.zeros(T, env.ld, dtype=torch.int32, device=env.device)
    rw = torch.zeros(T, env.ld, dtype=torch.float32, device=env.device)
    env.reset()
    env.rollout_sampled(T, rw, fl)
    torch.cuda.synchronize()
    st, sc, total, _ = oracle.rollout(key, B, T, flavor=oracle.MATH_POLY, nthreads=8)
    assert np.array_equal(env.get_state().cpu().numpy().view(np.uint32), st.view(np.uint32))
    assert np.array_equal(env.current_step.cpu().numpy(), sc)
    L = ni._lib
    nv = int(((fl[:, :B] >> L.FLAG_NVIOL_SHIFT) & 3).sum().item())
    nc = int(((fl[:, :B] >> L.FLAG_NCRIT_SHIFT) & 3).sum().item())
    assert (nv, nc) == (total.violations, total.critical)
    assert int(env.tally[L.T_EPISODES].sum().item()) == total.episodes > 0
    env.close()


# ----------------------------------------------------------------------------------------- 3. sharding independence
@pytest.mark.parametrize("key", ["cr", "pg", "ra"])
def test_two_shards_produce_the_rows_of_one_handle(ni, key):
    """the action of (lane, t) depends on the lane's GLOBAL index: two handles of B/2 lanes with env_index0 = 0 and B/2 write
    the rows one handle of B lanes writes (whatever kernel form each of the three batches takes)"""
    ni.tune(split_blocks=-1, wide_min_blocks=-1)
    B, T = 2048, 40
    H = B // 2
    kw = dict(seed=77, autoreset=True, tally=True, max_episode_steps=11)
    whole = ni.make_batched(ENV_NAME[key], B, env_index0=0, **kw)
    lo, hi = ni.make_batched(ENV_NAME[key], H, env_index0=0, **kw), ni.make_batched(ENV_NAME[key], H, env_index0=H, **kw)
    outs = []
    for e in (whole, lo, hi):
        e.reset()
        rew, fl, obs = _bufs(e, T, "aos")
        e.rollout_sampled(T, rew, fl, obs)
        outs.append((rew[:, :e.batch], fl[:, :e.batch], obs))
    torch.cuda.synchronize()
    (rw, fw, ow), (rl, fll, ol), (rh, fh, oh) = outs
    assert torch.equal(_bits(rw), _bits(torch.cat([rl, rh], dim=1)))
    assert torch.equal(fw, torch.cat([fll, fh], dim=1))
    assert torch.equal(_bits(ow), _bits(torch.cat([ol, oh], dim=1)))
    assert torch.equal(_bits(whole.state_soa), _bits(torch.cat([lo.state_soa, hi.state_soa], dim=1)))
    assert torch.equal(whole.ctr, torch.cat([lo.ctr, hi.ctr]))
    assert int(whole.tally[ni._lib.T_EPISODES].sum().item()) > 0
    for e in (whole, lo, hi):
        e.close()


# ----------------------------------------------------------------------------------------- 4. no ring-sized allocation
@pytest.mark.parametrize("key,B,T", [("pg", 16384, 128), ("cr", 65536, 128)])
def test_no_ring_sized_allocation(ni, key, B, T):
    """The measure of tests/test_gpu_action_layout.py, restated: the drop of the device's free memory (it sees the library's own
    hipMallocs too) across two rollout_sampled calls, every buffer of the test allocated beforehand.  The ring an equivalent
    nig_rollout needs -- one slot per step -- is T x A x ld x 4 bytes, at least 64 MiB here; the drop must stay below half of it."""
    ni.tune(split_blocks=-1, wide_min_blocks=-1)
    env = ni.make_batched(ENV_NAME[key], B, autoreset=True, tally=True)
    ring_bytes = T * env.action_dim * env.ld * 4
    assert ring_bytes >= (64 << 20)
    env.reset()
    outs = [_bufs(env, T, "aos"), _bufs(env, T, "min")]
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for rew, fl, obs in outs:
        env.rollout_sampled(T, rew, fl, obs)
        torch.cuda.synchronize()
    used = free0 - torch.cuda.mem_get_info()[0]
    print(f"{ENV_NAME[key]}: free memory dropped by {used} bytes across two sampled calls; an equivalent ring is {ring_bytes} bytes")
    assert used < ring_bytes // 2, (used, ring_bytes)
    assert env.counter == 2 * T and not bool((outs[1][1][:, :B] == CANARY_I).any())
    env.close()


# ----------------------------------------------------------------------------------------- 5. refusals
def test_refusals_match_nig_rollout_and_write_nothing(ni):
    """every argument check of nig_rollout that does not concern the ring: the same error code, a message naming the check, no
    launch (the canary buffer and the handle are untouched, the counter does not move)"""
    ni.tune(split_blocks=-1, wide_min_blocks=-1)
    B, T = 1024, 8
    env = ni.make_batched("ChemicalReactor-v0", B, autoreset=True, tally=True)
    env.reset()
    L, S, ld, st = env._L, env.state_dim, env.ld, env._stream()
    ring = torch.zeros(T, env.action_dim, ld, dtype=torch.float32, device=env.device)
    canary = torch.full((T * S * ld + 64,), CANARY_F, dtype=torch.float32, device=env.device)
    p = canary.data_ptr()
    state0, ctr0 = env.state_soa.clone(), env.ctr.clone()
    vp = C.c_void_p
    rew, fl, obs = vp(p), vp(p + 4 * T * ld), vp(p)
    cases = [   # (what, n_steps, reward, flags, out_stride, obs, ld_obs, obs_step_stride, fragment of the message)
        ("n_steps <= 0", 0, rew, fl, ld, None, 0, 0, b"bad argument"),
        ("n_steps < 0", -3, rew, fl, ld, None, 0, 0, b"bad argument"),
        ("reward without flags", T, rew, None, ld, None, 0, 0, b"go together"),
        ("flags without reward", T, None, fl, ld, None, 0, 0, b"go together"),
        ("observations without reward", T, None, None, 0, obs, ld, S * ld, b"needs reward_out"),
        ("out_stride below the batch", T, rew, fl, B - 1, None, 0, 0, b"out_stride"),
        ("ld_obs below the batch", T, rew, fl, ld, obs, B - 1, S * ld, b"observation trajectory pitch"),
        ("obs_step_stride below one [S][ld_obs] block", T, rew, fl, ld, obs, ld, S * ld - 1, b"observation trajectory pitch"),
        ("row-major trajectory off 16-byte alignment", T, rew, fl, ld, vp(p + 4), 0, S * B, b"row-major trajectory"),
        ("row-major obs_step_stride not a multiple of 4", T, rew, fl, ld, obs, 0, S * B + 2, b"row-major trajectory"),
    ]

    def both(n, r, f, os_, o, ldo, so):
        rc_s = L.nig_rollout_sampled(env._h, n, r, f, os_, o, ldo, so, st)
        msg_s = L.nig_last_error()
        rc_r = L.nig_rollout(env._h, n, vp(ring.data_ptr()), ld, env.action_dim * ld, T, r, f, os_, o, ldo, so, st)
        return rc_s, msg_s, rc_r, L.nig_last_error()
    for what, n, r, f, os_, o, ldo, so, frag in cases:
        rc_s, msg_s, rc_r, msg_r = both(n, r, f, os_, o, ldo, so)
        assert rc_s == rc_r != 0, (what, rc_s, rc_r)
        assert frag in msg_s and msg_s == msg_r, (what, msg_s, msg_r)
        assert env.counter == 0, what
    env.counter = 0xFFFFFFF0                        # the launch counter would wrap
    rc_s, msg_s, rc_r, msg_r = both(32, rew, fl, ld, None, 0, 0)
    assert rc_s == rc_r != 0 and b"wrap" in msg_s and msg_s == msg_r
    assert env.counter == 0xFFFFFFF0
    env.counter = 0
    torch.cuda.synchronize()
    assert bool((canary == CANARY_F).all()), "a refused call wrote to its output buffer"
    assert torch.equal(_bits(env.state_soa), _bits(state0)) and torch.equal(env.ctr, ctr0)
    # the method refuses what the ring-fed method refuses, before the library is asked
    with pytest.raises(AssertionError):
        env.rollout_sampled(T, torch.zeros(T, ld, device=env.device), None)
    # ... and the good call goes through
    assert L.nig_rollout_sampled(env._h, T, rew, fl, ld, None, 0, 0, st) == 0
    torch.cuda.synchronize()
    assert env.counter == T and not bool((canary[:T * ld].view(T, ld)[:, :B] == CANARY_F).any())
    env.close()


# ----------------------------------------------------------------------------------------- 6. reference statistics
MAX_STEPS = {"cr": 500, "pg": 1000, "ra": 1000}
STAT_CASES = {"cr": (65536, 16, "split_rollout_kernel<ChemicalReactor,1,4>"),          # sizes and K of tests/test_gpu_reference_stats.py
              "pg": (262144, 4, "rollout_wide_kernel<PowerGrid,1,512>"),
              "ra": (65536, 16, "split_rollout_kernel<RobotAssembly,1,4>")}


@pytest.mark.parametrize("key", ["cr", "pg", "ra"])
def test_sampled_path_statistics_match_the_reference(ni, key):
    """uniform_action_statistics(action_source="generated"): no ring, no fill launches, rollout_sampled -- every statistic of the
    first K episodes of every lane within refstats.NSIGMA combined standard errors of the reference's own sample
    (tests/golden/reference_stats.npz), as tests/test_gpu_reference_stats.py asks of the ring-fed path."""
    ni.tune(split_blocks=-1, wide_min_blocks=-1)
    B, K, kernel = STAT_CASES[key]
    assert _kernel(ni, key, B, "min") == kernel                         # the form the ring-fed twin of this workload takes
    s = ni.uniform_action_statistics(ENV_NAME[key], B, K, action_source="generated")
    n = s["episodes"]
    assert n == B * K >= 1_000_000 and int(s["hist"].sum()) == n and int((s["hist"] * np.arange(s["hist"].size)).sum()) == s["steps"]
    table, th = refstats.reference_table(key, MAX_STEPS[key])
    cdf = np.cumsum(s["hist"]) / n
    got = {"length_mean": s["steps"] / n, "violations_per_episode": s["viol"] / n, "critical_per_episode": s["crit"] / n,
           "return_mean": s["ret"] / n, "p_terminated": s["term"] / n, "p_truncated": s["trunc"] / n,
           "p_critical_shutdown": s["shut"] / n}
    for k in range(3):
        got[f"constraint{k}_violated_steps_per_episode"] = s[f"c{k}"] / n
    for t in th:
        got[f"p_length_le_{t}"] = float(cdf[t])
    rows, bad = refstats.compare(table, got, n)
    print(f"\n{ENV_NAME[key]}: {n} episodes ({B} lanes x first {K}), {s['launches']} sampled launches of 250 steps")
    print(refstats.format_rows(rows))
    assert len(rows) == len(got) >= 14
    assert not bad, "sampled-path statistics off the reference's by more than %g standard errors:\n%s" % (refstats.NSIGMA, refstats.format_rows(bad))
