"""-m gpu: the three-wave rollout kernels decide a step's outcome ONCE (csrc/nig_split_body.inc): the integrator hands
`terminated` / `truncated` to the recorder in the word that carries the violation bits (outcome_word, csrc/nig_step.hpp), and the
recorder takes bits 2-9 of the flag word from a table indexed by the violation bits (post_record).  What can go wrong is an ending
the recorder no longer sees for itself: a critical shutdown (the uniform-action workload never produces one), the env's own done,
a truncation, both in one step -- and a table entry that is not what pack_flags packs.  So states are PLACED on every kind of
ending, one kind per lane of every group of eight (mixed within each wave), and the three-wave form runs against the one-wave
rollout_kernel on the same handle state: everything a rollout leaves behind bit-identical, and the first step's flag bits as
base.py defines them, from first principles.  Shapes: 256 and 512 lanes, at most 19 steps per launch."""
import numpy as np
import pytest
import torch

from conftest import ENV_NAME
from test_gpu_split_slots import KERNEL, _kernel, _same

pytestmark = pytest.mark.gpu

MAX_STEPS = 50


@pytest.fixture(scope="module")
def ni():
    import neorl_industrial_gym_amd as ni
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    yield ni
    ni.tune(split_blocks=-1, wide_min_blocks=-1)


def _roll(ni, split, key, B, chunks, outputs="aos", sampled=False, max_steps=MAX_STEPS, first_counter=0, place=None, seed=11):
    """test_gpu_split_slots._run with a hook: place(env) -> (state [B, S], current_step [B]) puts the lanes where the test wants
    them after the reset.  Returns every observable as CPU tensors: per launch reward, flags, rows; then state, counter words,
    lifetime violations, running returns, tally."""
    ni.tune(split_blocks=256 if split else 0)
    if not sampled:
        want = ("split_rollout_kernel<%s,3,4>" if split else "rollout_kernel<%s,3>") % KERNEL[key]
        assert _kernel(ni, key, B) == want
    env = ni.make_batched(ENV_NAME[key], B, seed=seed, autoreset=True, tally=True, max_episode_steps=max_steps)
    ring = None
    if not sampled:
        ring = torch.empty(7, env.action_dim, env.ld, dtype=torch.float32, device=env.device)
        for s in range(7):
            env.fill_actions(70 + s, ring[s])
    env.reset()
    if place is not None:
        state, steps = place(env)
        env.set_state(state, current_step=steps)
    env.counter = first_counter
    got = []
    for T in chunks:
        rew = fl = obs = None
        if outputs != "none":
            rows = () if outputs == "last" else (T,)
            rew = torch.full(rows + (env.ld,), float("nan"), dtype=torch.float32, device=env.device)
            fl = torch.zeros(rows + (env.ld,), dtype=torch.int32, device=env.device)
        if outputs == "aos":
            obs = torch.full((T, B, env.state_dim), float("nan"), dtype=torch.float32, device=env.device)
        if sampled:
            env.rollout_sampled(T, rew, fl, obs)
        else:
            env.rollout(T, ring, rew, fl, obs)
        torch.cuda.synchronize()
        got += [t.cpu() if t is obs else t[..., :B].cpu() for t in (rew, fl, obs) if t is not None]
    got += [env.state_soa.cpu(), env.ctr.cpu(), env.life_viol.cpu(), env.ep_return.cpu(), env.tally.cpu()]
    env.close()
    return got


def _fields(L, vb, crit_mask=3):
    """bits 2-9 of the flag word as pack_flags packs them from what post_finish makes of the violation bits `vb`"""
    nviol, ncrit = bin(vb).count("1"), bin(vb & crit_mask).count("1")
    return (vb << L.FLAG_VIOL_SHIFT) | (nviol << L.FLAG_NVIOL_SHIFT) | (ncrit << L.FLAG_NCRIT_SHIFT) | (L.FLAG_SHUTDOWN if ncrit else 0)


# ---- placed states ------------------------------------------------------------------------------------------------------------
# ChemicalReactor (csrc/nig_envs.hpp): state = T, P, coolant, feed, conc, catalyst, hx, relief, estop, alarm, level, batch time.
# Violations on the PRE-state: T > 350 (bit 0, critical), P > 506 625 (bit 1, critical), level outside [20, 90] (bit 2).
# done on the NEXT state: estop > 0.5, level < 5 or > 95, batch time > 50.  A reset state has T = 320 +- 11, P = 253 312 +- 54 200,
# level = 60 +- 27, feed = 30 +- 16 (|z| <= 5.42), everything else at rest: no violation and no done within one step.
def _cr_endings(env):
    B = env.batch
    st = env.get_state().cpu().numpy().copy()
    steps = np.zeros(B, dtype=np.int64)
    g = np.arange(B) % 8
    st[g == 0, 0] = 351.0                      # critical constraint 0 -> shutdown
    st[g == 1, 1] = 510000.0                   # critical constraint 1 -> shutdown
    st[g == 2, 10] = 95.5                      # level: violated (> 90) and, a step later (+- 0.07), still > 95: done
    st[g == 3, 8] = 1.0                        # estop
    st[g == 4, 11] = 49.95                     # batch time: 50.05 after the step
    steps[g == 5] = MAX_STEPS - 1              # truncation
    steps[g == 6] = MAX_STEPS - 1              # truncation and termination in one step
    st[g == 6, 8] = 1.0
    return st, steps                           # g == 7: none of these


#            terminated, truncated, shutdown, violation bits
CR_EXPECT = [(1, 0, 1, 1), (1, 0, 1, 2), (1, 0, 0, 4), (1, 0, 0, 0), (1, 0, 0, 0), (0, 1, 0, 0), (1, 1, 0, 0), (0, 0, 0, 0)]


def _cr_all_vb(env):
    B = env.batch
    st = env.get_state().cpu().numpy().copy()
    vb = np.arange(B) % 8
    st[(vb & 1) != 0, 0] = 351.0
    st[(vb & 2) != 0, 1] = 510000.0
    st[(vb & 4) != 0, 10] = 92.0
    return st, np.zeros(B, dtype=np.int64)


# RobotAssembly: state = position (0-2), 3-6 fixed, joints (7-13), velocity (14-17), force (18-20), align, depth, align * depth.
# Violations on the PRE-state: a force component >= 50 (bit 0, critical), position outside [-0.5, 0.5]^2 x [0, 0.8] (bit 1,
# critical), a joint value >= 2 (bit 2).  done on the NEXT state: the position -- forward kinematics of the joints, links
# 0.3 0.3 0.25 0.25 0.15 0.1 0.05, even joints -> x, z, odd joints -> y -- outside [-0.6, 0.6]^2 x [-0.1, 0.9] (also n[23] > 0.95
# and a force above 80, which the dynamics never produce from these states).  Base state: even joints 1.0, odd joints 0.5
# (+- 0.1 after one action) -> x in [0.34, 0.47], y in [0.25, 0.37], z in [0.59, 0.67]: inside, far from the target, no force.
def _ra_base(B):
    st = np.zeros((B, 24), dtype=np.float32)
    st[:, 0:3] = (0.4, 0.3, 0.6)
    st[:, 6] = 1.0
    st[:, 7:14:2] = 1.0
    st[:, 8:14:2] = 0.5
    return st


def _ra_endings(env):
    B = env.batch
    st = _ra_base(B)
    steps = np.zeros(B, dtype=np.int64)
    g = np.arange(B) % 8
    st[g == 0, 18] = 60.0                      # critical constraint 0 (force) -> shutdown
    st[g == 1, 0] = 0.55                       # critical constraint 1 (workspace) -> shutdown
    st[g == 2, 7] = 2.5                        # joint limit: violated, not critical; x = 0.3 cos 2.5 + 0.45 cos 1 ~ 0: no done
    for k in (3, 4, 6):                        # the env's own done: even joints 0 -> x = 0.75 cos(<= 0.1) > 0.6
        for j in (7, 9, 11, 13):
            st[g == k, j] = 0.0
    st[g == 4, 8] = 2.5                        # ... with a non-critical violation
    steps[g == 5] = MAX_STEPS - 1              # truncation
    steps[g == 6] = MAX_STEPS - 1              # truncation and termination in one step
    return st, steps


RA_EXPECT = [(1, 0, 1, 1), (1, 0, 1, 2), (0, 0, 0, 4), (1, 0, 0, 0), (1, 0, 0, 4), (0, 1, 0, 0), (1, 1, 0, 0), (0, 0, 0, 0)]


def _ra_all_vb(env):
    B = env.batch
    st = _ra_base(B)
    vb = np.arange(B) % 8
    st[(vb & 1) != 0, 18] = 60.0
    st[(vb & 2) != 0, 0] = 0.55
    st[(vb & 4) != 0, 7] = 2.5
    return st, np.zeros(B, dtype=np.int64)


ENDINGS = {"cr": (_cr_endings, CR_EXPECT), "ra": (_ra_endings, RA_EXPECT)}
ALL_VB = {"cr": _cr_all_vb, "ra": _ra_all_vb}


@pytest.mark.parametrize("B", [256, 512])
@pytest.mark.parametrize("key", ["cr", "ra"])
def test_every_kind_of_ending(ni, key, B):
    """Cases 1 and 3: one kind of ending per lane of every group of eight; two chained launches (3 and 4 steps) from launch
    counters 0 and 1, against the one-wave form, and the first step's terminated / truncated / shutdown / violation bits per group
    from first principles.  The critical lanes must show up in the tally's critical and shutdown rows."""
    L = ni._lib
    place, expect = ENDINGS[key]
    for first_counter in (0, 1):
        kw = dict(key=key, B=B, chunks=[3, 4], place=place, first_counter=first_counter)
        a = _roll(ni, True, **kw)
        _same(a, _roll(ni, False, **kw), f"{key} B={B} endings from {first_counter}")
        fl = a[1][0].numpy().astype(np.int64)                 # flags of the first launch, first step
        for g, (term, trunc, shut, vb) in enumerate(expect):
            w = fl[g::8]
            print(f"{key} B={B} from {first_counter} group {g}: flag words {sorted(set(hex(int(x)) for x in w))}")
            assert np.all((w & L.FLAG_TERMINATED != 0) == bool(term)), (key, g, "terminated")
            assert np.all((w & L.FLAG_TRUNCATED != 0) == bool(trunc)), (key, g, "truncated")
            assert np.all((w & L.FLAG_SHUTDOWN != 0) == bool(shut)), (key, g, "shutdown")
            assert np.all(((w >> L.FLAG_VIOL_SHIFT) & 7) == vb), (key, g, "violation bits")
            assert np.all((w & L.FLAG_DID_RESET != 0) == bool(term or trunc)), (key, g, "did_reset")
            assert np.all((w >> L.FLAG_STEP_SHIFT) == (MAX_STEPS if trunc else 1)), (key, g, "step")
        tally = a[-1]
        assert int(tally[L.T_SHUTDOWN].sum().item()) >= B // 4 and int(tally[L.T_CRIT].sum().item()) >= B // 4


@pytest.mark.parametrize("B", [256, 512])
@pytest.mark.parametrize("key", ["cr", "ra"])
def test_all_eight_violation_patterns(ni, key, B):
    """Cases 2 and 3: lane l starts with violation pattern l mod 8 (each of the three constraints in or out of its limit);
    bits 2-9 of the first step's flag word must be what pack_flags packs (include/nig.h), and everything equals the one-wave form."""
    L = ni._lib
    for first_counter in (0, 1):
        kw = dict(key=key, B=B, chunks=[2, 3], place=ALL_VB[key], first_counter=first_counter)
        a = _roll(ni, True, **kw)
        _same(a, _roll(ni, False, **kw), f"{key} B={B} patterns from {first_counter}")
        fl = a[1][0].numpy().astype(np.int64)
        for vb in range(8):
            got = fl[vb::8] & 0x3FC
            print(f"{key} B={B} from {first_counter} vb {vb}: bits 2-9 {sorted(set(hex(int(x)) for x in got))}, want {hex(_fields(L, vb))}")
            assert np.all(got == _fields(L, vb)), (key, vb)
            assert np.all((fl[vb::8] & L.FLAG_TERMINATED != 0) | ((vb & 3) == 0))      # a critical violation terminates


@pytest.mark.parametrize("n_steps", [1, 5, 6, 7, 13, 19])
@pytest.mark.parametrize("sampled", [False, True], ids=["ring", "sampled"])
@pytest.mark.parametrize("key", ["cr", "ra"])
def test_chained_launches_equal_the_one_wave_form(ni, key, sampled, n_steps):
    """Case 4: two chained launches of n_steps, 5-step episodes (truncations and resets in the unrolled iterations and in the
    tails), 256 and 512 lanes, from launch counters 0 and 1 for ChemicalReactor, outputs aos / last / none."""
    for outputs in ("aos", "last", "none"):
        for B in (256, 512):
            for first_counter in ((0, 1) if key == "cr" else (0,)):
                kw = dict(key=key, B=B, chunks=[n_steps, n_steps], outputs=outputs, sampled=sampled, max_steps=5, first_counter=first_counter)
                _same(_roll(ni, True, **kw), _roll(ni, False, **kw), f"{key} B={B} {outputs} n={n_steps} from {first_counter}")


def test_recorded_draws_instantiation(ni):
    """Case 4, the NOISE instantiation of the same body (recorded step and reset draws), once: the check of
    tests/test_gpu_split_slots.py, against step_kernel's parity mode."""
    from test_gpu_split_slots import test_recorded_draws_equal_the_parity_step_kernel as check
    check(ni)
