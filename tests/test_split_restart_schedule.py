"""not-gpu: the restart schedule of tests/test_gpu_split_restart.py (tests/split_restart_plan.py) run through the CPU oracle
alone.  The oracle, stepped one step at a time on the injected counters, must finish exactly the planned lanes at exactly the
planned steps, every one by truncation, and no lane on its own account -- so the GPU test, which compares the device with the
oracle, cannot pass for the wrong reason (a natural termination that hides or adds a finisher)."""
import numpy as np
import pytest

import split_restart_plan as plan

CASES = [(256, 0, 0x5EED), (512, 3 * 65536 + 512, 0xABCDEF)]          # (lanes, env_index0, seed): the GPU test's cases


@pytest.mark.parametrize("B,env0,seed", CASES)
def test_oracle_finishes_exactly_the_planned_lanes(oracle, B, env0, seed):
    O = oracle
    st0, sc0, _, _ = O.rollout("cr", B, 0, seed=seed, env0=env0)
    assert (sc0 == 0).all()
    st, sc = st0, plan.counters(B)
    want = plan.did_reset_rows(B)
    eps = np.zeros(B, dtype=np.int64)
    for i in range(plan.T):
        st, sc_new, total, tl = O.rollout("cr", B, 1, seed=seed, env0=env0, t0=i, state=st, step=sc, per_env=True)
        fin = np.array([t.episodes for t in tl]) == 1
        trunc = np.array([t.truncated for t in tl]) == 1
        term = np.array([t.terminated for t in tl]) == 1
        assert np.array_equal(fin, want[i]), "step %d: finishers %s, planned %s" % (i + 1, np.flatnonzero(fin), np.flatnonzero(want[i]))
        assert np.array_equal(trunc, fin) and not term.any()          # every planned finish is a truncation at max_episode_steps
        assert np.array_equal(sc_new, np.where(fin, 0, sc + 1))
        eps += fin
        sc = sc_new
    assert int(eps.sum()) == plan.PER_BLOCK * (B // 256) and eps.max() == 1
    assert np.array_equal(sc, plan.counters_after(B))
    # per wave and block: 13 lone finishes, the 2 + 3 + 33 of the list path, nobody, everybody
    per_wave = eps.reshape(-1, 4, 64).sum(axis=2)
    assert (per_wave == np.array([13, 38, 0, 64])).all()
    assert (want[:, :64].sum(axis=1) == 1).all()                      # wave 0: exactly one finisher in every step
    # the same rollout in one call: the chained steps are the oracle's own 13-step run
    st1, sc1, total1, tl1 = O.rollout("cr", B, plan.T, seed=seed, env0=env0, state=st0, step=plan.counters(B), per_env=True)
    assert np.array_equal(st1.view(np.uint32), st.view(np.uint32)) and np.array_equal(sc1, sc)
    assert np.array_equal(np.array([t.episodes for t in tl1]), eps) and total1.episodes == eps.sum()


def test_partial_launch_expectations():
    """the helpers the GPU test uses for launches of 6 + 7 and 1 + 12 steps"""
    B = 256
    full = plan.did_reset_rows(B)
    assert np.array_equal(np.concatenate([plan.did_reset_rows(B, 6), plan.did_reset_rows(B, 7, first=6)]), full)
    assert np.array_equal(np.concatenate([plan.did_reset_rows(B, 1), plan.did_reset_rows(B, 12, first=1)]), full)
    c6 = plan.counters_after(B, 6)
    k = plan.finish_step(B)
    assert (c6[(k > 0) & (k <= 6)] == 6 - k[(k > 0) & (k <= 6)]).all() and (c6[k > 6] == plan.MAX_STEPS - k[k > 6] + 6).all()
    assert (c6[k == 0] == 6).all()
