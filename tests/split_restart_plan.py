"""The restart schedule shared by tests/test_split_restart_schedule.py (oracle alone) and tests/test_gpu_split_restart.py.

ChemicalReactor lanes are made to finish (truncate) at chosen local steps by injecting step counters: with
max_episode_steps = 500, a lane whose counter starts at 500 - k finishes at local step k; every other lane starts at 0.
Per 256-lane block (four wave triples of the three-wave form, csrc/nig_split.hpp):

    wave 0   lane (5 k mod 64) finishes at step k, k = 1 .. 13: ONE finisher per step -- the lone-finisher path of
             coop_reset (csrc/nig_step.hpp) at every position of the integrator's unrolled loop, in its tail, back to back
    wave 1   lanes 0 and 63 at step 2, lanes 1-3 at step 3, lanes 4-36 at step 5 (33 finishers x 2 items = 66 > 64: two
             passes of the item loop): the work-list path
    wave 2   nobody
    wave 3   all 64 lanes at step 7
"""
import numpy as np

MAX_STEPS = 500
T = 13
PER_BLOCK = 13 + 2 + 3 + 33 + 64          # planned episodes per 256-lane block


def finish_step(B):
    """int32 [B]: the local step (1 .. T) at which the lane is planned to finish, 0 = never."""
    assert B % 256 == 0
    k = np.zeros(B, dtype=np.int32)
    for o in range(0, B, 256):
        for s in range(1, T + 1):
            k[o + (5 * s) % 64] = s
        k[o + 64 + 0] = k[o + 64 + 63] = 2
        k[o + 64 + 1:o + 64 + 4] = 3
        k[o + 64 + 4:o + 64 + 37] = 5
        k[o + 192:o + 256] = 7
    assert int((k > 0).sum()) == PER_BLOCK * (B // 256)
    return k


def counters(B):
    """int32 [B]: the injected step counters."""
    k = finish_step(B)
    return np.where(k > 0, MAX_STEPS - k, 0).astype(np.int32)


def did_reset_rows(B, n_steps=T, first=0):
    """bool [n_steps, B]: row i is local step first + i + 1; True where the lane is planned to finish at that step."""
    k = finish_step(B)
    return np.stack([k == first + i + 1 for i in range(n_steps)])


def counters_after(B, n_steps=T):
    """int32 [B]: the step counters after n_steps local steps, if exactly the planned episodes finish."""
    k = finish_step(B)
    c = counters(B) + n_steps
    return np.where((k > 0) & (k <= n_steps), n_steps - k, c).astype(np.int32)
