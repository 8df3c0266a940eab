"""not-gpu: the per-episode state machine (csrc/nig_episodes.hpp episode_row -- the code collect_episodes_kernel runs) called on
the host through tests/episodes_probe.cpp, built with the host compiler, against its NumPy restatement
(episodes.episodes_from_rows), bit for bit, returns included; both against the reference's recorded rollouts
(tests/golden/<env>_g3.npz); the counting rule k * B + i < n_episodes and the log layout."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden

CANARY = 0x5A5A5A5B
CSRC = os.path.join(ROOT, "neorl-industrial-gym_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "episodes_probe.cpp")


def _cxx():
    cxx = next((c for c in (os.environ.get("CXX"), shutil.which("c++"), shutil.which("g++"), shutil.which("clang++")) if c), None)
    assert cxx, "no host C++ compiler: the probe is the library's own header, compiled for the host"
    return cxx


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("episodes") / "episodes_probe"
    # -ffp-contract=off as the library's build; the state machine has no product to fuse, the flag keeps it that way
    subprocess.run([_cxx(), "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC, "-o", str(exe), SRC], check=True)

    def run(text):
        out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        return out.stdout.splitlines()
    return run


@pytest.fixture(scope="module")
def ni():
    import neorl_industrial_gym_amd as ni
    return ni


def _probe_rows(probe, reward, flags, ret_f32, K, cuts):
    """The probe on rows [T, B], cut in two calls at every position of `cuts`: one episodes_from_rows-shaped dict per cut."""
    T, B = reward.shape
    rb, fb = reward.astype(np.float32).view(np.uint32), flags.astype(np.uint32)
    text = "R %d %d %d %d %x %d %s\n" % (T, B, K, int(ret_f32), CANARY, len(cuts), " ".join(str(c) for c in cuts))
    text += "\n".join(" ".join("%x %x" % (rb[t, i], fb[t, i]) for i in range(B)) for t in range(T)) + "\n"
    lines = probe(text)
    per = 1 + K + 5 * K + 1 + 4
    assert len(lines) == per * len(cuts)
    out = []
    for c in range(len(cuts)):
        blk = [[int(x, 16) for x in l.split()] for l in lines[c * per:(c + 1) * per]]
        u32 = lambda rows: np.array(rows, dtype=np.uint64).astype(np.uint32)                    # noqa: E731
        f64 = lambda rows: np.array(rows, dtype=np.uint64).view(np.float64)                     # noqa: E731
        out.append({"count": u32(blk[0]), "ret": f64(blk[1:1 + K]).reshape(K, B), "w": u32(blk[1 + K:1 + 6 * K]).reshape(5, K, B),
                    "carry_ret": f64(blk[1 + 6 * K]), "carry_w": u32(blk[2 + 6 * K:6 + 6 * K]).reshape(4, B)})
    return out


def _same_log(got, want, K, canary=None):
    """count, carry and every record a lane has, as bits; with `canary`: every other record word of `got` still holds it."""
    assert np.array_equal(got["count"], want["count"])
    assert np.array_equal(got["carry_ret"].view(np.uint64), want["carry_ret"].view(np.uint64))
    assert np.array_equal(got["carry_w"], want["carry_w"])
    have = np.arange(K)[:, None] < np.minimum(want["count"].astype(np.int64), K)[None, :]
    assert np.array_equal(got["ret"].view(np.uint64)[have], want["ret"].view(np.uint64)[have])
    for j in range(5):
        assert np.array_equal(got["w"][j][have], want["w"][j][have]), j
    if canary is not None:
        assert np.all(got["ret"].view(np.uint64)[~have] == ((canary << 32) | canary))
        assert np.all(got["w"][:, ~have] == canary)


def synthetic_rows(L, T=48, B=9, seed=7):
    """Rows that visit every branch of the state machine: lane 0 finishes on every step (length-1 episodes, far more than any
    small capacity); lane 1 episodes of length 5; lane 2 one episode of 20 steps, then frozen (INACTIVE rows with a reward that
    must not be added); lane 3 the Advanced envs' words (NVIOL_HI, VIOL3); lane 4 SHIELDED / UNCERTAIN steps; lane 5 never
    finishes (everything stays in the carry); the others finish at random.  Rewards of magnitude up to 1e3 with 24 random
    mantissa bits: their float32 and float64 sums differ after a few steps."""
    rng = np.random.default_rng(seed)
    reward = ((rng.random((T, B)) - 0.3) * 1000.0).astype(np.float32)
    flags = np.zeros((T, B), np.uint32)
    step = np.zeros(B, np.int64)
    frozen = np.zeros(B, bool)
    for t in range(T):
        for i in range(B):
            if frozen[i]:
                flags[t, i] = L.FLAG_INACTIVE | (int(step[i]) << L.FLAG_STEP_SHIFT) | L.FLAG_TERMINATED      # the done bit of a frozen row is ignored too
                continue
            step[i] += 1
            nv = int(rng.integers(0, 4))
            bits = int(rng.integers(0, 8)) << L.FLAG_VIOL_SHIFT
            f = (int(step[i]) << L.FLAG_STEP_SHIFT) | (nv << L.FLAG_NVIOL_SHIFT) | bits
            if i == 3:
                f |= (L.FLAG_NVIOL_HI if rng.random() < 0.5 else 0) | (L.FLAG_VIOL3 if rng.random() < 0.5 else 0)
            if i == 4:
                f |= (L.FLAG_SHIELDED if rng.random() < 0.5 else 0) | (L.FLAG_UNCERTAIN if rng.random() < 0.3 else 0)
            done = {0: True, 1: step[i] == 5, 2: step[i] == 20, 5: False}.get(i, rng.random() < 0.15)
            if done:
                crit = int(rng.integers(0, 3))
                f |= (L.FLAG_TERMINATED if (crit or rng.random() < 0.5) else L.FLAG_TRUNCATED) | (crit << L.FLAG_NCRIT_SHIFT)
                f |= L.FLAG_SHUTDOWN if crit else 0
                f |= L.FLAG_DID_RESET if i != 2 else 0
                frozen[i] = i == 2
                if i != 2:
                    step[i] = 0
            flags[t, i] = f
    return reward, flags


@pytest.mark.parametrize("ret_f32", [True, False])
def test_probe_equals_numpy_restatement_at_every_cut(probe, ni, ret_f32):
    L = ni._lib
    K = 3
    reward, flags = synthetic_rows(L)
    T, B = reward.shape
    whole = ni.episodes_from_rows(reward, flags, ret_f32, K)
    # the rows do what their docstring says
    assert whole["count"][0] == T > K and whole["count"][1] == T // 5 and whole["count"][2] == 1 and whole["count"][5] == 0
    assert whole["carry_w"][0, 5] > 0 and whole["carry_ret"][5] != 0.0
    assert (whole["w"][0, 0, 2] & L.CTR_STEP_MASK) == 20 and (whole["w"][0, 0, 1] & L.CTR_STEP_MASK) == 5
    assert np.all(whole["w"][0, :, 0] & L.CTR_STEP_MASK == 1) and np.all(whole["w"][0, :, 0] & L.CTR_DONE != 0)
    assert whole["w"][3, :, 3].max() >> 16 > 0 and (whole["w"][0, :, 3] >> 16).max() > 3 * 5      # VIOL3 steps; NVIOL_HI adds 4
    assert (whole["w"][4, :, 4] & 0xFFFF).max() > 0 and (whole["w"][4, :, 4] >> 16).max() > 0
    assert whole["w"][4][:, [0, 1, 2, 3]].max() == 0
    cuts = list(range(T + 1))
    got = _probe_rows(probe, reward, flags, ret_f32, K, cuts)
    for c, g in zip(cuts, got):
        _same_log(g, whole, K, canary=CANARY)
        first = ni.episodes_from_rows(reward[:c], flags[:c], ret_f32, K)
        second = ni.episodes_from_rows(reward[c:], flags[c:], ret_f32, K, carry=first)
        _same_log(second, whole, K)
        assert np.array_equal(second["ret"].view(np.uint64), whole["ret"].view(np.uint64)) and np.array_equal(second["w"], whole["w"])


def test_float32_and_float64_accumulation_differ_on_these_rows(ni):
    reward, flags = synthetic_rows(ni._lib)
    a = ni.episodes_from_rows(reward, flags, True, 3)
    b = ni.episodes_from_rows(reward, flags, False, 3)
    assert np.array_equal(a["count"], b["count"]) and np.array_equal(a["w"], b["w"])
    longer = (a["w"][0] & ni._lib.CTR_STEP_MASK) > 3
    assert longer.any() and np.any(a["ret"][longer] != b["ret"][longer])
    assert np.array_equal(a["ret"], a["ret"].astype(np.float32).astype(np.float64))          # a float32 return, widened
    one = (a["w"][0] & ni._lib.CTR_STEP_MASK) == 1
    assert np.array_equal(a["ret"][one], b["ret"][one])                                         # one reward: nothing to round


@pytest.mark.parametrize("key", ["cr", "pg", "ra"])
def test_against_the_reference_recorded_rollouts(probe, ni, key):
    """Flag words built from the per-step outcomes the reference recorded, one of the 64 episodes per lane, frozen after its
    end: lengths, violation counts, critical counts and end kinds per episode exact; ChemicalReactor's returns bit-equal to
    the sequential float32 sum of the recorded float32 rewards (what utils.py:99 computes under NumPy 2)."""
    L = ni._lib
    d = load_golden(key, "g3")
    E = len(d["ep_length"])
    assert E == 64
    off, T = d["ep_offsets"], int(d["ep_length"].max()) + 2
    reward = np.full((T, E), 123.0, np.float32)
    flags = np.zeros((T, E), np.uint32)
    for e in range(E):
        n = int(d["ep_length"][e])
        j = slice(off[e], off[e] + n)
        reward[:n, e] = d["reward"][j].astype(np.float32)
        f = (np.arange(1, n + 1, dtype=np.uint32) << L.FLAG_STEP_SHIFT) | (d["viol"][j].astype(np.uint32) << L.FLAG_NVIOL_SHIFT) \
            | (d["crit"][j].astype(np.uint32) << L.FLAG_NCRIT_SHIFT) | np.where(d["terminated"][j] != 0, L.FLAG_TERMINATED, 0).astype(np.uint32) \
            | np.where(d["truncated"][j] != 0, L.FLAG_TRUNCATED, 0).astype(np.uint32) | np.where(d["crit"][j] > 0, L.FLAG_SHUTDOWN, 0).astype(np.uint32)
        flags[:n, e] = f
        flags[n:, e] = L.FLAG_INACTIVE | (n << L.FLAG_STEP_SHIFT)
    ret_f32 = key == "cr"
    if ret_f32:
        assert np.array_equal(d["reward"].astype(np.float32).astype(np.float64), d["reward"])    # the recorded rewards ARE float32
    rec = ni.episodes_from_rows(reward, flags, ret_f32, 1)
    got = _probe_rows(probe, reward, flags, ret_f32, 1, [0, T // 2])
    for g in got:
        _same_log(g, rec, 1, canary=CANARY)
    assert np.all(rec["count"] == 1)
    w0, w1 = rec["w"][0, 0], rec["w"][1, 0]
    assert np.array_equal(w0 & L.CTR_STEP_MASK, d["ep_length"])
    assert np.array_equal(w0 >> L.CTR_VIOL_SHIFT, d["ep_viol"])
    assert np.array_equal((w1 >> L.FLAG_NCRIT_SHIFT) & 3, d["ep_crit"])
    assert np.array_equal((w1 & L.FLAG_SHUTDOWN) != 0, d["ep_shutdown"] > 0)
    last = off[1:] - 1
    assert np.array_equal((w1 & L.FLAG_TERMINATED) != 0, d["terminated"][last] != 0)
    assert np.array_equal((w1 & L.FLAG_TRUNCATED) != 0, d["truncated"][last] != 0)
    want = np.zeros(E)
    for e in range(E):
        acc = np.float32(0.0) if ret_f32 else 0.0
        for x in d["reward"][off[e]:off[e + 1]]:
            acc = np.float32(acc + np.float32(x)) if ret_f32 else acc + float(np.float32(x))
        want[e] = acc
    assert np.array_equal(rec["ret"][0].view(np.uint64), want.view(np.uint64))
    # and the reference's own episode_return: float32 arithmetic for ChemicalReactor, within the rounding of the stored float32
    # rewards (2^-24 relative each) for the float64 envs
    if ret_f32:
        assert np.array_equal(rec["ret"][0], d["ep_return"])
    else:
        bound = np.array([np.abs(d["reward"][off[e]:off[e + 1]]).sum() for e in range(E)]) * 2.0 ** -23
        assert np.all(np.abs(rec["ret"][0] - d["ep_return"]) <= bound)


@pytest.mark.parametrize("B,K", [(100, 3), (257, 3), (7, 5)])
def test_counting_rule_counts_exactly_n_episodes(probe, ni, B, K):
    from neorl_industrial_gym_amd.episodes import counted
    full = np.full(B, K + 2)                                  # every lane has (more than) its records
    ns = sorted({1, B - 1, B, B + 1, 2 * B + 5 if 2 * B + 5 <= K * B else K * B - 1, K * B})
    lines = probe("".join("C %d %d %d\n" % (B, K, n) for n in ns))
    for n, line in zip(ns, lines):
        m = counted(full, B, K, n)
        pairs, index_sum = (int(x) for x in line.split())
        assert m.sum() == n == pairs and index_sum == n * (n - 1) // 2          # exactly the indices 0 .. n-1 of k * B + i
        assert np.array_equal(np.flatnonzero(m.reshape(-1)), np.arange(n))      # a fixed count per lane: whole rows, then lanes [0, r)
        per_lane = m.sum(0)
        assert per_lane.max() - per_lane.min() <= 1 and np.all(np.diff(per_lane) <= 0)
    # a lane that has not finished its share is not counted for it
    short = full.copy(); short[0] = 1
    assert counted(short, B, K, K * B).sum() == K * B - (K - 1)


def test_layout_query_matches_the_header_and_refuses_bad_shapes(probe, ni):
    L = ni._lib
    for B, K, ld in [(100, 3, 0), (100, 3, 131), (257, 3, 0), (257, 1, 300), (65536, 4, 0)]:
        lay = L.episode_log_query(B, K, ld)
        got = [lay.batch, lay.capacity, lay.ld, lay.bytes, lay.off_ret, *lay.off_w, lay.off_count, lay.off_carry_ret, lay.off_carry_w,
               lay.off_tally, lay.off_scratch]
        assert got == [int(x) for x in probe("L %d %d %d\n" % (B, K, ld))[0].split()]
        assert lay.ld == (ld or -(-B // 64) * 64) and lay.bytes % 256 == 0
        offs = got[4:] + [lay.bytes]
        sizes = [K * lay.ld * 8] + [K * lay.ld * 4] * 5 + [lay.ld * 4, lay.ld * 8, 4 * lay.ld * 4, (L.T_ROWS + 1) * lay.ld * 8, 256 * L.T_ROWS * 8]
        assert all(a + s <= b and a % 8 == 0 for a, s, b in zip(offs[:-1], sizes, offs[1:]))
    out = L.EpisodeLogLayout()
    for B, K, ld, what in [(100, 0, 0, "capacity"), (100, -1, 0, "capacity"), (100, 3, 99, "ld"), (0, 3, 0, "batch"), (100, 2 ** 20 + 1, 0, "capacity")]:
        assert L.lib().nig_episode_log_query(B, K, ld, C.byref(out)) == 1
        assert what in L.lib().nig_last_error().decode()
    assert L.lib().nig_episode_log_query(100, 3, 0, None) == 1


def test_probe_runs_clean_under_address_and_undefined_sanitizers(tmp_path):
    """The state machine as a stand-alone host program (its own main, no Python) under -fsanitize=address,undefined.  The
    runtimes are linked statically where the compiler can, so the program does not depend on the order of the process's
    shared libraries."""
    exe = tmp_path / "episodes_probe_san"
    base = [_cxx(), "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
            "-I", CSRC, "-o", str(exe), SRC]
    for extra in (["-static-libasan", "-static-libubsan"], ["-static-libsan"], []):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        if r.returncode == 0:
            break
    if r.returncode != 0 and any(x in r.stderr for x in ("lasan", "lubsan", "libasan", "libubsan", "libclang_rt")):
        pytest.skip("the host compiler has no sanitizer runtimes")
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([str(exe), "--self"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("self-test ok"), out.stderr[-2000:]
