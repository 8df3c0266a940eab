"""not-gpu: the launch planner (csrc/nig_launch_plan.hpp) -- which kernel form every 256-lane block of a rollout launch runs --
called on the host through tests/launch_plan_probe.hip with the library's own traits (csrc/nig_launch.hpp PlanTraits) and
compared with the independent statements of the rule:
  (a) bench.rollout_kernel_name / bench.policy_kernel_name, the names the footprint tests expect on the GPU;
  (b) the plan's own shape: the segments cover the batch's blocks exactly once and in order, a ragged block and every block of
      a handle on which a lane can be frozen run the one-wave forms;
  (c) the row-major action ring's "read in place" answer (rollout_rows_native) against the predicate as it was written out before
      it became a question to the plan.
One host-only compile (hipcc --cuda-host-only, no device code, no device needed) and one run of the probe per module."""
import itertools
import os
import shutil
import subprocess
import types

import pytest

from conftest import ROOT

import bench

ENVS = {"cr": "ChemicalReactor", "pg": "PowerGrid", "ra": "RobotAssembly", "acr": "AdvancedChemicalReactor",
        "apg": "AdvancedPowerGrid", "hvac": "HVACControl", "water": "WaterTreatment", "steel": "SteelAnnealing",
        "supply": "SupplyChain"}
# ragged sizes, and whole-block sizes on both sides of: one round (1 / 4 / 8 blocks), a last round 3/4 full (7 of 4 + 4, 14 of
# 8 + 8, against 6 and 10), the closed loop's two-round cap (2 against 4 rounds of 1, 2 against 3 rounds of 4), 1 / 3 / 5 wide blocks
BATCHES = [1, 255, 256, 300, 512, 1024, 1280, 1536, 1792, 2048, 2304, 2597, 3072, 3584, 4096, 5000]
SPLIT_BLOCKS = [0, 1, 4, 8]
WIDE_MIN_BLOCKS = [0, 1, 3, 5, 2 ** 30]
OUTPUTS = {"none": 0, "min": 1, "full": 3}
HANDLES = ["plain", "noreset", "held"]
ONE_WAVE = ("one_wave_full", "one_wave_ragged")

ROLLOUT_CASES = list(itertools.product(ENVS, range(4), BATCHES, HANDLES, SPLIT_BLOCKS, WIDE_MIN_BLOCKS))
# ("rar": RobotAssembly's traits with SPLIT_ROUNDS on, as the diagnostic build with rounds has them)
POLICY_CASES = list(itertools.product(list(ENVS) + ["rar"], (1, 0), (1, 0), BATCHES, HANDLES, SPLIT_BLOCKS))


def _segments(words):
    """'<blocks covered> <form>:<block0>:<grid> ...' -> (blocks covered, [(form, block0, grid), ...])"""
    return int(words[0]), [(form, int(block0), int(grid)) for form, block0, grid in (w.split(":") for w in words[1:])]


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    hipcc = next((c for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc") if c and os.path.exists(c)), None)
    assert hipcc, "hipcc not found: the probe is the library's own header, compiled for the host"
    exe = tmp_path_factory.mktemp("launch_plan") / "launch_plan_probe"
    subprocess.run([hipcc, "--cuda-host-only", "-std=c++17", "-O1", "-w", "-I", os.path.join(ROOT, "neorl-industrial-gym_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), "-o", str(exe), os.path.join(ROOT, "tests", "launch_plan_probe.hip")], check=True)
    lines = [f"T {e}" for e in ENVS]
    lines += ["R %s %d %d %s %d %d" % c for c in ROLLOUT_CASES]
    lines += ["P %s %d %d %d %s %d" % c for c in POLICY_CASES]
    out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    got = out.stdout.splitlines()
    assert len(got) == len(lines)
    n = len(ENVS)
    traits = {}
    for e, l in zip(ENVS, got[:n]):
        wide, A, pair, pair_reg = (int(x) for x in l.split())
        traits[e] = types.SimpleNamespace(wide=wide, A=A, pair=bool(pair), pair_reg=bool(pair_reg))
    rollout = {c: (l.split()[0] == "1", _segments(l.split()[1:])) for c, l in zip(ROLLOUT_CASES, got[n:n + len(ROLLOUT_CASES)])}
    policy = {c: _segments(l.split()[1:]) for c, l in zip(POLICY_CASES, got[n + len(ROLLOUT_CASES):])}
    return types.SimpleNamespace(traits=traits, rollout=rollout, policy=policy)


def _rollout_name(key, form, out, wide):
    """the kernel of a form, as bench.rollout_kernel_name spells it"""
    if form == "three_wave":
        return "split_rollout_kernel<%s,%d,4>" % (ENVS[key], out)
    if form in ("wide", "wide_256"):
        return "rollout_wide_kernel<%s,%d,%d>" % (ENVS[key], out, wide if form == "wide" else 256)
    if form in ("paired_reg", "paired_lds"):
        return "rollout_pg_pair_kernel<%d>" % out
    assert form in ONE_WAVE
    return "rollout_kernel<%s,%d>" % (ENVS[key], out)


def _policy_name(key, form):
    if form == "three_wave":
        return "split_policy_kernel<%s,4>" % ENVS[key]
    if form == "paired_reg":
        return "rollout_pg_pair_policy_kernel<PolicyArgs> (pg_policy_reg_body)"
    assert form == "one_wave_ragged"
    return "rollout_policy_kernel<%s>" % ENVS[key]


def _tune(split_blocks, wide_min_blocks=0):
    return types.SimpleNamespace(tune=lambda: {"split_blocks": split_blocks, "wide_min_blocks": wide_min_blocks})


def test_first_segment_is_the_kernel_bench_names(plans):
    """(a) auto-reset handles without held lanes, cr / ra / pg: the first kernel of the plan is the one bench.py names."""
    n = 0
    for key, (outputs, out), B, split, wide_min in itertools.product(bench.KERNEL_ENV, OUTPUTS.items(), BATCHES, SPLIT_BLOCKS, WIDE_MIN_BLOCKS):
        _, (_, segs) = plans.rollout[(key, out, B, "plain", split, wide_min)]
        want = bench.rollout_kernel_name(types.SimpleNamespace(key=key, outputs=outputs, B=B, ni=_tune(split, wide_min)))
        assert _rollout_name(key, segs[0][0], out, plans.traits[key].wide) == want, (key, outputs, B, split, wide_min, segs)
        n += 1
    assert n == 3 * 3 * len(BATCHES) * 4 * 5
    # bench's names cannot say out_mode 2 (observation rows [T][S][ld]): the rule asks "is an observation trajectory written",
    # so modes 2 and 3 get the same plan, for every env, handle kind and knob setting
    for key, B, handle, split, wide_min in itertools.product(ENVS, BATCHES, HANDLES, SPLIT_BLOCKS, WIDE_MIN_BLOCKS):
        assert plans.rollout[(key, 2, B, handle, split, wide_min)][1] == plans.rollout[(key, 3, B, handle, split, wide_min)][1]
    for key, affine, obs, B, split in itertools.product(bench.KERNEL_ENV, (1, 0), (1, 0), BATCHES, SPLIT_BLOCKS):
        _, segs = plans.policy[(key, affine, obs, B, "plain", split)]
        want = bench.policy_kernel_name(_tune(split), key, B, "affine" if affine else "pid", bool(obs))
        assert _policy_name(key, segs[0][0]) == want, (key, affine, obs, B, split, segs)
        if key == "ra":         # the BIG layout keeps RobotAssembly to one round whatever SPLIT_ROUNDS says: same plan
            assert plans.policy[("rar", affine, obs, B, "plain", split)] == plans.policy[(key, affine, obs, B, "plain", split)]


def _check_cover(case, plan, wide, B, handle):
    covered, segs = plan
    n_full, ragged = B // 256, B % 256 != 0
    at = 0
    for form, block0, grid in segs:
        assert block0 == at and grid > 0, (case, segs)
        at += grid * (wide // 256 if form == "wide" else 1)       # a wide block covers WIDE_ROLLOUT_BLOCK / 256 blocks
    assert at == covered == n_full + ragged, (case, plan)      # == ceil(B / 256): every block once, in order
    if handle != "plain":
        assert all(s[0] in ONE_WAVE for s in segs), (case, segs)
    return n_full, ragged


def test_segments_cover_the_batch_once(plans):
    """(b) for every env, output mode, batch, handle kind and knob setting."""
    for case, (_, plan) in plans.rollout.items():
        key, _, B, handle, _, _ = case
        segs = plan[1]
        assert 1 <= len(segs) <= 4
        n_full, ragged = _check_cover(case, plan, plans.traits[key].wide, B, handle)
        for form, block0, grid in segs:                       # the ragged block: one-wave ragged, and nothing else is
            assert (form == "one_wave_ragged") == (block0 == n_full and ragged), (case, segs)
    for case, plan in plans.policy.items():
        _, _, _, B, handle, _ = case
        segs = plan[1]
        n_full, ragged = _check_cover(case, plan, 0, B, handle)
        if ragged:                                             # (the closed loop's one-wave kernel has the predicated form only)
            assert segs[-1][0] == "one_wave_ragged" and segs[-1][1] <= n_full, (case, segs)
        assert all(s[0] in ("three_wave", "paired_reg", "one_wave_ragged") for s in segs), (case, segs)


def _rows_native_as_it_was(t, out_mode, B, handle, split_blocks, wide_min_blocks):
    """rollout_rows_native before it asked the plan: the form selection mirrored predicate by predicate."""
    if t.wide == 0 or t.A != 8:
        return False
    if handle != "plain" or wide_min_blocks >= 2 ** 30 or B % 256 != 0 or B == 0:
        return False
    n_full, n_wide = B // 256, B // t.wide
    wide = n_wide > 0 and n_wide >= wide_min_blocks
    if t.pair:
        paired = not wide and split_blocks != 0 and n_full <= split_blocks
        if paired and out_mode <= 1 and t.pair_reg:
            return False
    return True


def test_rows_native_is_the_old_predicate(plans):
    """(c) and it says yes somewhere, no somewhere, for the env that has the contiguous-byte forms."""
    seen = set()
    for case, (native, (_, segs)) in plans.rollout.items():
        key, out_mode, B, handle, split, wide_min = case
        assert native == _rows_native_as_it_was(plans.traits[key], out_mode, B, handle, split, wide_min), (case, segs)
        seen.add((key, native))
    assert ("pg", True) in seen and ("pg", False) in seen
