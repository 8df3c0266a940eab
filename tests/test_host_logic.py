"""not-gpu: host-side logic -- sharding, the partial-tally combine and its world_size-2 gloo
exchange, the 13-key aggregation against the reference's golden evaluate_with_safety dicts,
and the boundary types."""
import os
import time
import sys

import numpy as np
import pytest
import torch

from conftest import KEYS, ROOT, load_golden, result_of


def _tally_from_episodes(ret, length, viol, crit, shut, n_constraints=3):
    import neorl_industrial_gym_amd as ni
    T = ni._lib
    p = np.zeros(T.T_ROWS)
    p[T.T_EPISODES] = len(ret); p[T.T_RET_SUM] = ret.sum(); p[T.T_RET_SQ] = (ret ** 2).sum()
    p[T.T_RET_MIN] = ret.min() if len(ret) else np.inf; p[T.T_RET_MAX] = ret.max() if len(ret) else -np.inf
    p[T.T_LEN_SUM] = length.sum(); p[T.T_LEN_SQ] = (length.astype(np.float64) ** 2).sum()
    p[T.T_VIOL] = viol.sum(); p[T.T_CRIT] = crit.sum(); p[T.T_SHUTDOWN] = shut.sum()
    p[T.T_SUCCESS] = (ret > 0).sum()
    p[T.T_CONSTRAINTS] = n_constraints * length.sum()
    p[T.T_SATISFIED] = n_constraints * length.sum() - viol.sum()
    return p


@pytest.mark.parametrize("n_constraints", [0, 2, 3, 4])
def test_constraint_satisfaction_rate_for_any_constraint_count(n_constraints):
    """utils.py:109,144-147: the mean over steps of satisfied/total -- with 4 conditions
    (AdvancedChemicalReactor), after remove_safety_constraint (2), and with none left (every step 1.0)."""
    from neorl_industrial_gym_amd.core import SafetyMetrics
    from neorl_industrial_gym_amd.parallel import metrics_from_partial
    rng = np.random.default_rng(7)
    length = rng.integers(1, 40, size=25)
    per_step = [rng.integers(0, n_constraints + 1, size=n) for n in length]      # violations of every step
    viol = np.array([v.sum() for v in per_step])
    rates = [SafetyMetrics(n_constraints - int(x), n_constraints, int(x), 0, 0.0).satisfaction_rate
             for v in per_step for x in v]
    ret = rng.normal(size=25)
    p = _tally_from_episodes(ret, length, viol, np.zeros(25), np.zeros(25), n_constraints)
    got = metrics_from_partial(p, 25)
    assert got["constraint_satisfaction_rate"] == pytest.approx(np.mean(rates), rel=1e-12)


def test_shard_range_partitions_exactly():
    from neorl_industrial_gym_amd.parallel import shard_range
    for total in (1, 7, 8, 65536, 2097152, 1000003):
        for world in (1, 2, 3, 8):
            spans = [shard_range(total, r, world) for r in range(world)]
            assert spans[0][0] == 0 and sum(c for _, c in spans) == total
            for (s0, c0), (s1, _) in zip(spans, spans[1:]):
                assert s0 + c0 == s1
            assert max(c for _, c in spans) - min(c for _, c in spans) <= 1
    with pytest.raises(ValueError):
        shard_range(10, 2, 2)


@pytest.mark.parametrize("key", KEYS)
def test_metrics_from_partial_matches_reference_dict(key):
    """Aggregating the golden per-episode arrays through the build's tally formulas reproduces the
    reference's evaluate_with_safety() dict (utils.py:128-152)."""
    from neorl_industrial_gym_amd.parallel import combine_partials, metrics_from_partial
    d = load_golden(key, "g4")
    want = result_of(d)
    n = len(d["ep_length"])
    cut = n // 3      # two uneven shards
    parts = []
    for sl in (slice(0, cut), slice(cut, n)):
        parts.append(_tally_from_episodes(d["ep_return"][sl], d["ep_length"][sl], d["ep_viol"][sl],
                                          d["ep_crit"][sl], d["ep_shutdown"][sl]))
    got = metrics_from_partial(combine_partials(torch.tensor(np.stack(parts))), n)
    assert set(got) == set(want) and len(got) == 13
    for k in ("safety_violations", "critical_violations", "emergency_shutdowns", "successful_episodes"):
        assert got[k] == want[k], k
    for k in ("return_mean", "return_std", "return_min", "return_max", "length_mean", "length_std",
              "safety_violations_per_episode", "constraint_satisfaction_rate", "success_rate"):
        assert got[k] == pytest.approx(want[k], rel=1e-5, abs=1e-9), k


def _gloo_worker(rank, world, port, tmp):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    from conftest import load_golden
    from neorl_industrial_gym_amd.parallel import all_reduce_partial, metrics_from_partial, shard_range
    dist.init_process_group("gloo", rank=rank, world_size=world)
    d = load_golden("pg", "g4")
    n = len(d["ep_length"])
    s, c = shard_range(n, rank, world)
    sl = slice(s, s + c)
    part = torch.tensor(_tally_from_episodes(d["ep_return"][sl], d["ep_length"][sl], d["ep_viol"][sl],
                                             d["ep_crit"][sl], d["ep_shutdown"][sl]))
    total = all_reduce_partial(part)
    res = metrics_from_partial(total)
    np.save(os.path.join(tmp, f"r{rank}.npy"), total.numpy())
    assert res["safety_violations"] == int(d["ep_viol"].sum())
    dist.destroy_process_group()


def test_all_gather_combine_world2_gloo(tmp_path):
    """N>1 path on CPU: two ranks, contiguous shards, gloo all-gather, identical combine on both."""
    import socket
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]
    mp.spawn(_gloo_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    a, b = np.load(tmp_path / "r0.npy"), np.load(tmp_path / "r1.npy")
    assert np.array_equal(a, b)                      # bit-identical on every rank
    d = load_golden("pg", "g4")
    whole = _tally_from_episodes(d["ep_return"], d["ep_length"], d["ep_viol"], d["ep_crit"], d["ep_shutdown"])
    import neorl_industrial_gym_amd as ni
    T = ni._lib
    for r in (T.T_EPISODES, T.T_LEN_SUM, T.T_LEN_SQ, T.T_VIOL, T.T_CRIT, T.T_SHUTDOWN, T.T_SUCCESS, T.T_RET_MIN, T.T_RET_MAX):
        assert a[r] == whole[r]                      # integer rows / extrema exact
    assert a[T.T_RET_SUM] == pytest.approx(whole[T.T_RET_SUM], rel=1e-14)


def test_boundary_types():
    import neorl_industrial_gym_amd as ni
    sm = ni.SafetyMetrics(constraints_satisfied=2, total_constraints=3, violation_count=1, critical_violations=1,
                          safety_score=2 / 3)
    assert sm.satisfaction_rate == 2 / 3 and sm.violation_severity == {} and sm.adaptive_threshold == 0.95
    assert ni.SafetyMetrics(0, 0, 0, 0, 1.0).satisfaction_rate == 1.0
    c = ni.SafetyConstraint(name="x", check_fn=lambda s, a: True, penalty=-1.0)
    assert c.critical is False and c.description == ""
    assert [q.value for q in ni.DatasetQuality] == ["expert", "medium", "mixed", "random"]
    from neorl_industrial_gym_amd.core import Box
    b = Box(-1.0, 1.0, (3,), np.float32)
    x = b.sample()
    assert x.dtype == np.float32 and b.contains(x) and b.low.dtype == np.float32


def test_evaluate_requires_trained_agent():
    import neorl_industrial_gym_amd as ni

    class A:
        is_trained = False
    with pytest.raises(RuntimeError, match="Agent must be trained before evaluation"):
        ni.evaluate_with_safety(A(), object(), 1)


def test_device_policy_host_predict_matches_oracle_policy(oracle):
    """DevicePolicy.predict (host float32 mirror of the on-device arithmetic) equals the oracle's
    restatement of nig-policy-v1 for every deterministic policy family; the struct handed to the
    device has the oracle's layout."""
    import ctypes as C
    import neorl_industrial_gym_amd as ni
    assert C.sizeof(ni._lib.Policy) == C.sizeof(oracle.Policy)
    rng = np.random.default_rng(3)
    for key, name, S, A in (("cr", "ChemicalReactor-v0", 12, 3), ("pg", "PowerGrid-v0", 32, 8), ("ra", "RobotAssembly-v0", 24, 7)):
        obs = oracle.reset(key, np.stack([oracle.gen_reset_noise(key, 1, i, 0) for i in range(20)]))
        pols = [ni.behaviour_policy(name, "expert"), ni.mpc_agent(S, A), ni.constant_agent(S, A, rng.uniform(-1, 1, A)),
                ni.DevicePolicy(S, A, W=rng.normal(0, 0.02, (A, S)), b=rng.normal(0, 0.1, A), clip=(-0.7, 0.9))]
        for pol in pols:
            pol.sigma[:] = 0
            P = oracle.Policy.from_buffer_copy(bytes(pol.to_struct()))
            want = np.stack([oracle.policy_action(key, P, o) for o in obs])
            got = pol.predict(obs)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        pid = ni.pid_agent(S, A, kp=0.3, ki=0.02, kd=0.1, setpoint=rng.normal(0, 1, A))
        P = oracle.Policy.from_buffer_copy(bytes(pid.to_struct()))
        integ, eprev = np.zeros(8, dtype=np.float32), np.zeros(8, dtype=np.float32)
        for o in obs[:6]:                      # stateful: same sequence on both sides
            want = oracle.policy_action(key, P, o, integ=integ, eprev=eprev)
            got = pid.predict(o)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_behaviour_policy_tables():
    """The device behaviour policies encode the reference's get_dataset formulas."""
    import neorl_industrial_gym_amd as ni
    from neorl_industrial_gym_amd.policies import DATASET_SHAPE
    assert DATASET_SHAPE["ChemicalReactor-v0"]["medium"] == (200, 350)          # chemical_reactor.py:337-339
    assert DATASET_SHAPE["PowerGrid-v0"]["mixed"] == (200, 1000)                 # power_grid.py:197-215
    assert DATASET_SHAPE["RobotAssembly-v0"]["random"] == (100, 1000)            # robot_assembly.py:248-265
    p = ni.behaviour_policy("ChemicalReactor-v0", "expert")
    obs = np.zeros(12, dtype=np.float32); obs[0] = 330.0; obs[10] = 65.0
    te, le = (330.0 - 320.0) / 50, (65.0 - 55.0) / 50
    assert np.allclose(p.predict(obs), [-te * 0.5, te * 0.3, -le * 0.2], atol=2e-6)   # chemical_reactor.py:368-376
    assert np.allclose(p.sigma, 0.01) and p.clip == (-1.0, 1.0)
    p = ni.behaviour_policy("ChemicalReactor-v0", "mixed")
    assert float(p.p_uniform) == 0.5 and np.allclose(p.sigma, [0.15, 0.25, 0.15])      # :380-391
    p = ni.behaviour_policy("PowerGrid-v0", "expert")
    obs = np.zeros(32, dtype=np.float32); obs[0] = 0.2; obs[9:17] = 50; obs[17:25] = 52
    assert np.allclose(p.predict(obs), -0.5 * 0.2 + 0.1 * 16.0 / 8, atol=1e-5)          # power_grid.py:218-222
    assert float(ni.behaviour_policy("PowerGrid-v0", "random").uniform_range) == 5.0
    p = ni.behaviour_policy("RobotAssembly-v0", "expert")
    obs = np.zeros(24, dtype=np.float32); obs[0:3] = [0.1, 0.2, 0.3]; obs[7:14] = np.arange(7) * 0.1
    assert np.allclose(p.predict(obs), [0.4, -0.4, 0.2, -0.03, -0.04, -0.05, -0.06], atol=1e-6)   # robot_assembly.py:268-278
    p = ni.behaviour_policy("RobotAssembly-v0", "mixed")
    assert float(p.p_uniform) == np.float32(0.3) and np.allclose(p.half_range, [0, 0, 0, .5, .5, .5, .5])
    with pytest.raises(AssertionError):
        ni.random_agent(4, 2, -1.0, 2.0)


def test_constant_division_is_correctly_rounded(tmp_path):
    """Every divisor the device code hands to fdiv_c (csrc/nig_envs.hpp) is proven exhaustively: the
    4-instruction sequence equals IEEE x / c for all 2^23 significands (tests/constdiv_check.c)."""
    import re
    import subprocess
    src = open(os.path.join(ROOT, "neorl-industrial-gym_amd", "csrc", "nig_envs.hpp")).read()
    consts = sorted({m.group(1) for m in re.finditer(r"fdiv_c\([^;]*?,\s*([0-9.eE+-]+)f\)", src)})
    assert len(consts) >= 10, consts
    exe = tmp_path / "constdiv_check"
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-mfma", "-o", str(exe),
                    os.path.join(ROOT, "tests", "constdiv_check.c"), "-lm"], check=True)
    out = subprocess.run([str(exe)] + consts, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout
    assert out.stdout.count("mismatches=0") == len(consts), out.stdout


def test_fp64_division_by_a_shared_divisor_is_correctly_rounded(tmp_path):
    """ddiv_y (csrc/nig_detmath.hpp: product with the reciprocal + two fused corrections, Markstein) against IEEE fp64
    division on 3.6e7 operands per divisor -- random binades, RobotAssembly's x - s0 differences, numerators placed at
    rounding boundaries of the quotient -- for every constant divisor the device code uses and a set of step sizes."""
    import re
    import subprocess
    src = open(os.path.join(ROOT, "neorl-industrial-gym_amd", "csrc", "nig_envs.hpp")).read()
    consts = sorted({m.group(1) for m in re.finditer(r"ddiv_y\([^;]*?,\s*([0-9.eE+-]+),\s*1\.0\s*/", src)})
    assert set(consts) >= {"0.005", "0.05", "1000.0"}, consts
    exe = tmp_path / "ddiv_check"
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-mfma", "-o", str(exe), os.path.join(ROOT, "tests", "ddiv_check.c"), "-lm"], check=True)
    divisors = consts + ["0.1", "0.01", "0.02", "0.05", "0.001", "0.25", "1.0", "0.3333333333333333", "7.0", "1e-30", "1e30"]
    out = subprocess.run([str(exe), "1000000"] + divisors, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:]
    assert out.stdout.count("mismatches=0") == len(divisors), out.stdout[-2000:]


def test_probit_table_with_folded_scale_is_bit_identical(tmp_path):
    """The normal transform's table stores {c0, c1 2^-18, c2 2^-36, c3 2^-54} and the position in a piece is taken as
    an integer (one multiply less per normal): over all 768 x 2^18 inputs the result has the same bits as the unscaled
    evaluation (tests/probit_scale_check.c)."""
    import subprocess
    exe = tmp_path / "probit_scale_check"
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-mfma", "-o", str(exe),
                    os.path.join(ROOT, "tests", "probit_scale_check.c"), "-lm"], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "mismatches=0" in out.stdout, out.stdout


def test_probit_piece_number_from_the_unshifted_word_is_the_same_piece():
    """nig_detmath.hpp probit_fetch (round 5): x = float((word & 0x7FFFFF00) | 0x80) = 64 (4 m + 2) -- one v_and_or_b32 on the
    word as it stands -- instead of m = bits 30..8, float(m), fma(m, 4, 2).  For ALL 2^23 values of m: the conversion is exact,
    the mantissa is the same, so the position in the piece (low 18 bits) is the same and the piece number is the old one plus
    PROBIT_BIAS = 192 (the constant that rides in the table's address).  The oracle keeps the round-4 form: GPU == oracle bit for
    bit (tests/test_gpu_parity.py) rests on this identity."""
    m = np.arange(1 << 23, dtype=np.uint32)
    for sign in (np.uint32(0), np.uint32(0x80000000)):
        for low in (np.uint32(0), np.uint32(0xFF), np.uint32(0x5A)):                     # sign bit and low byte never matter
            word = sign | (m << np.uint32(8)) | low
            u = (word & np.uint32(0x7FFFFF00)) | np.uint32(0x80)
            x_new = u.astype(np.float32)
            assert (x_new.astype(np.float64) == u.astype(np.float64)).all()             # exact conversion: 2 m + 1 is an odd 24-bit integer
            x_old = m.astype(np.float32) * np.float32(4.0) + np.float32(2.0)            # exact too (4 m + 2 < 2^25, even)
            b_new, b_old = x_new.view(np.uint32), x_old.view(np.uint32)
            assert ((b_new & np.uint32(0x3FFFF)) == (b_old & np.uint32(0x3FFFF))).all()
            piece_new = ((b_new >> np.uint32(18)) & np.uint32(0x3FF)).astype(np.int64)
            piece_old = ((b_old >> np.uint32(18)) & np.uint32(0x3FF)).astype(np.int64)
            assert (piece_new == piece_old + 192).all() and piece_old.min() == 0 and piece_old.max() == 767
    src = open(os.path.join(ROOT, "neorl-industrial-gym_amd", "csrc", "nig_detmath.hpp")).read()
    assert "constexpr int PROBIT_BIAS = 192;" in src and "0x7fffff00" in src


def test_stale_library_is_never_rebuilt_under_a_profiler(monkeypatch):
    """ADVICE (round 1): importing the package inside a rocprofv3-preloaded process rebuilt a stale libnig.so
    there (hipcc -> sh -c -> clang++ from a GPU-initialised process).  _build.ensure() must refuse instead."""
    from neorl_industrial_gym_amd import _build
    assert not _build.stale(), "the test needs a current library (run __graft_entry__.build())"
    assert _build.ensure() == _build.LIB                      # current: nothing to do, whatever the environment
    monkeypatch.setattr(_build, "stale", lambda: True)
    called = []
    monkeypatch.setattr(_build, "build", lambda **kw: called.append(kw) or _build.LIB)
    monkeypatch.setenv("NIG_NO_AUTOBUILD", "1")
    with pytest.raises(ImportError, match="auto-build is disabled"):
        _build.ensure()
    monkeypatch.delenv("NIG_NO_AUTOBUILD")
    monkeypatch.setenv("LD_PRELOAD", "/opt/rocm/lib/librocprofiler-sdk-tool.so")
    with pytest.raises(ImportError, match="auto-build is disabled"):
        _build.ensure()
    assert not called
    monkeypatch.delenv("LD_PRELOAD")
    monkeypatch.setenv("LOCAL_RANK", "0")
    assert _build.ensure() == _build.LIB and len(called) == 1  # only local rank 0 compiles


def test_build_hash_covers_every_source_of_the_library():
    """Staleness is a content hash over csrc/*.hip, *.hpp, *.inc and include/nig.h (round 1 missed the .inc files)."""
    from neorl_industrial_gym_amd import _build
    names = {os.path.basename(p) for p in _build.sources() + _build.headers()}
    for f in ("nig_api.hip", "nig_mixed.hip", "env_pg.hip", "nig_kernels.hpp", "nig_episode.hpp", "nig_envs.hpp", "nig_detmath.hpp",
              "nig_device.hpp", "nig_step.hpp", "nig_step_kernel.hpp", "nig_rollout.hpp", "nig_rollout_wide.hpp", "nig_policy.hpp",
              "nig_rollout_policy.hpp", "nig_mlp.hpp", "nig_mlp_stream.hpp", "nig_probit_table.inc", "nig_spec_plants.inc", "nig.h"):
        assert f in names, f


def test_bench_traffic_lookup_is_per_env_step_and_keyed_by_plan_length():
    sys.path.insert(0, ROOT)
    import bench
    per_step, src = bench.measured_traffic("cr", 65536, "rollout", "full", 250)
    assert per_step is not None and 60.0 < per_step < 80.0 and "pmc" in src          # ~69 B vs 68 algorithmic
    assert bench.measured_traffic("cr", 65536, "rollout", "full", 20) == (None, None)    # another launch length: no figure
    assert bench.measured_traffic("cr", 12345, "rollout", "full", 250) == (None, None)
    pg, _ = bench.measured_traffic("pg", 262144, "rollout", "full", 250)
    assert pg is not None and 160.0 < pg < 190.0
    assert bench.alg_bytes_rollout(12, 3, "full") == 68 and bench.alg_bytes_per_step(32, 8) == 304


def test_bench_names_the_kernel_the_library_launches():
    """bench.py's roofline.kernel follows the host rule of csrc/nig_launch_plan.hpp plan_rollout: the three-wave
    form for ChemicalReactor batches of whole 256-lane blocks that are at most one round (one block per CU) or whose
    last round is at least 3/4 full; everything else the one-wave rollout_kernel."""
    import types

    import bench
    import neorl_industrial_gym_amd as ni
    before = ni.tune()["split_blocks"]
    try:
        ni.tune(split_blocks=256)
        def name(key, B, outputs="full"):
            return bench.rollout_kernel_name(types.SimpleNamespace(key=key, B=B, outputs=outputs, ni=ni))
        assert name("cr", 65536) == "split_rollout_kernel<ChemicalReactor,3,4>"
        assert name("cr", 65536, "none") == "split_rollout_kernel<ChemicalReactor,0,4>"
        assert name("cr", 1024, "min") == "split_rollout_kernel<ChemicalReactor,1,4>"
        assert name("cr", 131072).startswith("split_") and name("cr", 1048576).startswith("split_")   # even rounds, with the trajectory
        assert name("cr", 131072, "min").startswith("rollout_kernel<") and name("cr", 1048576, "none").startswith("rollout_kernel<")   # round 5: rounds lose without it
        assert name("cr", 65536 + 49152 + 256).startswith("split_")                                   # last round 193 / 256 blocks
        assert name("cr", 98304).startswith("rollout_kernel<")                                        # 1.5 rounds
        assert name("cr", 65536 + 100).startswith("split_")          # whole blocks in this form, the ragged last block in a one-wave launch
        assert name("cr", 200).startswith("rollout_kernel<")          # no whole block at all
        assert name("pg", 262144) == "rollout_wide_kernel<PowerGrid,3,512>"      # >= 256 blocks of 512 lanes: the LDS-resident form
        assert name("pg", 65536) == "rollout_pg_pair_kernel<3>"                 # one 256-lane block per compute unit: the paired form (producer waves)
        assert name("pg", 98304) == "rollout_wide_kernel<PowerGrid,3,256>"      # 192 wide blocks: below the wide threshold, more than one round of pairs
        assert name("pg", 100) == "rollout_kernel<PowerGrid,3>"                 # no whole block
        assert name("ra", 262144) == "rollout_kernel<RobotAssembly,3>"          # more than one round: lanes fill the SIMDs
        assert name("ra", 65536) == "split_rollout_kernel<RobotAssembly,3,4>" and name("ra", 1024, "min") == "split_rollout_kernel<RobotAssembly,1,4>"
        assert name("ra", 65536 + 256) == "rollout_kernel<RobotAssembly,3>"
        ni.tune(split_blocks=0, wide_min_blocks=1 << 30)
        assert name("cr", 65536).startswith("rollout_kernel<") and name("pg", 262144) == "rollout_kernel<PowerGrid,3>"
        assert name("ra", 65536) == "rollout_kernel<RobotAssembly,3>"
        ni.tune(split_blocks=0, wide_min_blocks=256)
        assert name("pg", 65536) == "rollout_wide_kernel<PowerGrid,3,256>"
    finally:
        ni.tune(split_blocks=before, wide_min_blocks=256)


def _run_bench(args, env_extra, timeout=600):
    import json
    import subprocess
    import sys
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update(env_extra)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + args, env=env, capture_output=True, text=True,
                       timeout=timeout)
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    return p, (json.loads(lines[-1]) if lines else None)


def test_bench_launches_and_verifies_its_own_ranks():
    """`bench.py --gpus 2` WITHOUT torchrun starts two ranks itself (gloo here: no GPU in this container, so the
    device workload is replaced by a stand-in -- the launch, rendezvous, barriers, tally all-gather / combine /
    self-check and the result line are the real code), and the line says n_gpus == 2 with two ranks in the exchange.
    The same flow with the real workload on one GPU: tests/test_gpu_abi_round2.py::test_bench_two_ranks_on_one_gpu."""
    p, rec = _run_bench(["--gpus", "2", "--steps", "3", "--warmup", "1"], {"NIG_BENCH_REHEARSE": "cpu"})
    assert p.returncode == 0, p.stderr[-2000:]
    assert rec["n_gpus"] == 2 and rec["ranks"] == 2 and rec["tally_check"]["ranks"] == 2
    assert rec["episodes_per_rank"] == [100, 101] and rec["tally"]["episodes"] == 201
    assert rec["value"] is None and "rehearsal" in rec          # never mistaken for a measurement
    # the N-rank line says what it is: a rehearsal, not a hardware curve; every rank's own time; where the ranks were pinned
    assert rec["scale"]["measured_on_hardware"] is False and rec["scale"]["world"] == 2 and "REHEARSAL" in rec["scale"]["note"]
    rt = rec["rank_times"]
    assert rt["ranks"] == 2 and len(rt["wall_s_per_rank"]) == 2 and len(rt["launch_us_per_rank"]) == 2
    assert rt["wall_min_s"] <= rt["wall_median_s"] <= rt["wall_max_s"] == max(rt["wall_s_per_rank"])
    assert rec["ms_per_step"] == pytest.approx(rt["wall_max_s"] * 1e3 / 3)         # the line's time IS the slowest rank's interval
    aff = rec["scale"]["rank_affinity"]
    assert len(aff) == 2 and all("pinned" in a for a in aff)
    if all(a["pinned"] for a in aff):          # disjoint CPU shares (a NUMA node's CPU list need not be one range: 0-63,128-191)
        assert not set(aff[0]["cpu_set"]) & set(aff[1]["cpu_set"]) and all(len(a["cpu_set"]) == a["cpus"] for a in aff)
    # N = 1 and N = 2 time the same set of operations: K launches + the stream synchronisation, no collective inside
    p1, rec1 = _run_bench(["--gpus", "1", "--steps", "3", "--warmup", "1"], {"NIG_BENCH_REHEARSE": "cpu"})
    assert p1.returncode == 0, p1.stderr[-2000:]
    assert rec1["rank_times"]["timed_interval"] == rt["timed_interval"] and "outside the interval" in rt["timed_interval"]
    assert rec1["scale"]["measured_on_hardware"] is False and rec1["scale"]["world"] == 1


def test_bench_one_rank_process_group_takes_the_collective_branches():
    """NIG_BENCH_FORCE_PG=1: a ONE-rank process group makes bench.py run init_process_group, the barriers,
    the all-gathers of the rank times and tally partials, all_gather_object and destroy_process_group -- here over gloo with the
    stand-in workload; tests/test_gpu_rccl_one_rank.py runs the same switch over "nccl" (RCCL) with the real workload."""
    p, rec = _run_bench(["--gpus", "1", "--steps", "3", "--warmup", "1"], {"NIG_BENCH_REHEARSE": "cpu", "NIG_BENCH_FORCE_PG": "1"})
    assert p.returncode == 0, p.stderr[-2000:]
    pg = rec["scale"]["process_group"]
    assert pg == {"backend": "gloo", "world": 1, "forced_one_rank": True}
    assert rec["ranks"] == 1 and rec["tally_check"]["ok"] and rec["scale"]["measured_on_hardware"] is False
    p0, rec0 = _run_bench(["--gpus", "1", "--steps", "3", "--warmup", "1"], {"NIG_BENCH_REHEARSE": "cpu"})
    assert p0.returncode == 0 and rec0["scale"]["process_group"] is None        # the plain one-GPU run builds no group


def test_bench_timed_interval_holds_no_collective():
    """bench.timed(): the clock stops after the stream synchronisation and BEFORE the closing barrier (VERDICT r03 weak #5:
    with world > 1 the wall clock used to include one dist.barrier() the N = 1 run never pays)."""
    import bench
    import torch
    calls = []

    class FakeDist:
        def barrier(self):
            calls.append(("barrier", time.perf_counter()))
            time.sleep(0.05)

        def all_gather(self, out, t):
            for o in out:
                o.copy_(t)

    class W:
        def launch(self):
            calls.append(("launch", time.perf_counter()))

        def kernels_per_launch(self):
            return 1
    stats = {}
    wall, _ = bench.timed(torch, FakeDist(), 2, torch.device("cpu"), W(), 4, 1, stats=stats)
    kinds = [k for k, _ in calls]
    assert kinds == ["launch", "barrier", "launch", "launch", "launch", "launch", "barrier"]
    assert wall < 0.04, wall                     # neither 50 ms barrier is inside the interval
    assert stats["wall_s_per_rank"] == [wall, wall]


def test_bench_hbm_side_fraction_counts_only_what_the_cache_cannot_serve():
    """roofline.frac (round 4): a byte stream counts when its footprint exceeds the 256 MB Infinity Cache.  Headline shape:
    917 MB of per-step outputs count (56 of the 68 B), the 50 MB action ring does not; rings larger than the cache make all
    68 B count; the step API at 65 536 lanes (a 62 MB working set) moves nothing to HBM in steady state; at 4 M lanes it all counts."""
    import types

    import bench
    ring = lambda slots, A, ld: torch.empty(slots, A, ld, dtype=torch.float32, device="meta")
    wl = types.SimpleNamespace(mode="rollout", outputs="full", S=12, A=3, B=65536, P=250, R=64, env=types.SimpleNamespace(ld=65536),
                               rings=[ring(64, 3, 65536)])
    b, why = bench.hbm_side_bytes(wl)
    assert b == 56 and why["outputs_footprint_bytes"] == 56 * 250 * 65536 and why["action_ring_footprint_bytes"] == 64 * 3 * 65536 * 4
    wl.rings = [ring(250, 3, 65536) for _ in range(3)]
    assert bench.hbm_side_bytes(wl)[0] == 68
    wl.outputs, wl.rings = "min", [ring(64, 3, 65536)]
    assert bench.hbm_side_bytes(wl)[0] == 0                      # 131 MB of reward + flag rows, 50 MB ring: all inside the cache
    pg = types.SimpleNamespace(mode="rollout", outputs="full", S=32, A=8, B=262144, P=250, R=34, env=types.SimpleNamespace(ld=262144),
                               rings=[ring(34, 8, 262144)])
    assert bench.hbm_side_bytes(pg)[0] == 168                    # the PowerGrid record's 285 MB ring is larger than the cache
    st = types.SimpleNamespace(mode="graph", outputs="full", S=12, A=3, B=65536, P=250, R=64, env=types.SimpleNamespace(ld=65536), rings=[])
    assert bench.hbm_side_bytes(st)[0] == 0
    st.B, st.env.ld = 4194304, 4194304
    assert bench.hbm_side_bytes(st)[0] == bench.alg_bytes_per_step(12, 3) == 124


def test_phase_stats_cuts_a_kernel_trace_at_the_lines_own_launch_counts(tmp_path):
    """profiles/phase_stats.py: the headline kernel's launches of a profiled bench run, split by rank_times.phases."""
    import json
    import subprocess
    import sys
    name = "void nig::split_rollout_kernel<nig::ChemicalReactor, 3, 4, false>(nig::RolloutArgs)"
    durs = [200] * 3 + [170] * 2 + [168] * 4 + [210] * 4            # settle, warm-up, timed, cold
    rows, t = ['"Kind","Kernel_Name","Start_Timestamp","End_Timestamp"'], 1000
    for d in durs:
        rows.append(f'"KERNEL_DISPATCH","{name}",{t},{t + d * 1000}')
        t += d * 1000 + 500
    rows.insert(3, '"KERNEL_DISPATCH","void nig::fill_actions_kernel<nig::ChemicalReactor>(float*)",5,9')
    (tmp_path / "trace.csv").write_text("\n".join(rows) + "\n")
    line = {"ms_per_step": 0.1705, "roofline": {"kernel": "split_rollout_kernel<ChemicalReactor,3,4>", "launch_us": 168.9},
            "rank_times": {"phases": [{"name": "settle", "launches": 3}, {"name": "warmup", "launches": 2}, {"name": "timed", "launches": 4},
                                      {"name": "cold_first_launches", "launches": 4}]}}
    (tmp_path / "bench.json").write_text("some stderr noise\n" + json.dumps(line) + "\n")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "profiles", "phase_stats.py"), str(tmp_path / "trace.csv"),
                        str(tmp_path / "bench.json"), str(tmp_path / "out.csv")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    out = (tmp_path / "out.csv").read_text().splitlines()
    got = {l.split(",")[0]: l for l in out[1:] if not l.startswith("#")}
    assert ",3,200.00," in got["settle"] and ",2,170.00," in got["warmup"] and ",4,168.00," in got["timed"] and ",4,210.00," in got["cold_first_launches"]
    assert "timed phase: 168.00 us" in out[-1] and "WARNING" not in p.stderr


def test_bench_pins_ranks_to_disjoint_cpu_shares(monkeypatch):
    """bench.pin_rank: without topology information every local rank gets an even contiguous share of the allowed CPUs; a single
    rank (or too few CPUs) is left alone; a failure is reported, never raised."""
    import bench
    allowed = set(range(16))
    seen = {}
    monkeypatch.setattr(os, "sched_getaffinity", lambda pid: set(allowed))
    monkeypatch.setattr(os, "sched_setaffinity", lambda pid, cpus: seen.__setitem__("cpus", list(cpus)))
    monkeypatch.setattr(bench, "gpu_numa_nodes", lambda: None)
    monkeypatch.setattr(bench, "numa_cpulists", lambda allowed: [sorted(allowed)])      # one NUMA node, whatever this host has
    r0, r3 = bench.pin_rank(0, 4), None
    assert r0["pinned"] and seen["cpus"] == [0, 1, 2, 3]
    r3 = bench.pin_rank(3, 4)
    assert r3["pinned"] and seen["cpus"] == [12, 13, 14, 15] and r3["how"] == "even-split"
    assert bench.pin_rank(0, 1)["pinned"] is False
    # two NUMA nodes whose CPU numbers interleave cores and SMT siblings: ranks in node order, an even share of THEIR node
    monkeypatch.setattr(bench, "numa_cpulists", lambda allowed: [[0, 1, 2, 3, 8, 9, 10, 11], [4, 5, 6, 7, 12, 13, 14, 15]])
    r2 = bench.pin_rank(2, 4)
    assert r2["pinned"] and seen["cpus"] == [4, 5, 6, 7] and r2["how"].startswith("numa node 1 of 2")
    monkeypatch.setattr(os, "sched_setaffinity", lambda pid, cpus: (_ for _ in ()).throw(OSError("no")))
    assert bench.pin_rank(1, 4)["pinned"] is False


def test_bench_does_not_spawn_under_a_profiler_preload():
    """A rocprofv3 preload initialises the GPU before main(): spawning the ranks from that process would be an exec from a
    GPU-initialised process (forbidden on this pool) -- bench.py refuses with a message instead."""
    p, rec = _run_bench(["--gpus", "2"], {"NIG_BENCH_REHEARSE": "cpu", "ROCP_TOOL_LIBRARIES": "/opt/rocm/lib/librocprofiler-sdk-tool.so"})
    assert p.returncode != 0 and rec is None and "profiler preload" in p.stderr


def test_bench_refuses_a_world_that_differs_from_gpus():
    """--gpus N under a launcher that formed another world size: non-zero exit, message names the command."""
    p, rec = _run_bench(["--gpus", "2"], {"NIG_BENCH_REHEARSE": "cpu", "WORLD_SIZE": "3", "RANK": "0"})
    assert p.returncode != 0 and rec is None and "torch.distributed.run" in p.stderr
    p, rec = _run_bench(["--gpus", "1"], {"NIG_BENCH_REHEARSE": "cpu", "WORLD_SIZE": "2", "RANK": "0"})
    assert p.returncode != 0 and rec is None


def test_bench_plain_run_options_and_output_sample():
    """A plain run is the headline only (--full off by default); --steps below 1 and --dump-outputs without a device
    workload are refused, not bent into something else; the dumped lanes are all of them when they fit, else the same
    seeded, sorted sample every time, within the byte budget."""
    import bench
    args = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert args.full is False and args.dump_outputs is None and args.steps == 7
    assert bench.parse_args(["--full", "--dump-outputs", "out"]).full and bench.parse_args(["--dump-outputs", "out"]).dump_outputs == "out"
    assert np.array_equal(bench.dump_lanes(2048, 15048), np.arange(2048))
    a, b = bench.dump_lanes(65536, 15048), bench.dump_lanes(65536, 15048)
    assert np.array_equal(a, b) and np.all(np.diff(a) > 0) and a[0] >= 0 and a[-1] < 65536
    assert a.size * 15048 <= bench.DUMP_BYTES < a.size * 15048 + 15048
    with pytest.raises(SystemExit):
        bench.dump_lanes(8, bench.DUMP_BYTES + 1)
    for argv in (["--steps", "0"], ["--dump-outputs", "out"]):
        p, rec = _run_bench(["--gpus", "1"] + argv, {"NIG_BENCH_REHEARSE": "cpu"})
        assert p.returncode != 0 and rec is None, argv


def test_oracle_under_sanitizers():
    """SURVEY section 5 / VERDICT r02: the oracle's C restatement built with -fsanitize=address,undefined and the
    golden-vector tests (every entry point: step, step64, reset, rollouts, policies, the MLP actor, the generator) run
    against that build; any out-of-bounds access, use of an uninitialised-size object or undefined arithmetic aborts."""
    import subprocess
    import sys
    asan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(asan) or not os.path.exists(asan):
        pytest.skip("no libasan in this toolchain")
    preload = ":".join(p for p in (asan, os.environ.get("LD_PRELOAD", "")) if p)     # the runtime first; keep what is preloaded already
    env = dict(os.environ, NIG_ORACLE_SANITIZE="1", LD_PRELOAD=preload,
               ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1", OMP_NUM_THREADS="2")
    p = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "not gpu", "-p", "no:cacheprovider",
                        os.path.join(ROOT, "tests", "test_oracle_golden.py"), os.path.join(ROOT, "tests", "test_advanced_envs.py"),
                        os.path.join(ROOT, "tests", "test_spec_envs.py")],
                       env=env, capture_output=True, text=True, timeout=1500, cwd=ROOT)
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    assert " passed" in p.stdout and "ERROR: AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr
