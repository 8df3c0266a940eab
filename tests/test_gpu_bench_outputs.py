"""-m gpu: a plain `bench.py` run times the headline only, and `--dump-outputs DIR` writes what its last timed launch returned,
identically from run to run with the same arguments (the settle load runs on a twin of the timed workload, so the number
of settle launches -- a matter of wall time -- does not reach the outputs)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

B, S, P, K = 8192, 12, 250, 3
ARGS = ["--gpus", "1", "--batch", str(B), "--steps", str(K), "--warmup", "2", "--settle", "0.3"]


def _bench(out_dir, extra=()):
    env = dict(os.environ, NIG_NO_AUTOBUILD="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "NIG_BENCH_REHEARSE", "NIG_BENCH_FORCE_PG"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + ARGS + list(extra) + ["--dump-outputs", str(out_dir)],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("{") and '"metric"' in l][-1])


def test_plain_bench_dumps_the_same_outputs_every_run(tmp_path):
    import bench
    import neorl_industrial_gym_amd as ni
    lanes = bench.dump_lanes(B, P * (4 + 8 + 4 * S) + 4 * S).size      # a seeded sample of the 8192 lanes
    assert 0 < lanes < B
    recs = [_bench(tmp_path / name) for name in ("a", "b")]
    for rec in recs:
        assert rec["steps"] == K and rec["unit"] == "env-steps/s" and rec["higher_is_better"] is True and rec["dtype"] == "f32"
        assert rec["value"] > 0 and rec["ms_per_step"] == pytest.approx(rec["rank_times"]["wall_max_s"] * 1e3 / K)
        assert rec["rank_times"]["phases"][-1] == {"name": "timed", "launches": K}
        assert not {"cpu_baseline", "parity", "step_api", "powergrid", "robotassembly", "mixed", "single_env"} & set(rec)
        assert "cold_first_launches" not in rec["roofline"]
    assert recs[0]["tally"] == recs[1]["tally"]
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["flags.npy", "obs.npy", "reward.npy", "state.npy", "tally.npy"] and sorted(os.listdir(tmp_path / "b")) == names
    d = {n[:-4]: np.load(tmp_path / "a" / n) for n in names}
    for n in names:
        other = np.load(tmp_path / "b" / n)
        assert other.dtype == d[n[:-4]].dtype and np.array_equal(other.view(np.uint8), d[n[:-4]].view(np.uint8)), n
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= 64 * 10**6
    assert d["reward"].shape == d["flags"].shape == (P, lanes) and d["obs"].shape == (P, lanes, S) and d["state"].shape == (lanes, S)
    assert d["reward"].dtype == d["obs"].dtype == d["state"].dtype == np.float32 and d["flags"].dtype == d["tally"].dtype == np.float64
    assert np.isfinite(d["reward"]).all() and np.array_equal(d["flags"], np.round(d["flags"]))
    assert int(d["tally"][ni._lib.T_EPISODES]) == recs[0]["tally"]["episodes"]
    # the trajectory's last row is the state the launch left, on every lane that neither finished nor restarted in that step
    last = d["flags"][-1].astype(np.int64)
    calm = (last & (ni._lib.FLAG_TERMINATED | ni._lib.FLAG_TRUNCATED | ni._lib.FLAG_DID_RESET)) == 0
    assert calm.mean() > 0.5
    assert np.array_equal(d["obs"][-1][calm].view(np.uint32), d["state"][calm].view(np.uint32))


def _same_dumps(a, b):
    """The files of two dump directories, loaded from `a`, after checking that `b` holds the same names and bytes."""
    names = sorted(os.listdir(a))
    assert sorted(os.listdir(b)) == names
    d = {}
    for n in names:
        x, y = np.load(a / n), np.load(b / n)
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)), n
        d[n[:-4]] = x
    return d


@pytest.mark.parametrize("form,extra", [("traj_soa", ["--traj", "soa"]), ("outputs_min", ["--outputs", "min"]),
                                        ("outputs_none", ["--outputs", "none"]), ("graph", ["--mode", "graph"])])
def test_dump_outputs_in_every_output_form(tmp_path, form, extra):
    """The other shapes dump_outputs handles: the [T, S, ld] trajectory (transposed to [T, n, S]), reward + flags only, no
    per-step outputs, and the step API (graph mode: the last env.step's reward and flags, one row).  Twice each: same bytes."""
    import bench
    import neorl_industrial_gym_amd as ni
    recs = [_bench(tmp_path / name, extra) for name in ("a", "b")]
    assert recs[0]["tally"] == recs[1]["tally"] and recs[0]["steps"] == K
    d = _same_dumps(tmp_path / "a", tmp_path / "b")
    rows = 1 if form == "graph" else P
    per_step = {"traj_soa": ["flags", "obs", "reward"], "outputs_min": ["flags", "reward"], "outputs_none": [], "graph": ["flags", "reward"]}[form]
    assert sorted(d) == sorted(per_step + ["state", "tally"])
    lanes = bench.dump_lanes(B, (rows * (4 + 8 + (4 * S if "obs" in d else 0)) if per_step else 0) + 4 * S).size
    assert d["state"].shape == (lanes, S) and d["state"].dtype == np.float32 and d["tally"].dtype == np.float64
    assert int(d["tally"][ni._lib.T_EPISODES]) == recs[0]["tally"]["episodes"]
    if per_step:
        assert d["reward"].shape == d["flags"].shape == (rows, lanes) and d["flags"].dtype == np.float64
        assert np.isfinite(d["reward"]).all() and np.array_equal(d["flags"], np.round(d["flags"]))
    if "obs" in d:
        assert d["obs"].shape == (P, lanes, S)
        last = d["flags"][-1].astype(np.int64)
        calm = (last & (ni._lib.FLAG_TERMINATED | ni._lib.FLAG_TRUNCATED | ni._lib.FLAG_DID_RESET)) == 0
        assert calm.mean() > 0.5
        assert np.array_equal(d["obs"][-1][calm].view(np.uint32), d["state"][calm].view(np.uint32))
