"""-m gpu: WHERE the kernels behind include/nig.h write, and that the caller's pitches do not matter.

Every caller buffer of every call lives in a canary arena (tests/footprint.py): only element-aligned (16 bytes and only 16
where the header demands them), red zones of 4 KiB around it, the handle's workspace in an arena of its own.  Per case:

  (a) footprint   every word outside the documented written set still holds its canary -- pad columns, stride gaps, the
                  row behind the last step, red zones, the rows of lanes the header calls untouched, the workspace's pad
                  columns -- every word inside it does not, every input is bit-identical to its copy;
  (b) pitches     the same call at the wrapper's dense pitches (ld = B rounded up to 64), at B + a small odd gap, at a
                  pitch beyond ld that is no multiple of 64 and at pitch == B gives the same bits in every observable;
  (c) input pads  the pad columns and stride gaps of the action ring / noise rows hold zeros in one of those runs, NaN,
                  +inf and 3e38 in the others: out-of-range lanes contribute nothing, nig_reduce_tally included;
  (d) refusals    one below a documented minimum is an error code and writes nothing.

One configuration per env and entry point is anchored to the CPU oracle, so that two runs cannot be wrong together.
Each case forces its kernel form with ni.tune and asserts the form through bench.py's naming rules where one exists
(ChemicalReactor, PowerGrid, RobotAssembly; the other envs have the one-wave kernels only).  Every comparison is on
integer views; the module's only numbers are sizes."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from footprint import KINDS, Arena, Layout

pytestmark = pytest.mark.gpu

NAME = {"cr": "ChemicalReactor-v0", "pg": "PowerGrid-v0", "ra": "RobotAssembly-v0", "acr": "AdvancedChemicalReactor-v0",
        "apg": "AdvancedPowerGrid-v0", "hvac": "HVACControl-v0", "water": "WaterTreatment-v0", "steel": "SteelAnnealing-v0",
        "supply": "SupplyChain-v0"}
NEVER = 1 << 30
SEED = 0x5EED
MODES = ("dense", "odd", "wide", "tight")
POISON = {"dense": 0.0, "odd": float("nan"), "wide": float("inf"), "tight": 3e38}      # what the INPUT pads hold in that run
RAGGED = 3 * 512 + 256 + 37


@pytest.fixture(scope="module")
def ni():
    import neorl_industrial_gym_amd as ni
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    yield ni
    ni.tune(split_blocks=-1, wide_min_blocks=-1)


@pytest.fixture()
def knobs(ni):
    yield
    ni.tune(split_blocks=-1, wide_min_blocks=-1)


def ceil4(n):
    return (n + 3) // 4 * 4


def pitch(mode, B, ld, k=0):
    """A row pitch for `mode`; k tells the pitches of one call apart (every one its own odd gap)."""
    return {"dense": ld, "odd": B + 1 + 2 * k, "wide": ld + 37 + 2 * k, "tight": B}[mode]


def gap(mode, k=0, mult4=False):
    """What a step / slot stride adds to its minimum."""
    if mode in ("dense", "tight"):
        return 0
    return 4 * (1 + k) if mult4 else 3 + 2 * k


class Rig:
    """One handle whose workspace lies in a canary arena, and what every case does with it."""

    def __init__(self, ni, key, B, autoreset=True, max_steps=9, tally=True, env_index0=0):
        self.ni, self.key, self.B, self.L = ni, key, B, ni._lib.lib()
        flags = (ni._lib.F_AUTORESET if autoreset else 0) | (ni._lib.F_TALLY if tally else 0)
        from neorl_industrial_gym_amd.batched import ENV_IDS
        lay = ni._lib.layout_query(ENV_IDS[NAME[key]], B, flags)
        n = int(lay.bytes)
        self.wsa = Arena("cuda").add_and_build("workspace", "u8", Layout(1, n, 1, n, n), align=256, extra_outer=0)
        self.env = ni.make_batched(NAME[key], B, seed=SEED, autoreset=autoreset, tally=tally, max_episode_steps=max_steps,
                                   env_index0=env_index0, workspace=self.wsa["workspace"].ints)
        self.lay, self.S, self.A, self.ld = lay, self.env.state_dim, self.env.action_dim, self.env.ld
        self.h, self.ws0 = self.env._h, None

    def st(self):
        return self.env._stream()

    def reset(self):
        self.env.reset()
        torch.cuda.synchronize()
        self.ws0 = self.wsa["workspace"].ints.clone()

    def workspace_findings(self):
        """Pad columns [B, ld) of state, ctr, life_viol, ep_return and every tally row against the copy taken after
        nig_reset, and the red zones around the workspace."""
        out = [str(f) for f in self.wsa.check({"workspace": dict(n_outer=1, complete=False)})]
        now, lay, ld, B = self.wsa["workspace"].ints, self.lay, self.ld, self.B
        arrays = [("state", lay.off_state, self.S, 4), ("ctr", lay.off_ctr, 1, 4), ("life_viol", lay.off_life_viol, 1, 8)]
        if lay.off_tally >= 0:
            arrays += [("ep_return", lay.off_ep_return, 1, 8), ("tally", lay.off_tally, self.ni._lib.T_ROWS, 8)]
        for name, off, rows, isz in arrays:
            a = now[off:off + rows * ld * isz].view(rows, ld * isz)[:, B * isz:]
            b = self.ws0[off:off + rows * ld * isz].view(rows, ld * isz)[:, B * isz:]
            if not torch.equal(a, b):
                out.append(f"workspace.{name}: {int((a != b).sum())} byte(s) changed in pad columns")
        return out

    def final(self):
        """Every observable a launch leaves in the handle, as CPU integer tensors."""
        e = self.env
        torch.cuda.synchronize()
        o = {"state": e.state_soa.contiguous().view(torch.int32).cpu(), "ctr": e.ctr.cpu(), "life_viol": e.life_viol.cpu(),
             "counter": torch.tensor([e.counter])}
        if e.tally is not None:
            o["ep_return"] = e.ep_return.contiguous().view(torch.int64).cpu()
            o["tally"] = e.tally.contiguous().view(torch.int64).cpu()
            o["reduce_tally"] = e.reduce_tally().view(torch.int64).cpu()
        return o

    def hold(self, lanes):
        """Mark `lanes` done through nig_set_state's counter words: frozen until a nig_reset, on an auto-reset handle too."""
        c = self.env.ctr.clone()
        c[lanes] |= self.ni._lib.CTR_DONE
        assert self.L.nig_set_state(self.h, None, self.B, C.c_void_p(c.data_ptr()), self.st()) == 0, self.L.nig_last_error()
        torch.cuda.synchronize()

    def close(self):
        self.env.close()

    # ---- inputs -------------------------------------------------------------------------------------------------
    def add_ring(self, arena, mode, R, layout="rows"):
        """Register the action ring: [A][ld_act] rows, or row-major [B][A] slots ("aos16": 16-byte aligned slots with a
        stride that is a multiple of 4, the native read where a form has one; "aos4": element-aligned, odd stride)."""
        B, A = self.B, self.A
        if layout == "rows":
            lda = pitch(mode, B, self.ld)
            lay = Layout(R, A * lda + gap(mode), A, lda, B)
            return arena.add("action_ring", "f32", lay, role="in", extra_outer=0), lda, lay.outer_stride
        stride = ceil4(B * A) + gap(mode, mult4=True) if layout == "aos16" else (B * A + gap(mode)) | 1
        lay = Layout(R, stride, 1, B * A, B * A, lane_width=A)
        return arena.add("action_ring", "f32", lay, align=16 if layout == "aos16" else "elem", role="in", extra_outer=0), 0, stride

    def fill_ring(self, ring, lda, t0, poison):
        """Slot s = the generator's action stream at launch counter t0 + s (nig_fill_actions at the ring's own pitch for
        rows -- which must leave the pads alone), then every pad column and stride gap is set to `poison`."""
        L, lay = self.L, ring.layout
        if lda:
            for s in range(lay.n_outer):
                assert L.nig_fill_actions(self.h, t0 + s, C.c_void_p(ring.at(s * lay.outer_stride)), lda, self.st()) == 0, L.nig_last_error()
            torch.cuda.synchronize()
        else:
            tmp = torch.empty(self.A, self.ld, dtype=torch.float32, device="cuda")
            for s in range(lay.n_outer):
                self.env.fill_actions(t0 + s, tmp)
                ring.rows()[s, 0].copy_(tmp[:, :self.B].t().contiguous().view(torch.int32).reshape(-1))
        W = ring.geometry_mask()
        assert bool((ring.ints[~W] == KINDS["f32"][2]).all()), "nig_fill_actions wrote outside [A][B]"
        assert bool((ring.ints[W] != KINDS["f32"][2]).all())
        ring.data[~W] = poison


def same(a, b, what):
    assert a.keys() == b.keys(), (what, sorted(a), sorted(b))
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and not a[k].dtype.is_floating_point, (what, k)
        assert torch.equal(a[k], b[k]), f"{what}: observable {k}: {int((a[k] != b[k]).sum())} word(s) differ"


def clean(findings, what):
    assert not findings, what + ":\n  " + "\n  ".join(str(f) for f in findings)


def kernel_of(ni, key, B, outputs):
    """bench.py's naming rule: which kernel form nig_rollout takes.  It names the instantiations the bench times (no outputs,
    reward + flags, row-major trajectory = 0, 1, 3); an [S][ld_obs] trajectory takes the same form as the row-major one."""
    import bench
    out = {"none": "none", "rows": "min", "last": "min"}.get(outputs, "full")
    return bench.rollout_kernel_name(types.SimpleNamespace(key=key, B=B, outputs=out, ni=ni))


# ---------------------------------------------------------------------------------------------------------------------
# nig_rollout
# ---------------------------------------------------------------------------------------------------------------------
OUTPUTS = ["none", "rows", "last", "soa", "aos", "soa0", "aos0"]        # *0: out_stride == 0 and obs_step_stride == 0


def run_rollout(ni, key, B, mode, outputs, chunks=(7, 5, 3), R=5, autoreset=True, max_steps=9, ring_layout="rows",
                anchor=False, hold=None):
    """`chunks` launches of nig_rollout on one handle (the ring shorter than, equal to and longer than n_steps), every
    buffer in one arena.  anchor: slot s of a ring as long as the run = the generator's action stream at t = s + 1 and
    launch c starts at its own slot, which is the oracle's free-running rollout.  Returns (observables, findings)."""
    r = Rig(ni, key, B, autoreset=autoreset, max_steps=max_steps)
    S, ld, L = r.S, r.ld, r.L
    a = Arena("cuda")
    R = sum(chunks) if anchor else R
    ring, lda, slot_stride = r.add_ring(a, mode, R, ring_layout)
    overwrite = outputs in ("last", "soa0", "aos0")
    kind = outputs.rstrip("0")
    os_ = pitch(mode, B, ld, 1)
    ldo = pitch(mode, B, ld, 2)
    bufs = []
    for c, T in enumerate(chunks):
        rew = fl = obs = None
        n = 1 if overwrite else T
        if outputs != "none":
            rew = a.add(f"reward_out{c}", "f32", Layout(n, os_, 1, os_, B))
            fl = a.add(f"flags_out{c}", "flags", Layout(n, os_, 1, os_, B))
        if kind == "soa":
            obs = a.add(f"obs_out{c}", "f32", Layout(n, S * ldo + gap(mode, 1), S, ldo, B))
        elif kind == "aos":
            obs = a.add(f"obs_out{c}", "f32", Layout(n, ceil4(B * S) + gap(mode, 1, mult4=True), 1, B * S, B * S, lane_width=S), align=16)
        bufs.append((T, n, rew, fl, obs))
    a.build()
    r.fill_ring(ring, lda, 1, POISON[mode])
    a.freeze_inputs()
    r.reset()
    if hold is not None:                                   # lanes that are done before the first launch: frozen, "held"
        r.hold(hold)
        held = r.env.state_soa[:, hold].contiguous().view(torch.int32)
    obsv, written, slot0 = {}, {}, 0
    for c, (T, n, rew, fl, obs) in enumerate(bufs):
        p = lambda b: None if b is None else C.c_void_p(b.ptr)
        rc = L.nig_rollout(r.h, T, C.c_void_p(ring.at(slot0 * slot_stride)), lda, slot_stride, R - slot0, p(rew), p(fl),
                           0 if overwrite or rew is None else os_, p(obs), ldo if kind == "soa" else 0,
                           0 if overwrite or obs is None else obs.layout.outer_stride, r.st())
        assert rc == 0, L.nig_last_error()
        slot0 += T if anchor else 0
        for b in (rew, fl, obs):
            if b is not None:
                written[b.name] = dict(n_outer=n)
                torch.cuda.synchronize()
                obsv[b.name] = b.rows(n).cpu() if not overwrite else b.rows(1).cpu()
    obsv.update(r.final())
    findings = [str(f) for f in a.check(written)] + r.workspace_findings()
    if hold is not None:                                   # what nig_rollout leaves in a frozen lane's rows (include/nig.h)
        FL = ni._lib
        for c, (T, n, rew, fl, obs) in enumerate(bufs):
            if fl is not None:
                f = fl.rows(n)[:, 0, hold]
                assert bool(((f & FL.FLAG_INACTIVE) != 0).all()) and bool((rew.rows(n)[:, 0, hold] == 0).all())
            if obs is not None and kind == "soa":
                assert torch.equal(obs.rows(n)[:, :, hold], held[None].expand(n, -1, -1))
            if obs is not None and kind == "aos":
                assert torch.equal(obs.rows(n)[:, 0].view(n, B, S)[:, hold], held.t()[None].expand(n, -1, -1))
    r.close()
    return obsv, findings


ROLLOUT_FORMS = [
    # id, env, lanes, tune(split_blocks, wide_min_blocks)
    ("one-wave-cr-1", "cr", 1, (0, NEVER)),
    ("one-wave-pg-63", "pg", 63, (0, NEVER)),
    ("one-wave-ra-65", "ra", 65, (0, NEVER)),
    ("one-wave-cr-full-blocks-and-tail", "cr", RAGGED, (0, NEVER)),
    ("one-wave-pg-full-blocks-and-tail", "pg", RAGGED, (0, NEVER)),
    ("three-wave-cr-one-round-and-tail", "cr", 1024 + 37, (256, NEVER)),
    ("three-wave-cr-two-rounds", "cr", 7 * 256, (4, NEVER)),            # a 3/4-full last round (trajectory launches only)
    ("three-wave-ra-and-tail", "ra", 512 + 50, (256, NEVER)),
    ("wide-512-pg", "pg", RAGGED, (0, 1)),
    ("wide-256-pg", "pg", RAGGED, (0, 256)),
    ("pair-pg", "pg", RAGGED, (256, 256)),           # LDS-resident stepper with a trajectory, register-resident without
    ("one-wave-acr", "acr", 65, (0, NEVER)),
    ("one-wave-apg", "apg", 65, (0, NEVER)),
    ("one-wave-hvac", "hvac", 321, (0, NEVER)),      # S = 18 and 15: the S % 4 != 0 dword branches of the row-major stores
    ("one-wave-water", "water", 321, (0, NEVER)),
    ("one-wave-steel", "steel", 65, (0, NEVER)),
    ("one-wave-supply", "supply", 65, (0, NEVER)),
]
EXPECT = {  # kernel bench.rollout_kernel_name must report for outputs none / reward+flags / trajectory
    "one-wave-cr-1": "rollout_kernel<ChemicalReactor,%d>", "one-wave-pg-63": "rollout_kernel<PowerGrid,%d>",
    "one-wave-ra-65": "rollout_kernel<RobotAssembly,%d>", "one-wave-cr-full-blocks-and-tail": "rollout_kernel<ChemicalReactor,%d>",
    "one-wave-pg-full-blocks-and-tail": "rollout_kernel<PowerGrid,%d>",
    "three-wave-cr-one-round-and-tail": "split_rollout_kernel<ChemicalReactor,%d,4>",
    "three-wave-ra-and-tail": "split_rollout_kernel<RobotAssembly,%d,4>", "wide-512-pg": "rollout_wide_kernel<PowerGrid,%d,512>",
    "wide-256-pg": "rollout_wide_kernel<PowerGrid,%d,256>", "pair-pg": "rollout_pg_pair_kernel<%d>",
}


@pytest.mark.parametrize("outputs", OUTPUTS)
@pytest.mark.parametrize("form", ROLLOUT_FORMS, ids=[f[0] for f in ROLLOUT_FORMS])
def test_rollout_footprint_and_pitch_invariance(ni, knobs, form, outputs):
    """nig_rollout, every kernel form x every output set: (a), (b) and (c) of the module text.  9-step episodes over three
    launches of 7, 5 and 3 steps on a 5-slot ring: wrap inside a call, truncations, terminations, in-kernel resets."""
    fid, key, B, (split, wide) = form
    ni.tune(split_blocks=split, wide_min_blocks=wide)
    out_mode = {"none": 0, "rows": 1, "last": 1}.get(outputs, 3)
    if fid in EXPECT:
        assert kernel_of(ni, key, B, outputs) == EXPECT[fid] % out_mode
    elif fid == "three-wave-cr-two-rounds":          # rounds only for launches that write the observation trajectory
        assert kernel_of(ni, key, B, outputs) == ("split_rollout_kernel<ChemicalReactor,%d,4>" if out_mode >= 2 else "rollout_kernel<ChemicalReactor,%d>") % out_mode
    ref = None
    for mode in MODES:
        o, f = run_rollout(ni, key, B, mode, outputs)
        clean(f, f"{fid} {outputs} {mode}")
        if ref is None:
            ref = o
            assert int(o["tally"][ni._lib.T_EPISODES].view(torch.float64).sum()) > 0
        else:
            same(ref, o, f"{fid} {outputs} dense vs {mode}")
    if outputs in ("last", "soa0", "aos0"):          # "overwrite" keeps the LAST step's values: the strided run's last rows
        strided, f = run_rollout(ni, key, B, "odd", {"last": "rows", "soa0": "soa", "aos0": "aos"}[outputs])
        clean(f, f"{fid} strided twin of {outputs}")
        for k in ref:
            if k[:-1] in ("reward_out", "flags_out", "obs_out"):
                assert torch.equal(ref[k][0], strided[k][-1]), (fid, outputs, k)


@pytest.mark.parametrize("key", list(NAME))
def test_rollout_awkward_pitches_against_the_oracle(ni, knobs, oracle, key):
    """The anchor of the run-against-run comparisons: per env, odd pitches everywhere, row-major trajectory, two launches
    on the default kernel form -- final state words and step counters equal the CPU oracle's free-running rollout."""
    ni.tune(split_blocks=-1, wide_min_blocks=-1)
    B = 256 + 65
    o, f = run_rollout(ni, key, B, "odd", "aos", chunks=(7, 5), anchor=True)
    clean(f, key)
    st, sc, total, _ = oracle.rollout(key, B, 12, seed=SEED, flavor=oracle.MATH_POLY, max_steps=9)
    S = st.shape[1]
    assert np.array_equal(o["state"].numpy().view(np.uint32).reshape(S, B).T, st.view(np.uint32))
    assert np.array_equal(o["ctr"].numpy() & ni._lib.CTR_STEP_MASK, sc)
    assert int(o["tally"][ni._lib.T_EPISODES].view(torch.float64).sum()) == total.episodes > 0


@pytest.mark.parametrize("outputs", ["rows", "soa", "aos"])
@pytest.mark.parametrize("autoreset", [False, True], ids=["no-autoreset", "held-on-autoreset"])
@pytest.mark.parametrize("key,B", [("cr", 65 + 256), ("pg", 63 + 512), ("hvac", 65)])
def test_rollout_frozen_lanes_rows(ni, knobs, key, B, autoreset, outputs):
    """Frozen lanes under nig_rollout: a handle without auto-reset, where lanes finish (5-step episodes) and a few are done
    before the first launch; and an auto-reset handle with a few lanes HELD (marked done through nig_set_state: they wait
    for a nig_reset while the others restart).  What the header now states: a frozen lane's row holds
    NIG_FLAG_INACTIVE | step, reward 0.0f and the state the lane holds -- written, at every pitch, and nothing else is.
    Kernel form: a handle on which a lane can be frozen takes rollout_kernel for every block, whatever the knobs say
    (csrc/nig_launch_plan.hpp plan_rollout: the three-wave, wide and paired forms require `plain` = auto-reset and no
    held lane), so frozen lanes do not exist in the other forms.  No naming rule covers such handles; the cases run with
    the knobs that would select each other form for a plain handle of the size (and with them off) and must give the
    same bits."""
    hold = torch.arange(2, B, 7, device="cuda")
    ref = None
    for split, wide, mode in [(256, 1, m) for m in MODES] + [(0, NEVER, "odd"), (256, 256, "wide")]:
        ni.tune(split_blocks=split, wide_min_blocks=wide)
        if key in ("cr", "pg"):                               # what a plain handle of this size would run under these knobs
            plain = kernel_of(ni, key, B, outputs)
            assert plain.startswith("rollout_kernel") == (split == 0)
        o, f = run_rollout(ni, key, B, mode, outputs, autoreset=autoreset, max_steps=5, hold=hold)
        clean(f, f"{key} frozen {outputs} {mode} knobs {split}/{wide}")
        fl = torch.cat([o[k] for k in sorted(o) if k.startswith("flags_out")])[:, 0]
        inactive = (fl & ni._lib.FLAG_INACTIVE) != 0
        if autoreset:
            want = torch.zeros(B, dtype=torch.bool)
            want[hold.cpu()] = True
            assert torch.equal(inactive, want[None].expand_as(inactive))       # the held lanes and only they, in every step
        else:
            assert bool(inactive[-1].all())                                     # 15 steps of 5-step episodes: all frozen at the end
        ref = ref or o
        same(ref, o, f"{key} frozen {outputs} dense vs {mode}")


@pytest.mark.parametrize("layout,native", [("aos16", True), ("aos4", False)])
@pytest.mark.parametrize("key,B,tune", [("pg", 1024, (0, 1)), ("cr", 1024, (256, NEVER))])
def test_rollout_row_major_ring(ni, knobs, key, B, tune, layout, native):
    """ld_act == 0: 16-byte aligned slots at a stride that is a multiple of 4 (PowerGrid's wide form reads them natively)
    and slots that are only element-aligned at an odd stride (the row copy), both with a gap behind every slot: same bits
    as the [A][ld] rows, ring untouched, nothing written outside.  Native read or row copy is told apart as
    tests/test_gpu_action_layout.py does, by the ring-sized allocation the copy needs (a ring of 8 MiB makes it visible)."""
    ni.tune(split_blocks=tune[0], wide_min_blocks=tune[1])
    assert kernel_of(ni, key, B, "aos") == ("rollout_wide_kernel<PowerGrid,3,512>" if key == "pg" else "split_rollout_kernel<ChemicalReactor,3,4>")
    ref, f = run_rollout(ni, key, B, "odd", "aos", ring_layout="rows")
    clean(f, "rows")
    for mode in ("dense", "odd"):
        o, f = run_rollout(ni, key, B, mode, "aos", ring_layout=layout)
        clean(f, f"{key} {layout} {mode}")
        same(ref, o, f"{key} rows vs {layout} {mode}")
    # which path: one long call on a big ring
    A = 8 if key == "pg" else 3
    R = (8 << 20) // (4 * A * B) + 1
    r = Rig(ni, key, B)
    a = Arena("cuda")
    ring, lda, stride = r.add_ring(a, "odd", R, layout)
    a.build()
    ring.data.fill_(0.25)
    a.freeze_inputs()
    r.reset()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    assert r.L.nig_rollout(r.h, R, C.c_void_p(ring.ptr), 0, stride, R, None, None, 0, None, 0, 0, r.st()) == 0, r.L.nig_last_error()
    torch.cuda.synchronize()
    used = free0 - torch.cuda.mem_get_info()[0]
    clean([str(x) for x in a.check({})] + r.workspace_findings(), f"{key} {layout} long call")
    assert (used < R * A * B * 2) == (native and key == "pg"), (used, R * A * B * 4)
    r.close()


def test_the_checker_sees_a_call_made_at_another_pitch_than_declared(ni, knobs):
    """The device-side path of the checker, shown with a CORRECT kernel: the call is made at out_stride = ld and at
    ld_obs = ld while the checker is told B + 1 -- rows land in what it takes for pad columns, stride gaps and the row
    behind the last step, and the columns it expects stay canary.  (What the checker reports for hand-made stray writes:
    tests/test_footprint_checker.py, on the CPU.)"""
    ni.tune(split_blocks=0, wide_min_blocks=NEVER)
    B, T = 65, 4
    r = Rig(ni, "cr", B)
    S, A, ld = r.S, r.A, r.ld
    a = Arena("cuda")
    ring, lda, slot_stride = r.add_ring(a, "dense", T)
    rew = a.add("reward_out", "f32", Layout(T, B + 1, 1, B + 1, B), extra_outer=T)               # (room for T rows at pitch ld)
    fl = a.add("flags_out", "flags", Layout(T, B + 1, 1, B + 1, B), extra_outer=T)
    obs = a.add("obs_out", "f32", Layout(T, S * (B + 1) + 3, S, B + 1, B), extra_outer=T)
    a.build()
    r.fill_ring(ring, lda, 1, 0.0)
    a.freeze_inputs()
    r.reset()
    assert r.L.nig_rollout(r.h, T, C.c_void_p(ring.ptr), lda, slot_stride, T, C.c_void_p(rew.ptr), C.c_void_p(fl.ptr), ld,
                           C.c_void_p(obs.ptr), ld, S * ld, r.st()) == 0, r.L.nig_last_error()
    torch.cuda.synchronize()
    found = {(f.buffer, f.region) for f in a.check({b.name: dict(n_outer=T) for b in (rew, fl, obs)})}
    for name in ("reward_out", "flags_out", "obs_out"):
        assert {(name, "pad column"), (name, "unwritten"), (name, "row beyond n_steps")} <= found, (name, found)
    assert ("obs_out", "stride gap") in found
    assert not r.workspace_findings()
    r.close()


# ---------------------------------------------------------------------------------------------------------------------
# nig_rollout_noise
# ---------------------------------------------------------------------------------------------------------------------
def _noise_forms():
    # FORMS (and _chain below) come from the module whose kernel forms this test must follow one for one; a rename there
    # has to be made here too -- it fails the collection of this module, which is the reminder
    from test_gpu_noise_rollout import FORMS
    return FORMS


@pytest.mark.parametrize("form", _noise_forms(), ids=[f[0] for f in _noise_forms()])
def test_rollout_noise_footprint_and_pitch_invariance(ni, knobs, form):
    """nig_rollout_noise through every kernel form of tests/test_gpu_noise_rollout.py on the draws of tests/golden/*_g3.npz,
    with ld_noise, both noise step strides, ld_act and out_stride padded and the pads of all three inputs poisoned."""
    from conftest import load_golden
    from test_gpu_noise_rollout import _chain
    _, key, B, _, (split, wide), autoreset, kernel = form
    ni.tune(split_blocks=split, wide_min_blocks=wide)
    if kernel is not None:
        assert kernel_of(ni, key, B, "aos") == kernel
    d = load_golden(key, "g3")
    big = B > 1024                                          # the bench-sized rows: fewer steps, two pitch sets
    T = 6 if big else 12 if autoreset else min(40, int(d["ep_length"].max()))
    act, nz, rz, idx, first = _chain(d, B, T)
    K, KR = d["noise"].shape[1], d["ep_init_noise"].shape[1]
    ref = None
    for mode in MODES[:2] if big else MODES:
        r = Rig(ni, key, B, autoreset=autoreset, max_steps=None)
        S, A, ld = r.S, r.A, r.ld
        a = Arena("cuda")
        lda, ldn, os_ = pitch(mode, B, ld), pitch(mode, B, ld, 1), pitch(mode, B, ld, 2)
        ring = a.add("action_ring", "f32", Layout(T, A * lda + gap(mode), A, lda, B), role="in", extra_outer=0)
        sn = a.add("step_noise", "f64", Layout(T, K * ldn + gap(mode, 1), K, ldn, B), role="in", extra_outer=0) if K else None
        rn = a.add("reset_noise", "f64", Layout(T, KR * ldn + gap(mode, 2), KR, ldn, B), role="in", extra_outer=0) if autoreset else None
        rew = a.add("reward_out", "f32", Layout(T, os_, 1, os_, B))
        fl = a.add("flags_out", "flags", Layout(T, os_, 1, os_, B))
        obs = a.add("obs_out", "f32", Layout(T, ceil4(B * S) + gap(mode, mult4=True), 1, B * S, B * S, lane_width=S), align=16)
        a.build()
        for b, x in ((ring, act), (sn, nz), (rn, rz)):
            if b is not None:
                b.data.fill_(POISON[mode])
                src = torch.from_numpy(np.ascontiguousarray(x)).cuda()
                b.rows().copy_(src.view(torch.int32 if b.kind == "f32" else torch.int64))
        a.freeze_inputs()
        r.env.reset(init_noise=d["ep_init_noise"][first].T)
        torch.cuda.synchronize()
        r.ws0 = r.wsa["workspace"].ints.clone()
        cut = T // 3 + 1
        for t0, t1 in ((0, cut), (cut, T)):
            at = lambda b, stride: None if b is None else C.c_void_p(b.at(t0 * stride))
            rc = r.L.nig_rollout_noise(r.h, t1 - t0, at(ring, ring.layout.outer_stride), lda, ring.layout.outer_stride, T - t0,
                                       at(sn, sn.layout.outer_stride if sn else 0), sn.layout.outer_stride if sn else 0,
                                       at(rn, rn.layout.outer_stride if rn else 0), rn.layout.outer_stride if rn else 0, ldn,
                                       at(rew, os_), at(fl, os_), os_, at(obs, obs.layout.outer_stride), obs.layout.outer_stride, r.st())
            assert rc == 0, r.L.nig_last_error()
        torch.cuda.synchronize()
        o = {b.name: b.rows(T).cpu() for b in (rew, fl, obs)}
        o.update(r.final())
        clean([str(x) for x in a.check({b.name: dict(n_outer=T) for b in (rew, fl, obs)})] + r.workspace_findings(), f"{form[0]} {mode}")
        r.close()
        ref = ref or o
        same(ref, o, f"{form[0]} dense vs {mode}")
    # anchor: the first step's observations are the fixture's (float32 words; ChemicalReactor's concentration column is one
    # np.exp ulp off now and then and RobotAssembly's velocity rows differ, tests/test_gpu_noise_rollout.py -- compared there
    # under the suite's tolerance, here exact on the columns that are).  This is a thin anchor on purpose: the comparison of
    # the WHOLE trajectory, of rewards, flags, restart states and tallies with the reference's recording lives in
    # tests/test_gpu_noise_rollout.py (same forms, dense pitches), and this module relies on it -- what is added here is
    # that padded pitches give the bits of the dense run.
    got = ref["obs_out"][0, 0].view(B, -1).numpy().view(np.uint32)
    want = d["obs"][idx][0].view(np.uint32)
    cols = [c for c in range(got.shape[1]) if not (key == "cr" and c == 4) and not (key == "ra" and c in (14, 15, 16))]
    assert np.array_equal(got[:, cols], want[:, cols])


# ---------------------------------------------------------------------------------------------------------------------
# nig_rollout_policy / nig_rollout_mlp / nig_rollout_mlp_safe
# ---------------------------------------------------------------------------------------------------------------------
def _policy(ni, key, which, S, A):
    if which == "affine":
        if key in ("cr", "pg", "ra"):
            return ni.behaviour_policy(NAME[key], "medium")
        rng = np.random.default_rng(3)                       # the policy of tests/test_spec_envs.py::test_policy_rollout_bit_identical
        W = np.zeros((A, S), dtype=np.float32)
        W[:, :5] = rng.normal(0, 0.01, (A, 5))
        return ni.DevicePolicy(S, A, W=W, b=rng.normal(0, 0.2, A), sigma=np.full(A, 0.1), half_range=np.linspace(0, 0.2, A),
                               p_uniform=0.1, uniform_range=0.9, clip=(-1.0, 1.0))
    return {"pid": ni.pid_agent, "uniform": ni.random_agent}[which](S, A)


def _actor(S, A, seed):
    rng = np.random.default_rng(seed)
    return [(rng.normal(0, 1.0 / np.sqrt(S), (S, 256)).astype(np.float32) * np.float32(0.05), rng.normal(0, 0.05, 256).astype(np.float32)),
            (rng.normal(0, 1.0 / 16, (256, 256)).astype(np.float32), rng.normal(0, 0.05, 256).astype(np.float32)),
            (rng.normal(0, 1.0 / 8, (256, A)).astype(np.float32), rng.normal(0, 0.1, A).astype(np.float32))]


def _critic(S, A, seed):
    rng = np.random.default_rng(seed)
    D = S + A
    return [(rng.normal(0, 1.0 / np.sqrt(D), (D, 256)).astype(np.float32) * np.float32(0.05), rng.normal(0, 0.05, 256).astype(np.float32)),
            (rng.normal(0, 1.0 / 16, (256, 256)).astype(np.float32), rng.normal(0, 0.05, 256).astype(np.float32)),
            (rng.normal(0, 1.0 / 2, (256, 1)).astype(np.float32), rng.normal(0, 0.1, 1).astype(np.float32))]


def run_closed_loop(ni, key, B, mode, subset, entry="policy", which="affine", chunks=(6, 4), autoreset=True, max_steps=7,
                    hold=None, overwrite=False, threshold=0.5):
    """nig_rollout_policy / _mlp / _mlp_safe / _mlp_bf16: `subset` of "o" (obs_out), "a" (act_out), "r" (reward_out), "f" (flags_out),
    "p" (prob_out), "h" (hid_out: 512 rows of 16-bit words per step at a pitch of its own).  Frozen lanes (no auto-reset; `hold` =
    done before the first launch) leave their obs / act / prob / hid rows untouched and get NIG_FLAG_INACTIVE | step and reward
    0.0f.  Returns (observables, findings, rig's policy)."""
    r = Rig(ni, key, B, autoreset=autoreset, max_steps=max_steps)
    S, A, ld, L, FL = r.S, r.A, r.ld, r.L, ni._lib
    pol = None
    if entry == "policy":
        pol = _policy(ni, key, which, S, A)
        r.env.set_policy(pol)
    elif entry == "mlp_bf16":
        r.env.set_mlp_policy_bf16(_actor(S, A, 11))
    else:
        r.env.set_mlp_policy(_actor(S, A, 11))
        if entry == "mlp_safe":
            r.env.set_mlp_safety(_critic(S, A, 12), threshold)
    a = Arena("cuda")
    os_, lda, ldh = pitch(mode, B, ld, 1), pitch(mode, B, ld, 2), pitch(mode, B, ld, 3)
    assert set(subset) <= set("oarfph") and ("h" not in subset or entry == "mlp_bf16") and ("p" not in subset or entry == "mlp_safe")
    bufs = []
    for c, T in enumerate(chunks):
        n = 1 if overwrite else T
        rew = a.add(f"reward_out{c}", "f32", Layout(n, os_, 1, os_, B)) if "r" in subset else None
        fl = a.add(f"flags_out{c}", "flags", Layout(n, os_, 1, os_, B)) if "f" in subset else None
        pr = a.add(f"prob_out{c}", "f32", Layout(n, os_, 1, os_, B)) if "p" in subset else None
        obs = a.add(f"obs_out{c}", "f32", Layout(T, ceil4(B * S) + gap(mode, 1, mult4=True), 1, B * S, B * S, lane_width=S), align=16) if "o" in subset else None
        act = a.add(f"act_out{c}", "f32", Layout(T, A * lda + gap(mode, 2), A, lda, B)) if "a" in subset else None
        hid = a.add(f"hid_out{c}", "bf16", Layout(T, 512 * ldh + gap(mode, 3), 512, ldh, B)) if "h" in subset else None
        bufs.append((T, n, rew, fl, pr, obs, act, hid))
    a.build()
    r.reset()
    if hold is not None:
        r.hold(hold)
    obsv, written = {}, {}
    p = lambda b: None if b is None else C.c_void_p(b.ptr)
    for c, (T, n, rew, fl, pr, obs, act, hid) in enumerate(bufs):
        # who is live in step k of this launch: not done on entry of the step (a handle without auto-reset never revives a lane)
        args = [r.h, T, p(rew), p(fl), 0 if overwrite else os_, p(obs), obs.layout.outer_stride if obs else 0, p(act), lda if act else 0,
                act.layout.outer_stride if act else 0]
        done0 = (r.env.ctr & FL.CTR_DONE) != 0
        if entry == "policy":
            rc = L.nig_rollout_policy(*args, r.st())
        elif entry == "mlp":
            rc = L.nig_rollout_mlp(*args, r.st())
        elif entry == "mlp_bf16":
            rc = L.nig_rollout_mlp_bf16(*args, p(hid), ldh if hid else 0, hid.layout.outer_stride if hid else 0, r.st())
        else:
            rc = L.nig_rollout_mlp_safe(*args, p(pr), r.st())
        assert rc == 0, L.nig_last_error()
        torch.cuda.synchronize()
        live = None
        if not autoreset:
            assert fl is not None and not overwrite, "a case with frozen lanes records its flag rows"
            f = fl.rows(T)[:, 0]
            live = (f & FL.FLAG_INACTIVE) == 0
            ended = ((f & (FL.FLAG_TERMINATED | FL.FLAG_TRUNCATED)) != 0) & live
            # consistency of the mask itself: live in step 0 <=> not done on entry; live in step k+1 <=> live and not ended in k
            assert torch.equal(live[0], ~done0) and torch.equal(live[1:], live[:-1] & ~ended[:-1])
            if rew is not None:
                assert bool((rew.rows(T)[:, 0][~live] == 0).all())
        for b in (rew, fl, pr, obs, act, hid):
            if b is not None:
                per_lane = b in (obs, act, pr, hid)
                written[b.name] = dict(n_outer=n if b in (rew, fl, pr) else T, live=live if per_lane and live is not None else None)
                obsv[b.name] = b.rows(written[b.name]["n_outer"]).cpu()
        if live is not None:
            obsv[f"live{c}"] = live.cpu()
    obsv.update(r.final())
    findings = [str(f) for f in a.check(written)] + r.workspace_findings()
    r.close()
    return obsv, findings, pol


POLICY_FORMS = [
    # id, env, lanes, split_blocks, policy kind, kernel bench.policy_kernel_name must report (None: no naming rule for the env)
    ("one-wave-cr", "cr", 321, 0, "affine", "rollout_policy_kernel<ChemicalReactor>"),
    ("one-wave-cr-1", "cr", 1, 0, "uniform", "rollout_policy_kernel<ChemicalReactor>"),
    ("one-wave-pg-pid", "pg", 256 + 63, 256, "pid", "rollout_policy_kernel<PowerGrid>"),
    ("three-wave-cr-ragged-tail", "cr", 1024 + 100, 256, "affine", "split_policy_kernel<ChemicalReactor,4>"),
    ("three-wave-cr-in-rounds", "cr", 7 * 256, 4, "pid", "split_policy_kernel<ChemicalReactor,4>"),
    ("pair-pg", "pg", 512 + 77, 256, "affine", "rollout_pg_pair_policy_kernel<PolicyArgs> (pg_policy_reg_body)"),
    ("three-wave-ra", "ra", 256 + 50, 256, "affine", "split_policy_kernel<RobotAssembly,4>"),
    ("one-wave-hvac", "hvac", 65, 256, "affine", None),
    ("one-wave-water", "water", 65, 256, "uniform", None),
]
SUBSETS = ["oarf", "o", "a", "rf", "r", "oa", "arf", "orf", ""]        # "": no output at all -- only the handle may change


@pytest.mark.parametrize("subset", SUBSETS)
@pytest.mark.parametrize("form", POLICY_FORMS, ids=[f[0] for f in POLICY_FORMS])
def test_policy_rollout_footprint_and_pitch_invariance(ni, knobs, form, subset):
    """nig_rollout_policy: every kernel form x each subset of obs_out / act_out / reward+flags (and reward alone)."""
    import bench
    fid, key, B, split, which, kernel = form
    ni.tune(split_blocks=split, wide_min_blocks=-1)
    if kernel is not None:
        if fid == "three-wave-cr-in-rounds" and "o" not in subset:             # a second round only with the observation stream
            kernel = "rollout_policy_kernel<ChemicalReactor>"
        assert bench.policy_kernel_name(ni, key, B, which if which == "pid" else "affine", stream_obs="o" in subset) == kernel
    ref = None
    for mode in MODES:
        o, f, _ = run_closed_loop(ni, key, B, mode, subset, which=which)
        clean(f, f"{fid} {subset} {mode}")
        ref = ref or o
        same(ref, o, f"{fid} {subset} dense vs {mode}")
    assert int(ref["tally"][ni._lib.T_EPISODES].view(torch.float64).sum()) > 0


@pytest.mark.parametrize("form", POLICY_FORMS, ids=[f[0] for f in POLICY_FORMS])
def test_policy_rollout_frozen_lanes_and_overwrite(ni, knobs, form):
    """Handles without auto-reset (one-wave kernels whatever the knob): finished and held lanes leave obs / act rows untouched
    at every pitch; and out_stride == 0 keeps the last step's reward / flag row."""
    fid, key, B, split, which, _ = form
    ni.tune(split_blocks=split, wide_min_blocks=-1)
    hold = torch.arange(1, B, 5, device="cuda")
    ref = None
    for mode in MODES:
        o, f, _ = run_closed_loop(ni, key, B, mode, "oarf", which=which, autoreset=False, max_steps=4, hold=hold)
        clean(f, f"{fid} frozen {mode}")
        assert not bool(o["live1"][-1].any()) and bool(o["live0"][0].any())
        ref = ref or o
        same(ref, o, f"{fid} frozen dense vs {mode}")
    strided, f, _ = run_closed_loop(ni, key, B, "odd", "rf", which=which)
    clean(f, f"{fid} strided")
    last, f, _ = run_closed_loop(ni, key, B, "wide", "rf", which=which, overwrite=True)
    clean(f, f"{fid} overwrite")
    for k in ("reward_out0", "flags_out0", "reward_out1", "flags_out1"):
        assert torch.equal(last[k][0], strided[k][-1]), (fid, k)


BIG = 131072 + 256 + 37


@pytest.mark.parametrize("key", ["cr", "hvac", "water"])
def test_policy_rollout_transposed_branch_at_large_batch(ni, knobs, oracle, key):
    """Above 131 072 lanes rollout_policy_kernel writes row-major observations through the per-wave LDS transpose as whole
    16-byte lines while every lane of a wave is live: whole waves, the partial last wave (37 lanes) and waves that hold
    frozen lanes (every fifth lane of the second block and of the last is done before the launch; all lanes are truncated
    after 4 steps).  HVACControl (S = 18) and WaterTreatment (S = 15) take the guarded tail of that store (16 S % 64 != 0),
    the only thing between a wave's last line and the next wave's rows.  Footprint at odd pitches, the same bits at
    dense ones, and the oracle's closed loop for every live lane."""
    ni.tune(split_blocks=-1, wide_min_blocks=-1)
    B = BIG
    hold = torch.cat([torch.arange(256 + 1, 512, 5), torch.arange(B - 37 - 64, B, 5)]).cuda()
    o, f, pol = run_closed_loop(ni, key, B, "odd", "oarf", chunks=(4, 3), autoreset=False, max_steps=4, hold=hold)
    clean(f, f"{key} big odd")
    d, f, _ = run_closed_loop(ni, key, B, "dense", "oarf", chunks=(4, 3), autoreset=False, max_steps=4, hold=hold)
    clean(f, f"{key} big dense")
    same(d, o, f"{key} big dense vs odd")
    assert bool(o["live0"][0].sum() == B - hold.numel()) and not bool(o["live1"].any())
    P = oracle.Policy.from_buffer_copy(bytes(pol.to_struct()))
    r = oracle.rollout_policy(key, B, 4, P, seed=SEED, max_steps=4, autoreset=False, trajectories=True)
    live = o["live0"].numpy()
    assert np.array_equal(live | np.isin(np.arange(B), hold.cpu().numpy())[None], r["live"].astype(bool))
    S = r["obs"].shape[2]
    got = o["obs_out0"][:, 0].numpy().view(np.uint32).reshape(4, B, S)
    assert np.array_equal(got[live], r["obs"].view(np.uint32)[live])
    act = o["act_out0"].numpy().view(np.uint32).transpose(0, 2, 1)
    assert np.array_equal(act[live], r["act"].view(np.uint32)[live])
    free = ~np.isin(np.arange(B), hold.cpu().numpy())
    assert np.array_equal(o["state"].numpy().view(np.uint32).reshape(S, B).T[free], r["state"].view(np.uint32)[free])


MLP_CASES = [("mlp", "oarf", True), ("mlp", "a", True), ("mlp_safe", "oarfp", True), ("mlp_safe", "p", True), ("mlp_safe", "ap", True),
             ("mlp", "oarf", False), ("mlp_safe", "oarfp", False), ("mlp_safe", "fp", False)]   # frozen lanes are told from the flag rows


@pytest.mark.parametrize("entry,subset,autoreset", MLP_CASES, ids=[f"{e}-{s}-{'autoreset' if a else 'frozen'}" for e, s, a in MLP_CASES])
@pytest.mark.parametrize("B", [1, 33, 129, 3000])
@pytest.mark.parametrize("key", ["cr", "pg", "apg"])
def test_mlp_rollouts_footprint_and_pitch_invariance(ni, knobs, key, B, autoreset, entry, subset):
    """The MFMA actor alone and with the safety-critic shield (32 lanes per wave, 128 per block; AdvancedPowerGrid's critic
    layer 1 comes in two chunks): prob_out with and without reward / flags, auto-reset handles and frozen lanes."""
    ref = None
    for mode in ("dense", "odd", "wide") if B > 1 else MODES:
        o, f, _ = run_closed_loop(ni, key, B, mode, subset, entry=entry, autoreset=autoreset, max_steps=4 if not autoreset else 7)
        clean(f, f"{key} {B} {entry} {subset} {mode}")
        ref = ref or o
        same(ref, o, f"{key} {B} {entry} {subset} dense vs {mode}")
    assert int(ref["tally"][ni._lib.T_EPISODES].view(torch.float64).sum()) > 0


@pytest.mark.parametrize("key", ["cr", "pg", "apg"])
def test_mlp_rollout_awkward_pitches_against_the_oracle(ni, knobs, oracle, key):
    """Anchor of the MLP cases: tight pitches (pitch == B = 129), final state and step counters == oracle.rollout_mlp; the shielded
    entry point at a threshold no p reaches (2.0) leaves the same state."""
    B, T = 129, 10
    o, f, _ = run_closed_loop(ni, key, B, "tight", "oarf", entry="mlp")
    clean(f, key)
    s, f, _ = run_closed_loop(ni, key, B, "odd", "oarfp", entry="mlp_safe", threshold=2.0)
    clean(f, key + " safe")
    S = o["state"].shape[0]
    ws = _actor(S, s["act_out0"].shape[1], 11)
    r = oracle.rollout_mlp(key, B, T, ws, seed=SEED, max_steps=7, autoreset=True, trajectories=True)
    for run in (o, s):
        assert np.array_equal(run["state"].numpy().view(np.uint32).reshape(S, B).T, r["state"].view(np.uint32))
        assert np.array_equal(run["ctr"].numpy() & ni._lib.CTR_STEP_MASK, r["step"])
    for k in ("act_out0", "act_out1", "obs_out0", "obs_out1", "reward_out0", "flags_out1"):
        assert torch.equal(o[k], s[k]), k
    # out_stride == 0: one reward / flag / prob row, holding the last step's values
    last, f, _ = run_closed_loop(ni, key, B, "wide", "rfp", entry="mlp_safe", threshold=2.0, overwrite=True)
    clean(f, key + " safe, overwrite")
    for k in ("reward_out0", "flags_out0", "prob_out0", "reward_out1", "flags_out1", "prob_out1"):
        assert torch.equal(last[k][0], s[k][-1]), k


BF16_CASES = [("oarfh", True), ("h", True), ("a", True), ("rf", True), ("", True), ("oarfh", False), ("fh", False)]


@pytest.mark.parametrize("subset,autoreset", BF16_CASES, ids=[f"{s or 'none'}-{'autoreset' if a else 'frozen'}" for s, a in BF16_CASES])
@pytest.mark.parametrize("B", [1, 33, 129, 700])
@pytest.mark.parametrize("key", ["cr", "hvac", "supply"])
def test_mlp_bf16_footprint_and_pitch_invariance(ni, knobs, key, B, autoreset, subset):
    """The MFMA actor on the bf16 matrix unit (a kernel body of its own; 32 lanes per wave on both lane halves, 128 per block):
    ChemicalReactor (S 12: the 16-byte observation store, 3 head rows), HVACControl (S 18: scalar observation stores) and
    SupplyChain (S 28, A 10: head rows 8 and 9 from the second register group); hid_out at a pitch of its own, from both lane
    halves; every output alone, none at all, and frozen lanes told from the flag rows.  Pitch == B at one lane and at one lane
    past a block."""
    ref = None
    for mode in MODES if B in (1, 129) else ("dense", "odd", "wide"):
        o, f, _ = run_closed_loop(ni, key, B, mode, subset, entry="mlp_bf16", autoreset=autoreset, max_steps=4 if not autoreset else 7)
        clean(f, f"{key} {B} mlp_bf16 {subset} {mode}")
        ref = ref or o
        same(ref, o, f"{key} {B} mlp_bf16 {subset} dense vs {mode}")
    assert int(ref["tally"][ni._lib.T_EPISODES].view(torch.float64).sum()) > 0
    if subset == "":                                        # the outputs do not change the trajectory
        full, f, _ = run_closed_loop(ni, key, B, "dense", "oarfh", entry="mlp_bf16", autoreset=autoreset, max_steps=7)
        clean(f, f"{key} {B} mlp_bf16 oarfh dense")
        for k in ("state", "ctr", "tally", "life_viol", "ep_return", "reduce_tally", "counter"):
            assert torch.equal(ref[k], full[k]), (key, B, k)


# ---------------------------------------------------------------------------------------------------------------------
# nig_step / nig_step64 / nig_plan_*
# ---------------------------------------------------------------------------------------------------------------------
def run_steps(ni, key, B, mode, kind, T=12, max_steps=5):
    """T calls of nig_step (kind "fast" / "parity") or nig_step64 ("f64") with actions, noise rows, reward, reward64, flags
    and final_obs in arenas; final_obs rows of lanes that did not finish in the call stay untouched."""
    r = Rig(ni, key, B, max_steps=max_steps)
    S, A, ld, L, FL = r.S, r.A, r.ld, r.L, ni._lib
    K, KR = int(r.env.spec.k_step), int(r.env.spec.k_reset)
    a = Arena("cuda")
    lda, ldn, ldo = pitch(mode, B, ld), pitch(mode, B, ld, 1), pitch(mode, B, ld, 2)
    act = a.add("actions", "f64" if kind == "f64" else "f32", Layout(T, A * lda + gap(mode), A, lda, B), role="in", extra_outer=0)
    sn = a.add("step_noise", "f64", Layout(T, K * ldn + gap(mode, 1), K, ldn, B), role="in", extra_outer=0) if kind == "parity" and K else None
    rn = a.add("reset_noise", "f64", Layout(T, KR * ldn + gap(mode, 2), KR, ldn, B), role="in", extra_outer=0) if kind == "parity" else None
    outs = [(a.add(f"reward_out{t}", "f32", Layout(1, B + 3, 1, B + 3, B)), a.add(f"reward64_out{t}", "f64", Layout(1, B + 3, 1, B + 3, B)),
             a.add(f"flags_out{t}", "flags", Layout(1, B + 3, 1, B + 3, B)), a.add(f"final_obs{t}", "f32", Layout(1, S * ldo + 5, S, ldo, B)))
            for t in range(T)]
    a.build()
    g = torch.Generator(device="cpu").manual_seed(5)
    for b, lo, hi in ((act, -1.5, 1.5), (sn, -2.0, 2.0), (rn, 0.0, 1.0)):
        if b is not None:
            L_ = b.layout
            x = torch.rand((L_.n_outer, L_.n_rows, B), generator=g, dtype=torch.float64) * (hi - lo) + lo
            b.data.fill_(POISON[mode])
            b.rows().copy_(x.to(KINDS[b.kind][0]).cuda().view(KINDS[b.kind][1]))
    a.freeze_inputs()
    r.reset()
    obsv, written = {}, {}
    fn = L.nig_step64 if kind == "f64" else L.nig_step
    at = lambda b, t: None if b is None else C.c_void_p(b.at(t * b.layout.outer_stride))
    for t, (rew, r64, fl, fo) in enumerate(outs):
        rc = fn(r.h, at(act, t), lda, at(sn, t), at(rn, t), ldn if kind == "parity" else 0, C.c_void_p(rew.ptr), C.c_void_p(r64.ptr),
                C.c_void_p(fl.ptr), C.c_void_p(fo.ptr), ldo, r.st())
        assert rc == 0, L.nig_last_error()
    torch.cuda.synchronize()
    finished = 0
    for t, (rew, r64, fl, fo) in enumerate(outs):
        f = fl.rows(1)[:, 0]
        done = (f & (FL.FLAG_TERMINATED | FL.FLAG_TRUNCATED)) != 0
        finished += int(done.sum())
        for b in (rew, r64, fl):
            written[b.name] = dict(n_outer=1)
        written[fo.name] = dict(n_outer=1, live=done)
        for b in (rew, r64, fl, fo):
            obsv[b.name] = b.rows(1).cpu()
    assert finished > 0
    obsv.update(r.final())
    findings = [str(f) for f in a.check(written)] + r.workspace_findings()
    r.close()
    return obsv, findings


@pytest.mark.parametrize("kind", ["fast", "parity", "f64"])
@pytest.mark.parametrize("key,B", [("cr", 1000), ("pg", 1024), ("ra", 1000), ("water", 1000)])
def test_step_footprint_and_pitch_invariance(ni, knobs, key, B, kind):
    """nig_step in fast and parity mode and nig_step64, through the step kernel with helper waves (knob at 256: one wave per
    SIMD; ChemicalReactor, PowerGrid, RobotAssembly) and the plain one (knob 0; WaterTreatment has the plain one only),
    final_obs and reward64_out included; both forms and all pitches leave the same bits.  The two forms are told apart by
    the knob alone: no naming rule exists for the step kernel, so which one ran is not asserted here (nor is it in
    tests/test_gpu_split.py, which selects them the same way)."""
    ref = None
    for split in (256, 0):
        ni.tune(split_blocks=split, wide_min_blocks=-1)
        for mode in MODES:
            o, f = run_steps(ni, key, B, mode, kind)
            clean(f, f"{key} {B} {kind} split_blocks={split} {mode}")
            ref = ref or o
            same(ref, o, f"{key} {B} {kind} dense vs split_blocks={split} {mode}")


@pytest.mark.parametrize("key,B", [("cr", 1000), ("pg", 1024), ("ra", 1000), ("water", 1000)])
def test_step_awkward_pitches_against_the_oracle(ni, knobs, oracle, key, B):
    """Anchor of the step cases: nig_step in fast mode on the generator's own action stream (nig_fill_actions into an
    arena at an odd pitch), default knobs: state words and step counters after 12 steps equal the oracle's rollout."""
    ni.tune(split_blocks=-1, wide_min_blocks=-1)
    T = 12
    r = Rig(ni, key, B, max_steps=5)
    a = Arena("cuda")
    lda = B + 3
    act = a.add("actions", "f32", Layout(T, r.A * lda + 5, r.A, lda, B), role="in", extra_outer=0)
    fl = a.add("flags_out", "flags", Layout(T, B + 1, 1, B + 1, B))
    a.build()
    r.fill_ring(act, lda, 1, float("nan"))
    a.freeze_inputs()
    r.reset()
    for t in range(T):
        assert r.L.nig_step(r.h, C.c_void_p(act.at(t * act.layout.outer_stride)), lda, None, None, 0, None, None,
                            C.c_void_p(fl.at(t * (B + 1))), None, 0, r.st()) == 0, r.L.nig_last_error()
    o = r.final()
    clean([str(x) for x in a.check({"flags_out": dict(n_outer=T)})] + r.workspace_findings(), key)
    st, sc, total, _ = oracle.rollout(key, B, T, seed=SEED, flavor=oracle.MATH_POLY, max_steps=5)
    assert np.array_equal(o["state"].numpy().view(np.uint32).reshape(r.S, B).T, st.view(np.uint32))
    assert np.array_equal(o["ctr"].numpy() & ni._lib.CTR_STEP_MASK, sc)
    assert int(o["tally"][ni._lib.T_EPISODES].view(torch.float64).sum()) == total.episodes > 0
    r.close()


@pytest.mark.parametrize("overwrite", [False, True], ids=["padded-out-stride", "out-stride-0"])
@pytest.mark.parametrize("key,B", [("cr", 1000), ("pg", 1024)])
def test_plan_footprint_and_pitch_invariance(ni, knobs, key, B, overwrite):
    """nig_plan_create / nig_plan_launch: the hipGraph of 7 step launches on a 5-slot ring, replayed twice.  The reward / flag
    outputs are rings like the actions (include/nig.h: slot s = k % ring_len at base + s * out_stride): five padded slots,
    nothing behind them, or one overwritten row (the step kernel is anchored by test_step_awkward_pitches_against_the_oracle)."""
    ni.tune(split_blocks=-1, wide_min_blocks=-1)
    T, R, ref = 7, 5, None
    for mode in MODES:
        r = Rig(ni, key, B, max_steps=5)
        a = Arena("cuda")
        ring, lda, slot_stride = r.add_ring(a, mode, R)
        os_, n = pitch(mode, B, r.ld, 1), 1 if overwrite else min(T, R)
        rew = a.add("reward_out", "f32", Layout(n, os_, 1, os_, B))
        fl = a.add("flags_out", "flags", Layout(n, os_, 1, os_, B))
        a.build()
        r.fill_ring(ring, lda, 1, POISON[mode])
        a.freeze_inputs()
        r.reset()
        plan = C.c_void_p()
        assert r.L.nig_plan_create(r.h, T, C.c_void_p(ring.ptr), lda, slot_stride, R, C.c_void_p(rew.ptr), C.c_void_p(fl.ptr),
                                   0 if overwrite else os_, C.byref(plan)) == 0, r.L.nig_last_error()
        o = {}
        for rep in range(2):
            assert r.L.nig_plan_launch(plan, r.st()) == 0, r.L.nig_last_error()
            torch.cuda.synchronize()
            o[f"reward{rep}"], o[f"flags{rep}"] = rew.rows(n).cpu(), fl.rows(n).cpu()
        o.update(r.final())
        clean([str(x) for x in a.check({"reward_out": dict(n_outer=n), "flags_out": dict(n_outer=n)})] + r.workspace_findings(), f"{key} plan {mode}")
        assert r.L.nig_plan_destroy(plan) == 0
        r.close()
        ref = ref or o
        same(ref, o, f"{key} plan dense vs {mode}")
    assert ref["counter"].item() == 2 * T


# ---------------------------------------------------------------------------------------------------------------------
# nig_rollout_mixed / nig_rollout_mixed_obs
# ---------------------------------------------------------------------------------------------------------------------
MIX = [("cr", 300), ("ra", 257), ("hvac", 200), ("water", 511), ("steel", 64), ("pg", 333), ("supply", 129)]


@pytest.mark.parametrize("with_obs", [False, True], ids=["mixed", "mixed_obs"])
def test_mixed_rollout_footprint_and_pitch_invariance(ni, knobs, with_obs):
    """Seven env types with ragged segment sizes in one launch, handles bound (nig_bind_state) into a state matrix that lies
    in an arena at a padded pitch: the columns between the segments, the rows >= S of a segment, the pads of ld_act /
    out_stride / ld_obs stay untouched; every segment's final state equals the same handle rolled alone."""
    ni.tune(split_blocks=-1, wide_min_blocks=-1)
    offs, off = [], 0
    for _, n in MIX:
        offs.append(off)
        off += (n + 255) // 256 * 256
    cols, T, R = offs[-1] + MIX[-1][1], 6, 4                     # the last documented column; pitches are measured from it
    ref = None
    for mode in MODES:
        rigs = [Rig(ni, k, n, max_steps=5, env_index0=o) for (k, n), o in zip(MIX, offs)]
        Smax, Amax = max(r.S for r in rigs), max(r.A for r in rigs)
        ld = (cols + 63) // 64 * 64
        lds, lda, os_, ldo = pitch(mode, cols, ld), pitch(mode, cols, ld, 1), pitch(mode, cols, ld, 2), pitch(mode, cols, ld, 3)
        a = Arena("cuda")
        state = a.add("bound_state", "f32", Layout(1, Smax * lds, Smax, lds, cols), extra_outer=0)
        ring = a.add("action_ring", "f32", Layout(R, Amax * lda + gap(mode), Amax, lda, cols), role="in", extra_outer=0)
        rew = a.add("reward_out", "f32", Layout(T, os_, 1, os_, cols))
        fl = a.add("flags_out", "flags", Layout(T, os_, 1, os_, cols))
        obs = a.add("obs_out", "f32", Layout(T, Smax * ldo + gap(mode, 1), Smax, ldo, cols)) if with_obs else None
        a.build()
        seg1 = torch.zeros(cols, dtype=torch.bool, device="cuda")              # columns that belong to a segment
        segS = torch.zeros(Smax, cols, dtype=torch.bool, device="cuda")        # ... and rows < S of it
        ring.data.fill_(POISON[mode])
        for r, o in zip(rigs, offs):
            seg1[o:o + r.B] = True
            segS[:r.S, o:o + r.B] = True
            assert r.L.nig_bind_state(r.h, C.c_void_p(state.at(o)), lds) == 0, r.L.nig_last_error()
            for s in range(R):
                assert r.L.nig_fill_actions(r.h, 1 + s, C.c_void_p(ring.at(s * ring.layout.outer_stride + o)), lda, r.st()) == 0
        a.freeze_inputs()
        for r in rigs:
            r.reset()
        hs = (C.c_void_p * len(rigs))(*[r.h for r in rigs])
        lo = (C.c_int64 * len(rigs))(*offs)
        L = rigs[0].L
        for rep in range(2):
            if with_obs:
                rc = L.nig_rollout_mixed_obs(hs, lo, len(rigs), T, C.c_void_p(ring.ptr), lda, ring.layout.outer_stride, R, C.c_void_p(rew.ptr),
                                             C.c_void_p(fl.ptr), os_, C.c_void_p(obs.ptr), ldo, obs.layout.outer_stride, rigs[0].st())
            else:
                rc = L.nig_rollout_mixed(hs, lo, len(rigs), T, C.c_void_p(ring.ptr), lda, ring.layout.outer_stride, R, C.c_void_p(rew.ptr),
                                         C.c_void_p(fl.ptr), os_, rigs[0].st())
            assert rc == 0, L.nig_last_error()
        torch.cuda.synchronize()

        def mask_of(b, m2d, n):
            m = torch.zeros(b.size, dtype=torch.bool, device="cuda")
            Lb = b.layout
            torch.as_strided(m, (n, Lb.n_rows, Lb.n_cols), (Lb.outer_stride, Lb.pitch, 1)).copy_(m2d[None].expand(n, -1, -1))
            return m
        written = {"bound_state": dict(n_outer=1, mask=mask_of(state, segS, 1)), "reward_out": dict(n_outer=T, mask=mask_of(rew, seg1[None], T)),
                   "flags_out": dict(n_outer=T, mask=mask_of(fl, seg1[None], T))}
        if with_obs:
            written["obs_out"] = dict(n_outer=T, mask=mask_of(obs, segS, T))
        findings = [str(x) for x in a.check(written)]
        o = {b.name: b.rows(n).cpu() for b, n in ((state, 1), (rew, T), (fl, T))}
        if with_obs:
            o["obs_out"] = obs.rows(T).cpu()
        for i, r in enumerate(rigs):
            findings += r.workspace_findings()
            fin = r.final()
            fin.pop("state")                                              # (the bound matrix holds it)
            o.update({f"{k}{i}": v for k, v in fin.items()})
        clean(findings, f"mixed {mode}")
        if ref is None:                                                   # anchor: every segment alone, through nig_rollout
            for i, ((k, n), off_) in enumerate(zip(MIX, offs)):
                alone = ni.make_batched(NAME[k], n, seed=SEED, env_index0=off_, autoreset=True, tally=True, max_episode_steps=5)
                rg = torch.empty(R, alone.action_dim, alone.ld, dtype=torch.float32, device="cuda")
                for s in range(R):
                    alone.fill_actions(1 + s, rg[s])
                alone.reset()
                alone.rollout(T, rg)
                alone.rollout(T, rg)
                torch.cuda.synchronize()
                got = state.rows(1)[0, :alone.state_dim, off_:off_ + n]
                assert torch.equal(got, alone.state_soa.contiguous().view(torch.int32)), k
                assert torch.equal(o[f"ctr{i}"], alone.ctr.cpu())
                alone.close()
        for r in rigs:
            r.close()
        ref = ref or o
        same(ref, o, f"mixed dense vs {mode}")


# ---------------------------------------------------------------------------------------------------------------------
# nig_fill_actions, nig_get_state / nig_set_state, nig_get_safety_metrics, nig_bind_state, nig_reset with a mask
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["cr", "water", "supply"])
def test_small_entry_points_footprint_and_pitch_invariance(ni, knobs, key):
    B, ref = 257, None
    for mode in MODES:
        r = Rig(ni, key, B, max_steps=5)
        S, A, ld, L = r.S, r.A, r.ld, r.L
        p = [pitch(mode, B, ld, k) for k in range(5)]
        a = Arena("cuda")
        bound = a.add("bound_state", "f32", Layout(1, S * p[0], S, p[0], B), extra_outer=0)
        act = a.add("actions", "f32", Layout(1, A * p[1], A, p[1], B), extra_outer=0)
        got = a.add("get_state", "f32", Layout(1, S * p[2], S, p[2], B), extra_outer=0)
        gctr = a.add("get_ctr", "flags", Layout(1, B, 1, B, B), extra_outer=0)
        src = a.add("set_state", "f32", Layout(1, S * p[3], S, p[3], B), role="in", extra_outer=0)
        sctr = a.add("set_ctr", "flags", Layout(1, B, 1, B, B), role="in", extra_outer=0)
        mask = a.add("reset_mask", "u8", Layout(1, B, 1, B, B), role="in", extra_outer=0)
        fl = a.add("flags", "flags", Layout(1, B, 1, B, B))
        rew = a.add("reward", "f32", Layout(1, B, 1, B, B))
        met = a.add("metrics", "i32", Layout(1, 5 * p[4], 5, p[4], B), extra_outer=0)
        a.build()
        assert L.nig_bind_state(r.h, C.c_void_p(bound.ptr), p[0]) == 0, L.nig_last_error()
        src.data.fill_(POISON[mode])
        sctr.data.fill_(3)
        mask.ints.copy_((torch.arange(mask.size) % 3 == 0).to(torch.uint8))
        a.freeze_inputs()
        r.reset()
        st = r.st()
        assert L.nig_fill_actions(r.h, 7, C.c_void_p(act.ptr), p[1], st) == 0
        assert L.nig_step(r.h, C.c_void_p(act.ptr), p[1], None, None, 0, C.c_void_p(rew.ptr), None, C.c_void_p(fl.ptr), None, 0, st) == 0
        assert L.nig_get_safety_metrics(r.h, C.c_void_p(fl.ptr), C.c_void_p(met.ptr), p[4], st) == 0
        assert L.nig_get_state(r.h, C.c_void_p(got.ptr), p[2], C.c_void_p(gctr.ptr), st) == 0
        torch.cuda.synchronize()
        o = {b.name: b.rows().cpu() for b in (bound, act, got, gctr, fl, rew, met)}
        assert torch.equal(o["bound_state"], o["get_state"]) and bool(((o["get_ctr"] & ni._lib.CTR_STEP_MASK) == 1).all())
        # teacher forcing from the copy (its pads poisoned), then a masked reset: lanes outside the mask keep the forced state
        src.rows().copy_(got.rows())
        a.freeze_inputs()
        assert L.nig_set_state(r.h, C.c_void_p(src.ptr), p[3], C.c_void_p(sctr.ptr), st) == 0
        assert L.nig_reset(r.h, C.c_void_p(mask.ptr), None, 0, st) == 0
        torch.cuda.synchronize()
        o["after_reset"] = bound.rows().cpu()
        keep = (mask.ints == 0).cpu()
        assert torch.equal(o["after_reset"][0][:, keep], o["get_state"][0][:, keep])
        assert bool((r.env.ctr.cpu()[keep] == 3).all()) and bool((r.env.ctr.cpu()[~keep] == 0).all())
        w = {b.name: dict(n_outer=1) for b in (bound, act, got, gctr, fl, rew, met)}
        clean([str(x) for x in a.check(w)] + r.workspace_findings(), f"{key} small entry points {mode}")
        r.close()
        ref = ref or o
        same(ref, o, f"{key} small entry points dense vs {mode}")


# ---------------------------------------------------------------------------------------------------------------------
# (d) boundary refusals
# ---------------------------------------------------------------------------------------------------------------------
class RefusalRig:
    """A handle with every policy installed and full-size buffers for every entry point, all at the wrapper's pitch ld."""

    def __init__(self, ni, key):
        B, T, R = 321, 3, 3
        r = Rig(ni, key, B, max_steps=5)
        S, A, ld = r.S, r.A, r.ld
        K, KR = int(r.env.spec.k_step), int(r.env.spec.k_reset)
        self.closed_loop = S % 2 == 0                      # (the MFMA actor needs an even state dim)
        if self.closed_loop:
            r.env.set_policy(ni.behaviour_policy(NAME[key], "medium"))
            r.env.set_mlp_policy(_actor(S, A, 11))
            r.env.set_mlp_safety(_critic(S, A, 12), 0.5)
            r.env.set_mlp_ensemble([_actor(S, A, 13), _actor(S, A, 14)], weights=[0.5, 0.5], method="mean")
        a = Arena("cuda")
        nk = max(K, KR, 1)
        self.ring = a.add("action_ring", "f32", Layout(R, A * ld, A, ld, B), role="in")
        self.act64 = a.add("actions64", "f64", Layout(1, A * ld, A, ld, B), role="in")
        self.nz = a.add("noise", "f64", Layout(T, nk * ld, nk, ld, B), role="in")
        self.rew = a.add("reward_out", "f32", Layout(T, ld, 1, ld, B))
        self.fl = a.add("flags_out", "flags", Layout(T, ld, 1, ld, B))
        self.pr = a.add("prob_out", "f32", Layout(T, ld, 1, ld, B))
        self.obs = a.add("obs_out", "f32", Layout(T, S * ld + 4, S, ld, B), align=16)     # serves both trajectory layouts
        self.act = a.add("act_out", "f32", Layout(T, A * ld, A, ld, B))
        self.met = a.add("metrics", "i32", Layout(1, 5 * ld, 5, ld, B))
        a.build()
        self.ring.data.fill_(0.25)
        self.act64.data.fill_(0.25)
        self.nz.data.fill_(0.5)
        a.freeze_inputs()
        r.reset()
        self.r, self.a, self.B, self.T, self.R, self.S, self.A, self.ld, self.K, self.KR = r, a, B, T, R, S, A, ld, K, KR
        self.nothing = {b.name: None for b in (self.rew, self.fl, self.pr, self.obs, self.act, self.met)}

    def close(self):
        self.r.close()


def _refusal_rows(key):
    """(what, call(rig, v) with the argument under test = v, the documented minimum, the offending value, what the error
    text must say).  The at-minimum twin of every row must be ACCEPTED (the positive control: the row's other arguments are
    valid), the offending value refused with a message that names the argument's check."""
    P = lambda b, elems=0: C.c_void_p(b.ptr + 4 * elems)
    rows = []

    def row(what, call, good, bad, text):
        rows.append((what, call, good, bad, text))

    def base(g):
        return g.r.L, g.r.h, g.r.st(), g.B, g.T, g.R, g.S, g.A, g.ld

    # ---- nig_step64: envs with their own float64 arithmetic (cr) and envs that narrow the rows first (water) -------------
    def step64(what, text, lda=None, ldn=None, ldo=None):
        def call(g, v):
            L, h, st, B, T, R, S, A, ld = base(g)
            nz = C.c_void_p(g.nz.ptr) if ldn else None
            return L.nig_step64(h, C.c_void_p(g.act64.ptr), v if lda else ld, nz, nz, v if ldn else 0, P(g.rew), None, P(g.fl),
                                P(g.obs) if ldo else None, v if ldo else 0, st)
        row(f"nig_step64 {what}", call, "B", "B-1", text)
    step64("ld_act", "nig_step64: actions NULL or ld_act", lda=True)
    step64("ld_noise", "nig_step64: ld_noise outside", ldn=True)
    step64("ld_obs", "nig_step64: ld_obs outside", ldo=True)
    if key != "cr":
        return rows

    # ---- nig_rollout / nig_rollout_noise (one implementation, two argument lists) -------------------------------------------
    def rollout(what, text, good, bad, noise=False, **kw):
        def call(g, v):
            L, h, st, B, T, R, S, A, ld = base(g)
            q = dict(lda=ld, slot=A * ld, ring_len=R, out=ld, obs=None, ldo=0, ostep=0, ldn=ld, sstep=g.K * ld, rstep=g.KR * ld)
            if noise:
                q.update(obs=P(g.obs), ostep=ceil4(S * B))
            q.update({k: (f(g, v) if callable(f) else f) for k, f in kw.items()})
            if noise:
                nz = C.c_void_p(g.nz.ptr)
                return L.nig_rollout_noise(h, T, P(g.ring), q["lda"], q["slot"], q["ring_len"], nz, q["sstep"], nz, q["rstep"], q["ldn"],
                                           P(g.rew), P(g.fl), q["out"], q["obs"], q["ostep"], st)
            return L.nig_rollout(h, T, P(g.ring), q["lda"], q["slot"], q["ring_len"], P(g.rew), P(g.fl), q["out"], q["obs"], q["ldo"],
                                 q["ostep"], st)
        row(f"{'nig_rollout_noise' if noise else 'nig_rollout'} {what}", call, good, bad, text)
    val = lambda g, v: v
    obs = lambda g, v: P(g.obs)
    for noise in (False, True):
        rollout("ld_act", "ld_act outside", "B", "B-1", noise, lda=val, slot=lambda g, v: g.A * g.ld)
        rollout("slot_stride", "slot_stride smaller than one [A][ld_act]", "A*ld", "A*ld-1", noise, slot=val)
        rollout("out_stride", "out_stride outside", "B", "B-1", noise, out=val)
        rollout("obs_step_stride (row-major)", "row-major trajectory needs", "S*B", "S*B-4", noise, obs=obs, ostep=val)
        rollout("obs_step_stride % 4", "row-major trajectory needs", "S*B+4", "S*B+1", noise, obs=obs, ostep=val)
        rollout("obs_out alignment", "row-major trajectory needs", 0, 1, noise, obs=lambda g, v: P(g.obs, v), ostep=lambda g, v: ceil4(g.S * g.B))
    rollout("slot_stride (row-major ring)", "row-major action ring", "A*B", "A*B-1", lda=0, slot=val)
    rollout("ld_obs", "bad observation trajectory pitch", "B", "B-1", obs=obs, ldo=val, ostep=lambda g, v: g.S * g.ld)
    rollout("obs_step_stride", "bad observation trajectory pitch", "S*ld", "S*ld-1", obs=obs, ldo=lambda g, v: g.ld, ostep=val)
    rollout("ld_noise", "ld_noise outside", "B", "B-1", True, ldn=val)
    rollout("step_noise_stride", "step_noise NULL or its step stride", "K*ld", "K*ld-1", True, sstep=val)
    rollout("reset_noise_stride", "needs reset_noise", "KR*ld", "KR*ld-1", True, rstep=val)
    rollout("ring_len", "ring_len >= n_steps", "T", "T-1", True, ring_len=val)

    # ---- nig_step, nig_plan_create, the small entry points -------------------------------------------------------------------
    def simple(what, text, good, bad, call):
        row(what, call, good, bad, text)
    nzp = lambda g: C.c_void_p(g.nz.ptr)
    simple("nig_step ld_act", "nig_step: actions NULL or ld_act", "B", "B-1",
           lambda g, v: g.r.L.nig_step(g.r.h, P(g.ring), v, None, None, 0, P(g.rew), None, P(g.fl), None, 0, g.r.st()))
    simple("nig_step ld_noise", "nig_step: ld_noise outside", "B", "B-1",
           lambda g, v: g.r.L.nig_step(g.r.h, P(g.ring), g.ld, nzp(g), nzp(g), v, P(g.rew), None, P(g.fl), None, 0, g.r.st()))
    simple("nig_step ld_obs", "nig_step: ld_obs outside", "B", "B-1",
           lambda g, v: g.r.L.nig_step(g.r.h, P(g.ring), g.ld, None, None, 0, P(g.rew), None, P(g.fl), P(g.obs), v, g.r.st()))

    def plan(what, text, good, bad, **kw):
        def call(g, v):
            q = dict(lda=g.ld, slot=g.A * g.ld, out=g.ld)
            q.update({k: f(g, v) for k, f in kw.items()})
            p = C.c_void_p()
            rc = g.r.L.nig_plan_create(g.r.h, g.T, P(g.ring), q["lda"], q["slot"], g.R, P(g.rew), P(g.fl), q["out"], C.byref(p))
            if rc == 0:
                assert g.r.L.nig_plan_destroy(p) == 0
            return rc
        row(f"nig_plan_create {what}", call, good, bad, text)
    plan("ld_act", "nig_plan_create: bad argument", "B", "B-1", lda=val, slot=lambda g, v: g.A * g.ld)
    plan("ld_act == 0 (no row-major ring)", "nig_plan_create: bad argument", "B", 0, lda=val, slot=lambda g, v: g.A * g.ld)
    plan("slot_stride", "slot_stride smaller than one [A][ld_act]", "A*ld", "A*ld-1", slot=val)
    plan("out_stride", "out_stride < batch", "B", "B-1", out=val)
    simple("nig_fill_actions ld_act", "nig_fill_actions: bad argument", "B", "B-1",
           lambda g, v: g.r.L.nig_fill_actions(g.r.h, 1, P(g.act), v, g.r.st()))
    simple("nig_get_state ld", "nig_get_state: ld < batch", "B", "B-1", lambda g, v: g.r.L.nig_get_state(g.r.h, P(g.obs), v, None, g.r.st()))
    simple("nig_set_state ld", "nig_set_state: ld < batch", "B", "B-1", lambda g, v: g.r.L.nig_set_state(g.r.h, P(g.ring), v, None, g.r.st()))
    simple("nig_get_safety_metrics ld_out", "nig_get_safety_metrics: bad argument", "B", "B-1",
           lambda g, v: g.r.L.nig_get_safety_metrics(g.r.h, P(g.fl), P(g.met), v, g.r.st()))
    simple("nig_bind_state ld", "nig_bind_state: ld outside", "B", "B-1", lambda g, v: g.r.L.nig_bind_state(g.r.h, P(g.obs), v))
    simple("nig_reset ld_noise", "nig_reset: ld_noise < batch", "B", "B-1", lambda g, v: g.r.L.nig_reset(g.r.h, None, nzp(g), v, g.r.st()))

    # ---- closed loops ----------------------------------------------------------------------------------------------------------
    def closed(name, what, text, good, bad, **kw):
        def call(g, v):
            L, h, st, B, T, R, S, A, ld = base(g)
            q = dict(out=ld, obs=P(g.obs), ostep=ceil4(S * B), lda=ld, astep=A * ld)
            q.update({k: f(g, v) for k, f in kw.items()})
            extra = {"nig_rollout_mlp_safe": (P(g.pr),), "nig_rollout_mlp_ensemble": (P(g.pr), None)}.get(name, ())
            return getattr(L, name)(h, T, P(g.rew), P(g.fl), q["out"], q["obs"], q["ostep"], P(g.act), q["lda"], q["astep"], *extra, st)
        row(f"{name} {what}", call, good, bad, text)
    for name in ("nig_rollout_policy", "nig_rollout_mlp", "nig_rollout_mlp_safe", "nig_rollout_mlp_ensemble"):
        closed(name, "out_stride", name + ": out_stride outside", "B", "B-1", out=val)
        closed(name, "obs_step_stride", name + ": obs_out needs 16-byte alignment", "S*B", "S*B-4", ostep=val)
        closed(name, "obs_step_stride == 0 (no overwrite form)", name + ": obs_out needs 16-byte alignment", "S*B", 0, ostep=val)
        closed(name, "obs_step_stride % 4", name + ": obs_out needs 16-byte alignment", "S*B+4", "S*B+1", ostep=val)
        closed(name, "obs_out alignment", name + ": obs_out needs 16-byte alignment", 0, 1, obs=lambda g, v: P(g.obs, v))
        closed(name, "ld_act", name + ": bad action trajectory pitch", "B", "B-1", lda=val)
        closed(name, "act_step_stride", name + ": bad action trajectory pitch", "A*ld", "A*ld-1", astep=val)

    # ---- mixed launches (one handle at column 0) ----------------------------------------------------------------------------------
    def mixed(what, text, good, bad, with_obs, **kw):
        def call(g, v):
            L, h, st, B, T, R, S, A, ld = base(g)
            q = dict(lda=ld, slot=A * ld, out=ld, ldo=ld, ostep=S * ld)
            q.update({k: f(g, v) for k, f in kw.items()})
            hs, lo = (C.c_void_p * 1)(h), (C.c_int64 * 1)(0)
            if with_obs:
                return L.nig_rollout_mixed_obs(hs, lo, 1, T, P(g.ring), q["lda"], q["slot"], R, P(g.rew), P(g.fl), q["out"], P(g.obs),
                                               q["ldo"], q["ostep"], st)
            return L.nig_rollout_mixed(hs, lo, 1, T, P(g.ring), q["lda"], q["slot"], R, P(g.rew), P(g.fl), q["out"], st)
        row(f"{'nig_rollout_mixed_obs' if with_obs else 'nig_rollout_mixed'} {what}", call, good, bad, text)
    for with_obs in (False, True):
        mixed("ld_act", "does not fit the row pitch", "B", "B-1", with_obs, lda=val, slot=lambda g, v: g.A * g.ld)
        mixed("out_stride", "does not fit the row pitch", "B", "B-1", with_obs, out=val)
        mixed("slot_stride", "slot_stride smaller than one [A_max][ld_act]", "A*ld", "A*ld-1", with_obs, slot=val)
    mixed("ld_obs", "does not fit ld_obs", "B", "B-1", True, ldo=val, ostep=lambda g, v: g.S * g.ld)
    mixed("obs_step_stride", "obs_step_stride smaller than one [S_max][ld_obs]", "S*ld", "S*ld-1", True, ostep=val)
    return rows


@pytest.mark.parametrize("key", ["cr", "water"])
def test_one_below_every_documented_minimum_is_refused_and_writes_nothing(ni, knobs, key):
    """Every pitch / stride argument of every entry point one below its documented minimum (and the alignment rules of the
    row-major trajectories broken by one element): an error code whose text names the check, every arena still canary, the
    workspace and the launch counter unchanged -- and, as the positive control, the same argument list AT the minimum is
    accepted, so no row is refused for another reason.  nig_step64 is checked on an env with its own float64 arithmetic
    (ChemicalReactor) and on one whose rows are narrowed first (WaterTreatment).  All buffers have their full size, so even
    a wrongly accepted call stays inside the arena (it is listed, and the next row starts from a fresh handle and arena)."""
    ni.tune(split_blocks=-1, wide_min_blocks=-1)
    wrong = []
    for what, call, good, bad, text in _refusal_rows(key):
        g = RefusalRig(ni, key)
        sym = dict(B=g.B, T=g.T, S=g.S, A=g.A, ld=g.ld, K=g.K, KR=g.KR)
        value = lambda x: x if isinstance(x, int) else int(eval(x, {}, sym))
        rc = call(g, value(bad))
        msg = g.r.L.nig_last_error().decode()
        torch.cuda.synchronize()
        if rc == 0:
            wrong.append(f"{what} = {bad}: accepted")
        else:
            if text not in msg:
                wrong.append(f"{what} = {bad}: refused for another reason: {msg!r}")
            assert g.r.env.counter == 0, what
            clean([str(x) for x in g.a.check(g.nothing)], what + " (refused, yet wrote)")
            assert torch.equal(g.r.wsa["workspace"].ints, g.r.ws0), what + ": refused, yet the workspace changed"
            rc = call(g, value(good))
            torch.cuda.synchronize()
            if rc != 0:
                wrong.append(f"{what} = {good} (the minimum itself): refused: {g.r.L.nig_last_error().decode()!r}")
        g.close()
    assert not wrong, "\n".join(wrong)
