"""The footprint checker's own teeth (tests/footprint.py), on the CPU device and without any kernel: arenas are built as
tests/test_gpu_footprint.py builds them, the stray writes that module exists to catch are applied BY HAND, and the checker
must name each with its buffer and region.  This is what keeps the checker from rotting into "always green"."""
import torch

from footprint import KINDS, REDZONE_BYTES, Arena, Layout

B, S, T, LD = 37, 3, 4, 64          # a ragged batch, its wrapper pitch ld = 64, four steps asked for


def _arena():
    """reward rows at out_stride = B + 1, flag rows likewise, an [S][ld_obs] trajectory with a gap behind each step, a
    row-major trajectory (16-byte aligned, stride a multiple of 4 with a gap), an input ring."""
    a = Arena("cpu")
    a.add("reward_out", "f32", Layout(T, B + 1, 1, B + 1, B))
    a.add("flags_out", "flags", Layout(T, B + 1, 1, B + 1, B))
    a.add("obs_soa", "f32", Layout(T, S * (B + 3) + 5, S, B + 3, B))
    a.add("obs_rowmajor", "f32", Layout(T, B * S + 5 + 4, 1, B * S, B * S, lane_width=S), align=16)
    a.add("action_ring", "f32", Layout(2, 2 * (B + 1) + 1, 2, B + 1, B), role="in", extra_outer=0)
    a.build()
    a["action_ring"].data.fill_(0.25)
    a.freeze_inputs()
    return a


def _write_all(a, steps=T):
    """What a correct call leaves: every documented word of the first `steps` steps, nothing else."""
    for name, value in (("reward_out", 1.5), ("obs_soa", 2.5), ("obs_rowmajor", 3.5)):
        a[name].rows(steps).copy_(torch.tensor([value]).view(torch.int32))
    a["flags_out"].rows(steps).fill_(0x00010000)


def _written(steps=T, live=None):
    return {"reward_out": dict(n_outer=steps), "flags_out": dict(n_outer=steps), "obs_soa": dict(n_outer=steps, live=live),
            "obs_rowmajor": dict(n_outer=steps, live=live)}


def _strs(findings):
    return sorted(str(f) for f in findings)


def test_arena_geometry_alignment_and_red_zones():
    a = _arena()
    for kind, t in a.tensors.items():
        isz = t.element_size()
        bufs = sorted((b for b in a.bufs.values() if b.kind == kind), key=lambda b: b.off)
        assert bufs[0].off * isz >= REDZONE_BYTES and (t.numel() - bufs[-1].off - bufs[-1].size) * isz >= REDZONE_BYTES
        for x, y in zip(bufs, bufs[1:]):
            assert (y.off - x.off - x.size) * isz >= REDZONE_BYTES
        assert bool((t == KINDS[kind][2]).sum() == t.numel() - sum(b.size for b in bufs if b.role == "in"))
    assert a["reward_out"].ptr % 256 == 4 and a["flags_out"].ptr % 256 == 4 and a["action_ring"].ptr % 256 == 4   # element-aligned only
    assert a["obs_rowmajor"].ptr % 256 == 16                                                                      # 16 bytes and only 16
    assert a["reward_out"].size == (T + 1) * (B + 1)            # full documented size + the row behind the last step


def test_a_correct_call_has_no_findings():
    a = _arena()
    _write_all(a)
    assert a.check(_written()) == []
    live = torch.ones(T, B, dtype=torch.bool)
    live[2:, 5] = False                                         # lane 5 frozen from step 2 on: its trajectory rows stay canary
    b = _arena()
    _write_all(b)
    for name in ("obs_soa", "obs_rowmajor"):
        canary = KINDS["f32"][2]
        if name == "obs_soa":
            b[name].rows()[2:, :, 5] = canary
        else:
            b[name].rows()[2:, 0, 5 * S:6 * S] = canary
    assert b.check(_written(live=live)) == []
    assert "unwritten" in str(b.check(_written()))              # and without the mask the same rows are missing writes


def test_one_word_in_a_pad_column_is_reported():
    a = _arena()
    _write_all(a)
    a["obs_soa"].data[1 * (S * (B + 3) + 5) + 2 * (B + 3) + B] = 0.0        # step 1, row 2, column B: the first pad column
    f = a.check(_written())
    assert _strs(f) == [f"obs_soa: 1 word(s), pad column (first at element {1 * (S * (B + 3) + 5) + 2 * (B + 3) + B})"]


def test_a_row_written_at_the_wrong_pitch_is_reported():
    """The call said out_stride = B + 1; a kernel that used the wrapper's pitch ld = 64 puts row k at k * 64."""
    a = _arena()
    _write_all(a)
    r = a["reward_out"]
    r.rows(T).fill_(KINDS["f32"][2])                            # undo the correct rows: write them at pitch LD instead
    t, word = a.tensors["f32"], int(torch.tensor([1.5]).view(torch.int32))
    for k in range(T):                                          # (through the arena: the last row ends past the buffer)
        t[r.off + k * LD:r.off + k * LD + B] = word
    f = a.check(_written())
    regions = {x.region for x in f if x.buffer == "reward_out"}
    assert regions == {"pad column", "unwritten", "row beyond n_steps", "red zone after the buffer"}, _strs(f)
    assert all(x.buffer == "reward_out" for x in f)


def test_sixteen_bytes_past_a_row_major_block_are_reported():
    a = _arena()
    _write_all(a)
    o = a["obs_rowmajor"]
    o.data[B * S:B * S + 4] = 7.0                                # behind step 0's block: the gap before step 1
    f = a.check(_written())
    assert _strs(f) == [f"obs_rowmajor: 4 word(s), stride gap (first at element {B * S})"]
    # ... and behind the LAST block of a buffer that ends there: the red zone
    c = Arena("cpu")
    c.add("obs_rowmajor", "f32", Layout(T, B * S + 1, 1, B * S, B * S, lane_width=S), align=16, extra_outer=0)
    c.add("next", "f32", Layout(1, 8, 1, 8, 8))
    c.build()
    c["obs_rowmajor"].rows().fill_(5)
    c["next"].rows().fill_(5)
    t = c.tensors["f32"]
    p = c["obs_rowmajor"].off + c["obs_rowmajor"].size
    t[p:p + 4] = 9
    f = c.check({"obs_rowmajor": dict(n_outer=T), "next": dict(n_outer=1)})
    assert _strs(f) == [f"obs_rowmajor: 4 word(s), red zone after the buffer (first at element {p})"]


def test_a_row_beyond_n_steps_a_missing_write_and_a_changed_input_are_reported():
    a = _arena()
    _write_all(a, steps=T)
    f = a.check(_written(steps=T - 1))                           # the call was asked for T - 1 steps and wrote T
    assert {(x.buffer, x.region) for x in f} == {(n, "row beyond n_steps") for n in ("reward_out", "flags_out", "obs_soa", "obs_rowmajor")}
    b = _arena()
    _write_all(b)
    b["flags_out"].rows()[3, 0, B - 1] = KINDS["flags"][2]       # the last lane of the last step was silently not written
    b["action_ring"].data[B + 2] = 0.5                           # and an input word changed
    f = b.check(_written())
    assert _strs(f) == [f"action_ring: 1 word(s), input changed (first at element {B + 2})",
                        f"flags_out: 1 word(s), unwritten (first at element {3 * (B + 1) + B - 1})"]


def test_a_buffer_that_must_stay_untouched():
    a = _arena()
    a["reward_out"].data[0] = 0.0
    f = a.check({"reward_out": None, "flags_out": None, "obs_soa": None, "obs_rowmajor": None})
    assert _strs(f) == ["reward_out: 1 word(s), row beyond n_steps (first at element 0)"]


def test_explicit_masks_and_partly_written_buffers():
    """A written set that is no rectangle (mixed batches: rows < S of each segment's columns) is given as a mask; a
    library-owned block of which only the surroundings are checked is marked complete=False."""
    a = Arena("cpu").add_and_build("matrix", "f32", Layout(1, 3 * 10, 3, 10, 8), extra_outer=0)
    m = torch.zeros(a["matrix"].size, dtype=torch.bool)
    m.view(3, 10)[:2, 0:3] = True                                # segment 0: two rows of columns 0..2
    m.view(3, 10)[:3, 4:8] = True                                # segment 1: three rows of columns 4..7
    a["matrix"].ints[m] = 1
    assert a.check({"matrix": dict(n_outer=1, mask=m)}) == []
    a["matrix"].data[2 * 10 + 1] = 0.0                           # row 2 of segment 0: not its row
    a["matrix"].data[3] = 0.0                                    # the column between the segments
    f = a.check({"matrix": dict(n_outer=1, mask=m)})
    assert [(x.buffer, x.words) for x in f] == [("matrix", 2)] and f[0].first == 3
    w = Arena("cpu").add_and_build("workspace", "u8", Layout(1, 512, 1, 512, 512), align=256, extra_outer=0)
    w["workspace"].ints[:100] = 0
    assert w.check({"workspace": dict(n_outer=1, complete=False)}) == []
    assert [x.region for x in w.check({"workspace": dict(n_outer=1)})] == ["unwritten"]
    w.tensors["u8"][w["workspace"].off - 1] = 0
    assert _strs(w.check({"workspace": dict(n_outer=1, complete=False)})) == \
        [f"workspace: 1 word(s), red zone before the buffer (first at element {w['workspace'].off - 1})"]


def _hid_arena(H=6, ldh=B + 3, gap=5):
    """hid_out's shape in small: T steps of H unit rows at pitch ldh with a gap behind each step, 16-bit words, element-aligned;
    a second 16-bit buffer behind it, so that the red zone between two buffers of the kind is looked at too."""
    a = Arena("cpu")
    a.add("hid_out", "bf16", Layout(T, H * ldh + gap, H, ldh, B))
    a.add("hid_next", "bf16", Layout(1, 8, 1, 8, 8), extra_outer=0)
    a.build()
    return a


def test_the_16_bit_kind_shows_every_finding_class():
    """pad column, stride gap, row beyond n_steps, frozen lane, red zone, unwritten -- each applied by hand to a buffer of 16-bit
    words and named by the checker, one word at a time."""
    H, ldh, gap = 6, B + 3, 5
    step = H * ldh + gap
    torch_dtype, int_dtype, canary = KINDS["bf16"]
    assert torch_dtype == int_dtype == torch.int16 and canary < 0, "16-bit words; sign bit set: no bf16 word of a ReLU output"
    assert (canary & 0xFFFF) == 0xFA5B
    live = torch.ones(T, B, dtype=torch.bool)
    live[1:, 7] = False                                          # lane 7 frozen from step 1 on
    live[:, B - 1] = False                                       # the last lane held from the start

    def correct():
        a = _hid_arena(H, ldh, gap)
        a["hid_out"].rows().fill_(0x3F80)                        # bf16 1.0
        a["hid_out"].rows()[1:, :, 7] = canary
        a["hid_out"].rows()[:, :, B - 1] = canary
        a["hid_next"].rows().fill_(0)                            # bf16 +0: a written word that is not the canary
        return a

    def written(steps=T, lv=live):
        return {"hid_out": dict(n_outer=steps, live=None if lv is None else lv[:steps]), "hid_next": dict(n_outer=1)}

    a = correct()
    assert a["hid_out"].ptr % 256 == 2 and a["hid_out"].ints.element_size() == 2       # element-aligned only
    t = a.tensors["bf16"]
    assert (a["hid_next"].off - a["hid_out"].off - a["hid_out"].size) * 2 >= REDZONE_BYTES and a["hid_out"].off * 2 >= REDZONE_BYTES
    assert a.check(written()) == []
    cases = [("pad column", 2 * step + 3 * ldh + B),             # step 2, unit row 3, the first pad column
             ("stride gap", 1 * step + H * ldh),                 # behind step 1's last unit row
             ("row beyond n_steps", T * step + 4),               # the step behind the last (memory the buffer owns)
             ("frozen lane", 2 * step + 5 * ldh + 7),            # lane 7 in step 2
             ("frozen lane", 0 * step + 0 * ldh + B - 1)]        # the held lane in step 0
    for region, elem in cases:
        a = correct()
        a["hid_out"].ints[elem] = 0x4000
        assert _strs(a.check(written())) == [f"hid_out: 1 word(s), {region} (first at element {elem})"], region
    for side, off in (("before", -1), ("after", a["hid_out"].size)):
        a = correct()
        p = a["hid_out"].off + off
        a.tensors["bf16"][p] = 0
        assert _strs(a.check(written())) == [f"hid_out: 1 word(s), red zone {side} the buffer (first at element {p})"]
    a = correct()
    a["hid_out"].rows()[3, 2, 11] = canary                       # a live lane's word silently not written
    assert _strs(a.check(written())) == [f"hid_out: 1 word(s), unwritten (first at element {3 * step + 2 * ldh + 11})"]
    a = correct()
    f = a.check(written(steps=T - 1))                            # asked for T - 1 steps, wrote T
    assert {(x.buffer, x.region) for x in f} == {("hid_out", "row beyond n_steps")}
    a = correct()
    assert {(x.buffer, x.region) for x in a.check(written(lv=None))} == {("hid_out", "unwritten")}   # without the live mask
    a = correct()
    a["hid_out"].ints[0] = 0
    f = a.check({"hid_out": None, "hid_next": dict(n_outer=1)})  # a NULL hid_out's arena: everything is stray
    assert {(x.buffer, x.region) for x in f} == {("hid_out", "row beyond n_steps")}
