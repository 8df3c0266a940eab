"""Canary arenas for the footprint tests (tests/test_gpu_footprint.py; the checker itself: tests/test_footprint_checker.py).

Every caller buffer of a call is carved out of ONE larger tensor per element kind, pre-filled with a canary word no kernel
can produce, with a red zone of canary before and after each buffer.  After the call(s) `Arena.check` compares the whole
arena, as INTEGERS, with what the header (include/nig.h) says the call writes and reports every word that is wrong:

    pad column          a changed word in columns [n_cols, pitch) of a written row
    stride gap          a changed word between the end of a row set / block and the next step's
    row beyond n_steps  a changed word in a step the call was not asked for
    frozen lane         a changed word of a lane the header says stays untouched
    red zone            a changed word outside every buffer (named after the nearest one)
    unwritten           a word of the documented written set that still holds the canary
    input changed       any changed word of an input buffer (compared with the copy taken by `freeze_inputs`)

Sizes are the module's only numbers: the red zone is 4 KiB at least -- more than the widest burst one wave can store
(64 lanes x 16 B = 1 KiB), with room for a few rows."""
from dataclasses import dataclass
from typing import Dict, List, Optional

import torch

REDZONE_BYTES = 4096

# kind -> (torch dtype the kernels see, integer dtype used for every comparison, canary as that integer)
KINDS = {
    "f32": (torch.float32, torch.int32, 0x7FC0BEEF),                 # quiet NaN with a payload (hardware NaNs: 0x7FC00000)
    "f64": (torch.float64, torch.int64, 0x7FF8BEEF0BADF00D),         # likewise
    "flags": (torch.int32, torch.int32, -1),                         # 0xFFFFFFFF: step field 65 535 > NIG_MAX_EPISODE_STEPS
    "i32": (torch.int32, torch.int32, 0x5A5A5A5B),                   # fixed odd patterns
    "i64": (torch.int64, torch.int64, 0x5A5A5A5B5A5A5A5B),
    "u8": (torch.uint8, torch.uint8, 0xA5),
    # bf16 words of a ReLU output (hid_out of nig_rollout_mlp_bf16): 0xFA5B has its sign bit set and h >= +0, so no stored word is it
    "bf16": (torch.int16, torch.int16, 0xFA5B - 0x10000),
}


@dataclass
class Layout:
    """Geometry of a buffer: n_outer steps at outer_stride elements, each n_rows rows at `pitch` elements, n_cols written
    columns per row.  A row-major [B][S] block is one row of B*S columns (lane_width = S columns per lane); an overwritten
    ("stride 0") output is one step."""
    n_outer: int
    outer_stride: int
    n_rows: int
    pitch: int
    n_cols: int
    lane_width: int = 1

    def min_size(self):
        return (self.n_outer - 1) * self.outer_stride + (self.n_rows - 1) * self.pitch + self.n_cols


class Buf:
    def __init__(self, arena, name, kind, size, layout, align, role):
        self.arena, self.name, self.kind, self.size, self.layout, self.align, self.role = arena, name, kind, size, layout, align, role
        self.off = None          # element offset inside the arena tensor (set by Arena.build)

    @property
    def ints(self) -> torch.Tensor:
        """The buffer's words as the integer tensor every comparison uses."""
        return self.arena.tensors[self.kind][self.off:self.off + self.size]

    @property
    def data(self) -> torch.Tensor:
        """The buffer as the kernels see it (float32 / float64 / int32 ...): a view, writes go to the arena."""
        return self.ints.view(KINDS[self.kind][0])

    @property
    def ptr(self) -> int:
        return self.ints.data_ptr()

    def at(self, elem: int) -> int:
        """Device address of element `elem` (a slot or a step inside the buffer)."""
        assert 0 <= elem < self.size
        return self.ptr + elem * self.ints.element_size()

    def rows(self, n_outer: Optional[int] = None) -> torch.Tensor:
        """Strided INTEGER view [n_outer, n_rows, n_cols] of the documented columns (read or fill through it)."""
        L = self.layout
        n = L.n_outer if n_outer is None else n_outer
        return torch.as_strided(self.ints, (n, L.n_rows, L.n_cols), (L.outer_stride, L.pitch, 1))

    def geometry_mask(self, n_outer: Optional[int] = None, live: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Bool mask over the buffer's elements: the documented columns of the first n_outer steps; `live` (bool
        [n_outer, lanes]) removes the columns of lanes the header says stay untouched in that step."""
        L = self.layout
        n = L.n_outer if n_outer is None else n_outer
        m = torch.zeros(self.size, dtype=torch.bool, device=self.ints.device)
        view = torch.as_strided(m, (n, L.n_rows, L.n_cols), (L.outer_stride, L.pitch, 1))
        if live is None:
            view.fill_(True)
        else:
            lv = live.to(m.device).repeat_interleave(L.lane_width, dim=1) if L.lane_width > 1 else live.to(m.device)
            assert lv.shape == (n, L.n_cols), (lv.shape, n, L.n_cols)
            view.copy_(lv[:, None, :].expand(n, L.n_rows, L.n_cols))
        return m

    def region_of(self, elem: int, n_outer: int) -> str:
        """Name of the region a stray word at element `elem` lies in, for a call that was asked for n_outer steps."""
        L = self.layout
        o, rem = divmod(elem, L.outer_stride)
        if o >= n_outer:
            return "row beyond n_steps"
        r, col = divmod(rem, L.pitch)
        if r >= L.n_rows:
            return "stride gap"
        if col >= L.n_cols:
            return "pad column"
        return "frozen lane"


@dataclass
class Finding:
    buffer: str
    region: str
    words: int
    first: int           # element offset inside the buffer (inside the arena for a red zone)

    def __str__(self):
        return f"{self.buffer}: {self.words} word(s), {self.region} (first at element {self.first})"


class Arena:
    def __init__(self, device, redzone_bytes: int = REDZONE_BYTES):
        assert redzone_bytes >= REDZONE_BYTES
        self.device, self.redzone_bytes = torch.device(device), redzone_bytes
        self.bufs: Dict[str, Buf] = {}
        self.tensors: Dict[str, torch.Tensor] = {}
        self._raw = {}
        self._frozen: Dict[str, torch.Tensor] = {}

    def add(self, name, kind, layout: Layout, align="elem", role="out", extra_outer: int = 1) -> Buf:
        """Register a buffer.  Its size is the layout's full documented size plus `extra_outer` further steps (so that
        'row n_steps' is memory the buffer owns).  align: "elem" = only element-aligned (origin + 1 element), 16 = 16 bytes
        and only 16 (origin + 16 bytes), 256 = a 256-byte boundary."""
        assert name not in self.bufs and kind in KINDS and align in ("elem", 16, 256) and role in ("in", "out") and not self.tensors
        size = max(layout.min_size() + extra_outer * layout.outer_stride, (layout.n_outer + extra_outer) * layout.outer_stride)
        b = Buf(self, name, kind, size, layout, align, role)
        self.bufs[name] = b
        return b

    def add_and_build(self, *args, **kw):
        self.add(*args, **kw)
        return self.build()

    def build(self):
        for kind, (_, idt, canary) in KINDS.items():
            bufs = [b for b in self.bufs.values() if b.kind == kind]
            if not bufs:
                continue
            isz = torch.empty(0, dtype=idt).element_size()
            red, per256 = -(-self.redzone_bytes // isz), 256 // isz
            pos, offs = 0, []
            for b in bufs:
                pos = -(-(pos + red) // per256) * per256                    # red zone, then the next 256-byte boundary
                pos += {"elem": 1, 16: 16 // isz, 256: 0}[b.align]
                offs.append(pos)
                pos += b.size
            total = pos + red
            raw = torch.full((total + per256,), canary, dtype=idt, device=self.device)
            shift = (-raw.data_ptr() % 256) // isz                           # make element 0 a 256-byte boundary
            self._raw[kind] = raw
            self.tensors[kind] = raw[shift:shift + total]
            for b, o in zip(bufs, offs):
                b.off = o
                want = {"elem": isz % 256, 16: 16, 256: 0}[b.align]
                assert b.ptr % 256 == want, (b.name, b.ptr % 256, want)
        return self

    def __getitem__(self, name) -> Buf:
        return self.bufs[name]

    def freeze_inputs(self):
        """Take the copy every input buffer is compared with; call after the inputs are filled."""
        self._frozen = {b.name: b.ints.clone() for b in self.bufs.values() if b.role == "in"}

    def refill(self, *names):
        """Back to canary (between the launches of one case, after the words were read)."""
        for n in names:
            b = self.bufs[n]
            b.ints.fill_(KINDS[b.kind][2])

    def check(self, written: Dict[str, Optional[dict]]) -> List[Finding]:
        """written[name] = None (nothing may be written) or dict(n_outer=steps asked for, live=optional bool
        [n_outer, lanes], mask=optional explicit bool mask over the buffer's elements in place of the layout's, complete=False
        where not every word of the set need change) for every OUTPUT buffer; inputs are compared with their frozen copies.
        Returns every finding."""
        out: List[Finding] = []
        for kind, t in self.tensors.items():
            canary = KINDS[kind][2]
            bufs = sorted((b for b in self.bufs.values() if b.kind == kind), key=lambda b: b.off)
            outside = torch.ones(t.numel(), dtype=torch.bool, device=t.device)
            for b in bufs:
                outside[b.off:b.off + b.size] = False
            bad = torch.nonzero((t != canary) & outside).flatten()
            if bad.numel():                                                   # red zones: name the nearest buffer
                edges = [(b.off, f"before {b.name}") for b in bufs] + [(b.off + b.size - 1, f"after {b.name}") for b in bufs]
                groups: Dict[str, List[int]] = {}
                for e in bad.tolist()[:4096]:
                    label = min(edges, key=lambda x: abs(x[0] - e))[1]
                    groups.setdefault(label, []).append(e)
                for label, es in groups.items():
                    side, name = label.split(" ", 1)
                    out.append(Finding(name, f"red zone {side} the buffer", len(es) if bad.numel() <= 4096 else int(bad.numel()), es[0]))
            for b in bufs:
                w = b.ints
                if b.role == "in":
                    assert b.name in self._frozen, f"freeze_inputs() was not called for {b.name}"
                    d = torch.nonzero(w != self._frozen[b.name]).flatten()
                    if d.numel():
                        out.append(Finding(b.name, "input changed", int(d.numel()), int(d[0])))
                    continue
                assert b.name in written, f"no written set given for output buffer {b.name}"
                spec = written[b.name]
                n_outer = 0 if spec is None else spec["n_outer"]
                if spec is None:
                    W = torch.zeros(b.size, dtype=torch.bool, device=w.device)
                else:
                    W = spec["mask"] if spec.get("mask") is not None else b.geometry_mask(n_outer, spec.get("live"))
                changed = w != canary
                stray = torch.nonzero(changed & ~W).flatten()
                if stray.numel():
                    regions: Dict[str, List[int]] = {}
                    for e in stray.tolist()[:4096]:
                        regions.setdefault(b.region_of(e, n_outer), []).append(e)
                    for r, es in regions.items():
                        out.append(Finding(b.name, r, len(es), es[0]))
                missing = torch.nonzero(~changed & W).flatten()
                if missing.numel() and (spec is None or spec.get("complete", True)):
                    out.append(Finding(b.name, "unwritten", int(missing.numel()), int(missing[0])))
        return out
