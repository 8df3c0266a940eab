"""not-gpu: nig_rollout_sampled (the fused rollout that draws its uniform actions in the kernel) as far as a machine
without a device can check it.

  * the export: declared in include/nig.h, listed in _lib.SYMBOLS, present in libnig.so, and refusing a NULL handle;
  * the action mapping: the kernels do not evaluate fill_actions_kernel's float64 expression
    (float)(low + (high - low) * u), u = m * 2^-24, but csrc/nig_step.hpp action_from_word -- restated here in NumPy and
    compared with the float64 form over ALL 2^24 values of m, for every distinct (low, high) pair of the envs' action Boxes;
  * the generated ISA (same flags as tests/test_ring_isa.py): the sampled three-wave ChemicalReactor kernel and the sampled
    wide PowerGrid kernels hold no global load inside their step loops, and use no more scratch than their ring-fed twins."""
import ctypes as C
import os
import re
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "neorl-industrial-gym_amd", "csrc")
NIG_ERR_INVALID = 1                      # include/nig.h


# ------------------------------------------------------------------------------------------------ the export
def test_sampled_entry_point_is_declared_bound_and_exported():
    import neorl_industrial_gym_amd as ni
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nig.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+nig_rollout_sampled\s*\(\s*nig_handle\s*\*", txt), "include/nig.h does not declare nig_rollout_sampled"
    assert "nig_rollout_sampled" in ni._lib.SYMBOLS
    L = ni._lib.lib()
    assert hasattr(L, "nig_rollout_sampled")
    assert len(L.nig_rollout_sampled.argtypes) == 9          # nig_rollout's thirteen without the four ring arguments
    # a NULL handle is refused before anything touches a device (none can exist here), with nig_rollout's code
    assert L.nig_rollout_sampled(None, 4, None, None, 0, None, 0, 0, None) == NIG_ERR_INVALID == L.nig_rollout(None, 4, None, 0, 0, 1, None, None, 0, None, 0, 0, None)
    assert b"nig_rollout" in L.nig_last_error()
    assert L.nig_version().decode().startswith("nig 0.8.0 ") and "nig-philox-v3" in L.nig_version().decode()
    assert ni.__version__ == "0.8.0"
    assert hasattr(ni.batched.BatchedIndustrialEnv, "rollout_sampled")


def test_generated_action_source_is_an_option_and_ring_the_default():
    import inspect
    import neorl_industrial_gym_amd as ni
    sig = inspect.signature(ni.utils.uniform_action_statistics)
    assert sig.parameters["action_source"].default == "ring"
    with pytest.raises(ValueError):
        ni.utils.uniform_action_statistics("ChemicalReactor-v0", 256, 1, action_source="file")


# ------------------------------------------------------------------------------------------------ the action mapping
def action_boxes():
    """every distinct (low, high) of the action Boxes: [-1, 1) for ChemicalReactor, PowerGrid, RobotAssembly and the four spec
    plants (nig_envs.hpp act_low / act_high), the per-dimension Boxes of the two Advanced envs (envs.py _ACTION_BOX, which
    tests/test_advanced_envs.py ties to the kernels)."""
    import neorl_industrial_gym_amd as ni
    boxes = {(-1.0, 1.0)}
    for cls in (ni.envs.AdvancedChemicalReactorEnv, ni.envs.AdvancedPowerGridEnv):
        lo, hi = cls._ACTION_BOX
        boxes |= set(zip(map(float, lo), map(float, hi)))
    return sorted(boxes)


def kernel_action_from_m(m, low, high):
    """csrc/nig_step.hpp action_from_word on the word's top 24 bits, operation by operation in float32.
    [-1, 1): fmaf(mf, 2^-23, -1) -- a fused multiply-add rounds the exact sum once; the exact sum is formed in float64 here
    (24-bit integer times a power of two, minus one: exact) and narrowed, which is that one rounding.
    low == 0: the float32 product high * (mf * 2^-24).
    Any other Box keeps fill_actions_kernel's float64 expression (the float32 sum low + (high - low) * u rounds twice: it
    differs from it on 2 306 867 of the 2^24 words for 273.15 .. 473.15 and on 360 446 for 0.95 .. 1.05)."""
    f32 = np.float32
    mf = m.astype(f32)                                                   # exact: m < 2^24
    if low == -1.0 and high == 1.0:
        return (mf.astype(np.float64) * 2.0 ** -23 - 1.0).astype(f32)
    if low == 0.0:
        return f32(high) * (mf * f32(2.0 ** -24))
    return float64_form(m, low, high)


def float64_form(m, low, high):
    """fill_actions_kernel: (float)((double)low + ((double)high - (double)low) * u), low / high the Box's float32 limits"""
    lo, hi = np.float64(np.float32(low)), np.float64(np.float32(high))
    u = m.astype(np.float64) * 2.0 ** -24
    return (lo + (hi - lo) * u).astype(np.float32)


def test_boxes_cover_what_the_issue_names():
    boxes = action_boxes()
    for b in ((-1.0, 1.0), (0.0, 0.01), (0.0, 20.0), (0.0, 100.0), (0.0, 3000.0), (0.0, 1.0), (273.15, 473.15), (0.95, 1.05),
              (10.0, 50.0), (8.0, 40.0), (7.0, 35.0), (9.0, 45.0)):
        assert b in boxes, b


@pytest.mark.parametrize("box", ["all"])
def test_action_mapping_equals_the_float64_form_for_every_word(box):
    m = np.arange(1 << 24, dtype=np.uint32)
    kept_f64 = []
    for low, high in action_boxes():
        want = float64_form(m, low, high)
        got = kernel_action_from_m(m, low, high)
        bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, f"Box [{low}, {high}): {bad.size} of 2^24 words differ, first m = {bad[:4].tolist()}"
        assert want.min() >= np.float32(low) and want.max() <= np.float32(high)
        if not (low == -1.0 and high == 1.0) and low != 0.0:
            kept_f64.append((low, high))
            # the float32 sum rounds twice; where it differs from the definition is counted, not needed: the kernel takes the
            # float64 form for EVERY Box with a non-zero low (a range that is a power of two, 8 .. 40, happens to survive)
            naive = np.float32(low) + (np.float32(high) - np.float32(low)) * (m.astype(np.float32) * np.float32(2.0 ** -24))
            n_naive = int(np.count_nonzero(naive.view(np.uint32) != want.view(np.uint32)))
            print(f"Box [{low}, {high}): float32 low + (high - low) * u differs on {n_naive} of 2^24 words")
            if (low, high) == (273.15, 473.15):
                assert n_naive == 2306867
            if (low, high) == (0.95, 1.05):
                assert n_naive == 360446
    # the Boxes that keep the float64 form: a non-zero low (the Advanced envs' inlet temperature, dispatch and tap ranges)
    assert kept_f64 == [(0.95, 1.05), (7.0, 35.0), (8.0, 40.0), (9.0, 45.0), (10.0, 50.0), (273.15, 473.15)]


def test_source_states_the_forms_the_test_restates():
    """the restatement above is of THIS text: if action_from_word changes, this test must be looked at again"""
    src = open(os.path.join(CSRC, "nig_step.hpp")).read()
    body = src[src.index("float action_from_word("):]
    body = body[:body.index("\n}\n")]
    assert "__builtin_fmaf(mf, 1.0f / 8388608.0f, -1.0f)" in body and "low == -1.0f && high == 1.0f" in body
    assert "high * (mf * (1.0f / 16777216.0f))" in body and "low == 0.0f" in body
    assert "(float)((double)low + ((double)high - (double)low) * u01(word))" in body


# ------------------------------------------------------------------------------------------------ the generated ISA
FLAGS = ["--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fno-slp-vectorize", "-std=c++17", "-w", "-S", "--cuda-device-only"]
# (translation unit, mangled-name fragment) of a sampled kernel and of its ring-fed twin
PAIRS = {
    "cr_split": (("sampled_cr", "split_sampled_kernelINS_15ChemicalReactorELi3ELi4E"),
                 ("env_cr", "split_rollout_kernelINS_15ChemicalReactorELi3ELi4ELb0E")),
    "pg_wide512": (("sampled_pg", "rollout_sampled_wide_kernelINS_9PowerGridELi3ELi512E"),
                   ("env_pg", "rollout_wide_kernelINS_9PowerGridELi3ELi512ELb0E")),
    "pg_wide256": (("sampled_pg", "rollout_sampled_wide_kernelINS_9PowerGridELi3ELi256E"),
                   ("env_pg", "rollout_wide_kernelINS_9PowerGridELi3ELi256ELb0E")),
    "pg_wide512_rows": (("sampled_pg", "rollout_sampled_wide_kernelINS_9PowerGridELi2ELi512E"),
                        ("env_pg", "rollout_wide_kernelINS_9PowerGridELi2ELi512ELb0E")),
}


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    pytest.skip("hipcc not found")


@pytest.fixture(scope="module")
def listings():
    hipcc = _hipcc()
    tmp = tempfile.mkdtemp(prefix="nig_sampled_isa_")
    tus = sorted({tu for pair in PAIRS.values() for tu, _ in pair})

    def one(tu):
        out = os.path.join(tmp, tu + ".s")
        subprocess.check_call([hipcc] + FLAGS + ["-o", out, os.path.join(CSRC, tu + ".hip")])
        return tu, open(out).read().split("\n")
    with ThreadPoolExecutor(max_workers=4) as ex:
        return dict(ex.map(one, tus))


def _kernel(lines, frag):
    """(symbol, body lines) of the one kernel whose mangled name contains frag"""
    start = [i for i, l in enumerate(lines) if l.startswith("_ZN3nig") and frag in l and l.split(";")[0].rstrip().endswith(":")]
    assert len(start) == 1, (frag, [lines[i] for i in start])
    i = j = start[0]
    while not lines[j].startswith(".Lfunc_end"):
        j += 1
    return lines[i].split(":")[0], lines[i + 1:j]


def _scratch(lines, symbol):
    """.private_segment_fixed_size of the kernel's descriptor in the listing's metadata"""
    i = next(k for k, l in enumerate(lines) if l.strip() == f".amdhsa_kernel {symbol}")
    while ".amdhsa_private_segment_fixed_size" not in lines[i]:
        i += 1
    return int(lines[i].split()[-1])


def _loop_instructions(body):
    """the instructions that lie on a cycle of the kernel's control-flow graph, i.e. inside some loop: block b is in a loop iff b
    can reach itself.  Returns [(block label, instruction text)]."""
    blocks, cur = [("entry", [])], None
    for l in body:
        t = l.split(";")[0].strip()
        if not t:
            continue
        m = re.match(r"^(\.LBB\d+_\d+):", t)
        if m:
            blocks.append((m.group(1), []))
        elif l.startswith("\t") and not t.startswith("."):
            blocks[-1][1].append(t)
    index = {name: k for k, (name, _) in enumerate(blocks)}
    succ = [set() for _ in blocks]
    for k, (_, ins) in enumerate(blocks):
        falls = True
        for t in ins:
            op = t.split()[0]
            if op == "s_branch" or op.startswith("s_cbranch"):
                succ[k].add(index[t.split()[-1]])
            if op in ("s_branch", "s_endpgm"):
                falls = False
        if falls and k + 1 < len(blocks):
            succ[k].add(k + 1)
    in_loop = []
    for k in range(len(blocks)):
        seen, todo = set(), list(succ[k])
        while todo:
            b = todo.pop()
            if b in seen:
                continue
            seen.add(b)
            todo.extend(succ[b])
        in_loop.append(k in seen)
    return [(blocks[k][0], t) for k in range(len(blocks)) if in_loop[k] for t in blocks[k][1]]


def _loop_loads(body):
    return [t for _, t in _loop_instructions(body) if re.match(r"^(global|flat|buffer)_load", t)]


@pytest.mark.parametrize("case", sorted(PAIRS))
def test_sampled_kernels_load_nothing_in_their_loops_and_spill_no_more(listings, case):
    (tu_s, frag_s), (tu_r, frag_r) = PAIRS[case]
    sym_s, body_s = _kernel(listings[tu_s], frag_s)
    sym_r, body_r = _kernel(listings[tu_r], frag_r)
    loads_s, loads_r = _loop_loads(body_s), _loop_loads(body_r)
    print(f"{case}: loads inside loops: sampled {len(loads_s)}, ring-fed {len(loads_r)}; "
          f"scratch {_scratch(listings[tu_s], sym_s)} / {_scratch(listings[tu_r], sym_r)} B")
    # the method sees the ring-fed twin's action loads (3 rows for ChemicalReactor's producer, 8 rows or 2 row-major float4 for
    # PowerGrid) ...
    assert len(loads_r) >= 2, "the ring-fed twin's action loads were not found inside its loops: the check is blind"
    # ... and in the sampled kernel no load of any kind is left on a cycle.  (The probit table is staged into LDS by a strided
    # copy loop before the block barrier: that loop exists in both kernels and is the one place a load may sit on a cycle.)
    staging = [t for t in loads_s if "dwordx4" in t]
    others = [t for t in loads_s if "dwordx4" not in t]
    assert others == [], others
    assert len(staging) <= 1, staging
    if staging:
        assert len([t for t in loads_r if "dwordx4" in t]) >= 1
    assert _scratch(listings[tu_s], sym_s) <= _scratch(listings[tu_r], sym_r)
