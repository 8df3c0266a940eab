"""Build libnig.so (HIP kernels + C ABI) for gfx950 with hipcc, in-tree.

One translation unit per environment (csrc/env_*.hip; its nig_rollout_sampled kernels in csrc/sampled_*.hip) plus the C ABI
(csrc/nig_api.hip), compiled
in parallel and linked into ONE shared library.  Staleness is decided by a content hash of the
sources (mtimes do not survive a snapshot copy to another machine), stored next to the library.
"""
import glob
import hashlib
import os
import shutil
import subprocess
import time
from concurrent.futures import ThreadPoolExecutor

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
OBJ = os.path.join(CSRC, "_obj")
LIB = os.path.join(_HERE, "libnig.so")
STAMP = LIB + ".srchash"

# -ffp-contract=off: NumPy evaluates a*b+c with two roundings; the parity bar is bit-level.
# -fno-slp-vectorize: hipcc packs neighbouring scalar f32 adds/muls into v_pk_* pairs; the moves that
# gather their operands cost more issue slots than the packing saves (fused rollout -3 % with SLP on).
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fno-slp-vectorize", "-fPIC",
               "-std=c++17", "-Wall", "-Wno-unused-function"]


def sources():
    return sorted(glob.glob(os.path.join(CSRC, "*.hip")))


def headers():
    return sorted(glob.glob(os.path.join(CSRC, "*.hpp")) + glob.glob(os.path.join(CSRC, "*.inc"))
                  + [os.path.join(os.path.dirname(_HERE), "include", "nig.h")])


def _digest(paths, extra=""):
    h = hashlib.sha256(extra.encode())
    for p in paths:
        h.update(os.path.basename(p).encode())
        with open(p, "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def source_hash():
    return _digest(sources() + headers(), " ".join(HIPCC_FLAGS))


def find_hipcc():
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    return None


def stale():
    if not os.path.exists(LIB) or not os.path.exists(STAMP):
        return True
    try:
        return open(STAMP).read().strip() != source_hash()
    except OSError:
        return True


def _compile_one(hipcc, src, hdr_hash, verbose):
    """Compile one translation unit unless its object is current; returns the object path."""
    name = os.path.splitext(os.path.basename(src))[0]
    obj = os.path.join(OBJ, name + ".o")
    stamp = obj + ".srchash"
    want = _digest([src], hdr_hash)
    if os.path.exists(obj) and os.path.exists(stamp) and open(stamp).read().strip() == want:
        return obj
    cmd = [hipcc] + HIPCC_FLAGS + ["-c", "-o", obj, src]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    with open(stamp, "w") as f:
        f.write(want)
    return obj


def build(force=False, verbose=False, jobs=None):
    """Compile csrc/*.hip -> libnig.so.  Cross-compiles without a GPU.  The library is written to a
    temporary name and renamed into place, so a concurrent reader never maps a half-written file."""
    if not force and not stale():
        return LIB
    hipcc = find_hipcc()
    if hipcc is None:
        raise RuntimeError("hipcc not found: cannot build libnig.so (no CPU fallback exists)")
    os.makedirs(OBJ, exist_ok=True)
    if force:
        for f in glob.glob(os.path.join(OBJ, "*.srchash")):
            os.remove(f)
    hdr_hash = _digest(headers(), " ".join(HIPCC_FLAGS))
    srcs = sources()
    jobs = jobs or max(1, min(len(srcs), (os.cpu_count() or 2)))
    with ThreadPoolExecutor(max_workers=jobs) as ex:
        objs = list(ex.map(lambda s: _compile_one(hipcc, s, hdr_hash, verbose), srcs))
    tmp = f"{LIB}.tmp.{os.getpid()}"
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", tmp] + objs + ["-ldl"]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    os.replace(tmp, LIB)
    with open(STAMP, "w") as f:
        f.write(source_hash())
    return LIB


# Test-only library variants (loaded through NIG_LIB_PATH, never as libnig.so): name -> (translation units recompiled, flags)
VARIANTS = {
    # bounded ring waits + error reporting (csrc/nig_ring.hpp; tests/test_gpu_ring_limit.py)
    "ringlimit": (["env_cr", "env_pg", "env_ra", "sampled_cr", "sampled_pg", "sampled_ra", "nig_api"], ["-DNIG_RING_SPIN_LIMIT=4000000"]),
}


def variant_path(name):
    return os.path.join(_HERE, f"libnig_{name}.so")


def build_variant(name, verbose=False):
    """libnig_<name>.so = libnig.so's objects with the variant's translation units recompiled with its flags.
    Current when its stamp equals the hash of the sources + flags."""
    tus, flags = VARIANTS[name]
    out = variant_path(name)
    stamp = out + ".srchash"
    want = source_hash() + " " + " ".join(flags)
    if os.path.exists(out) and os.path.exists(stamp) and open(stamp).read().strip() == want:
        return out
    build(verbose=verbose)
    hipcc = find_hipcc()
    if hipcc is None:
        raise RuntimeError("hipcc not found: cannot build a library variant")
    vdir = os.path.join(OBJ, "variant_" + name)
    os.makedirs(vdir, exist_ok=True)

    def one(tu):
        obj = os.path.join(vdir, tu + ".o")
        cmd = [hipcc] + HIPCC_FLAGS + ["-w"] + flags + ["-c", "-o", obj, os.path.join(CSRC, tu + ".hip")]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
        return obj
    with ThreadPoolExecutor(max_workers=max(1, min(len(tus), os.cpu_count() or 2))) as ex:
        vobjs = list(ex.map(one, tus))
    base = [os.path.join(OBJ, os.path.splitext(os.path.basename(s_))[0] + ".o") for s_ in sources()
            if os.path.splitext(os.path.basename(s_))[0] not in tus]
    tmp = f"{out}.tmp.{os.getpid()}"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", tmp] + base + vobjs + ["-ldl"])
    os.replace(tmp, out)
    with open(stamp, "w") as f:
        f.write(want)
    return out


# Test-only device probe of the math library (tests/detmath_probe.hip, tests/test_gpu_detmath.py): a shared library of its
# own, never part of libnig.so, compiled with HIPCC_FLAGS -- the library's bits are a property of these flags.
PROBE_SRC = os.path.join(os.path.dirname(_HERE), "tests", "detmath_probe.hip")
PROBE = os.path.join(_HERE, "libnig_detmath_probe.so")
# det_rsqrtf's probe (tests/rsqrt_probe.hip, tests/test_gpu_rsqrt.py): the same kind of library, in a file of its own
RSQRT_PROBE_SRC = os.path.join(os.path.dirname(_HERE), "tests", "rsqrt_probe.hip")
RSQRT_PROBE = os.path.join(_HERE, "libnig_rsqrt_probe.so")


def build_rsqrt_probe(verbose=False):
    return build_probe(verbose, RSQRT_PROBE_SRC, RSQRT_PROBE)


def build_probe(verbose=False, PROBE_SRC=PROBE_SRC, PROBE=PROBE):
    stamp = PROBE + ".srchash"
    want = _digest([PROBE_SRC] + headers(), " ".join(HIPCC_FLAGS))
    if os.path.exists(PROBE) and os.path.exists(stamp) and open(stamp).read().strip() == want:
        return PROBE
    hipcc = find_hipcc()
    if hipcc is None:
        raise RuntimeError("hipcc not found: cannot build the math-library probe")
    os.makedirs(OBJ, exist_ok=True)
    tmp = f"{PROBE}.tmp.{os.getpid()}"
    cmd = [hipcc] + HIPCC_FLAGS + ["-shared", "-o", tmp, PROBE_SRC]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    os.replace(tmp, PROBE)
    with open(stamp, "w") as f:
        f.write(want)
    return PROBE


def ensure(verbose=False):
    """What importing the package calls.  Never compiles inside a profiled or GPU-initialised
    process: with NIG_NO_AUTOBUILD set, or under a rocprofiler preload, a stale library is an error
    (build first: `python -c 'import __graft_entry__ as g; g.build()'`).  Under torchrun only
    LOCAL_RANK 0 compiles; the other ranks wait for its stamp."""
    if not stale():
        return LIB
    preload = os.environ.get("LD_PRELOAD", "") + os.environ.get("ROCP_TOOL_LIBRARIES", "")
    if os.environ.get("NIG_NO_AUTOBUILD") or "rocprof" in preload:
        raise ImportError(f"{LIB} is missing or stale and auto-build is disabled (NIG_NO_AUTOBUILD / profiler preload): "
                          "run `python -c 'import __graft_entry__ as g; g.build()'` first")
    if find_hipcc() is None:
        if os.path.exists(LIB):
            return LIB                     # no compiler on this machine: use the library that travelled with the tree
        raise ImportError(f"{LIB} is missing and hipcc was not found; this package has no CPU fallback")
    if int(os.environ.get("LOCAL_RANK", "0")) != 0:
        deadline = time.time() + 900
        while stale():
            if time.time() > deadline:
                raise ImportError("timed out waiting for LOCAL_RANK 0 to build libnig.so")
            time.sleep(0.5)
        return LIB
    return build(verbose=verbose)
