"""-m gpu: det_rsqrtf (csrc/nig_detmath.hpp) on the device against the host restatement (tests/mlp_ln_ref.c: IEEE sqrt, then IEEE
division), bit for bit on every positive normal float32, through a probe library of its own (tests/rsqrt_probe.hip, built with the
product's HIPCC_FLAGS).  The restatement's accuracy over the same domain: tests/rsqrt_check.c (test_mlp_ln_host.py)."""
import ctypes as C
import os

import pytest
import torch

import mlp_ln_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 1 << 27
LO, HI = 0x00800000, 0x7F800000          # the positive normal floats


@pytest.fixture(scope="module")
def probe():
    import importlib.util
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    spec = importlib.util.spec_from_file_location("_nig_build", os.path.join(ROOT, "neorl-industrial-gym_amd", "_build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    torch.zeros(1, device="cuda")                       # the HIP runtime initialised by torch first
    return C.CDLL(b.build_rsqrt_probe())


def test_rsqrtf_bit_identical_on_every_positive_normal_float(probe):
    y = torch.empty(CHUNK, dtype=torch.float32, device="cuda")
    checked = 0
    for base in range(LO, HI, CHUNK):
        n = min(CHUNK, HI - base)
        assert probe.probe_rsqrt(C.c_uint32(base), C.c_uint64(n), C.c_void_p(y.data_ptr())) == 0
        bad, first = ref.rsqrt_mismatches(base, y[:n].cpu().numpy())
        assert bad == 0, (hex(base + first), bad)
        checked += n
    assert checked == 254 * 2 ** 23
