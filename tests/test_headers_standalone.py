"""not-gpu: every header under csrc/ is a header -- it includes what it uses and compiles on its own for the device, with the
build's own flags -- and none is a text fragment that only compiles at the line of another file where it is pasted:
no header includes another after it has opened `namespace nig`, and nig_kernels.hpp is the umbrella, nothing but includes."""
import glob
import os
import re
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "neorl-industrial-gym_amd", "csrc")
HEADERS = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*.hpp")))


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    pytest.skip("hipcc not found")


def test_there_are_headers_to_check():
    assert "nig_kernels.hpp" in HEADERS and len(HEADERS) >= 10


@pytest.mark.parametrize("header", HEADERS)
def test_header_compiles_on_its_own(header):
    from neorl_industrial_gym_amd import _build
    hipcc = _hipcc()
    r = subprocess.run([hipcc] + _build.HIPCC_FLAGS + ["-fsyntax-only", "--cuda-device-only", "-x", "hip", os.path.join(CSRC, header)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_no_header_is_pasted_into_an_open_namespace_and_the_umbrella_only_includes():
    for header in HEADERS:
        lines = open(os.path.join(CSRC, header)).read().split("\n")
        opened = next((i for i, l in enumerate(lines) if l.startswith("namespace nig {")), len(lines))
        late = [l for l in lines[opened:] if re.match(r'\s*#\s*include\s+"[^"]*\.hpp"', l)]
        assert not late, (header, late)
    rest = [l for l in open(os.path.join(CSRC, "nig_kernels.hpp")).read().split("\n")
            if l.strip() and not l.lstrip().startswith("//") and l.strip() != "#pragma once" and not re.match(r"\s*#\s*include\b", l)]
    assert not rest, rest
