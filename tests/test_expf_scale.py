"""det_expf's scaling by 2^k (csrc/nig_detmath.hpp): ldexpf(p, k) -- one v_ldexp_f32 on the device -- against the former
two-multiplication form (p 2^k1) 2^k2, which the oracle's restatement keeps.  CPU only: tests/expf_scale_check.c.

This is the host half of the argument: glibc's ldexpf against the two-step form, on a restatement of the polynomial (whose clamp is
fminf / fmaxf where the device uses v_med3_f32).  That the device's v_ldexp_f32 IS ldexpf -- subnormal results rounded once in the
kernels' denormal mode, a NaN through the clamp -- is the device half: tests/test_gpu_detmath.py compares det_expf on the GPU with the
oracle's two-step restatement bit for bit over the domain."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ldexp_scaling_equals_the_two_step_scaling(tmp_path):
    """Bit for bit: every float of [-103, -87) (2^21 inputs: the only range with subnormal results, i.e. where the scaling
    rounds at all), every 127th float of the rest of [-103, 88.72283] (>= 2^24 inputs), and the overridden ranges."""
    exe = tmp_path / "expf_scale_check"
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-mfma", "-o", str(exe),
                    os.path.join(ROOT, "tests", "expf_scale_check.c"), "-lm"], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "mismatches=0" in out.stdout, out.stdout
    m = re.search(r"\[-103, -87\) (\d+) inputs \((\d+) subnormal results\), rest of the domain (\d+), overridden (\d+)", out.stdout)
    assert m, out.stdout
    low, sub, rest, over = map(int, m.groups())
    assert low == 1 << 21 and sub > 1 << 20          # the whole low range was walked, and it is where the subnormals are
    assert rest >= 1 << 24 and over > 1000
