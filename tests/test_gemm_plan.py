"""Split-K planner of the GEMM host side (csrc/gemm_plan.h), checked without a GPU: the header is
plain host C++, so tests/gemm_plan_check.cpp includes it alone, sweeps the three plans and returns
nonzero when one is malformed, overruns its workspace or the documented bound, or differs at the
bound from the unlimited plan."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multimodal_sequencing_amd", "csrc")

# the plans of mmseq_gemm / mmseq_gemm_wgrad at 256 CUs, derived by hand from the arithmetic the
# planner replaced (M x N x K, workspace): the real wgrad shapes of the flagship step, the unsplit
# case whose bias partials the old workspace query forgot, no workspace, a workspace in the middle
# of the fit loop, and one case of each other plan
EXPECTED = """\
tn256 768x768x16384 bias 256MiB: splitk 16 kchunk 1024 cs_off 9437184
tn256 3072x768x20520 bias 256MiB: splitk 7 kchunk 2944 cs_off 16515072
tn256 768x768x1000 bias 256MiB: splitk 1 kchunk 1000 cs_off 0
tn256 768x768x16384 bias 0: splitk 1 kchunk 16384 cs_off -1
tn256 768x768x16384 bias 8MiB: splitk 3 kchunk 5504 cs_off 1769472
tn128 768x768x4100 256MiB: splitk 4 kchunk 1088 cs_off -1
f32 16x768x768 256MiB: splitk 6 kchunk 128 cs_off -1
"""


def _host_cxx():
    for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    return None


def test_gemm_plan(tmp_path):
    cxx = _host_cxx()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "gemm_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC,
                    os.path.join(ROOT, "tests", "gemm_plan_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:]
    lines = r.stdout.splitlines(keepends=True)
    assert lines[0].startswith("plans checked: 56320, failures: 0"), lines[0]
    assert "".join(lines[1:]) == EXPECTED
