"""Launch plans of the LayerNorm, embedding, column-sum and attention host sides
(csrc/launch_plan.h), checked without a GPU: the header is plain host C++, so
tests/launch_plan_check.cpp includes it alone, sweeps the plans and returns nonzero when a path
uses more than its size query, a workspace layout has a gap or an overlap, a grid does not cover
its rows, or the keep-bit words differ from what the kernels index."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multimodal_sequencing_amd", "csrc")

# Derived by hand from the arithmetic these plans replaced (the launch code before launch_plan.h),
# never read back from the header. LayerNorm backward at the flagship's 55368 x 768 and at 432 x 256;
# attention at P = 2, heads = 12 with dropout (forward writing keep bits; backward d1 = counter hash,
# d2 = keep bits): T = 513, 393 and 144 fold their tail, 120 (< 128) and 145 (17 tail rows) do not,
# and Tq = 171 is the row-subset form; the two embedding layouts at shapes of
# tests/test_embed_edges_gpu.py (the table scatter's bytes are an input: 1001 here).
EXPECTED = """\
ln 55368x768 fast dsum: rpb 112 nb 495 cs 1 pw 3 red_off 1140480 floats 1158912 query 2027520
ln 55368x768 fast dsum din: rpb 112 nb 495 cs 0 pw 2 red_off 760320 floats 772608 query 2027520
ln 55368x768 generic dsum: rpb 128 nb 433 cs 0 pw 2 red_off 665088 floats 675840 query 2027520
ln 432x256 fast dsum: rpb 64 nb 7 cs 1 pw 3 red_off 5376 floats 6144 query 6144
ln 432x256 generic dsum: rpb 128 nb 4 cs 0 pw 2 red_off 2048 floats 2560 query 6144
attn T=513 Tq=513 fwd v1: blocks 120 threads 256 lds 35108 nkt2 10 wide 0
attn T=513 Tq=513 fwd v2: blocks 120 threads 128 lds 35108 nkt2 10 wide 0
attn T=513 Tq=513 bwd d1: dq 120 lds 35072 | plain 120 lds 39424 | tail 0 lds 45568 | tail0 0 nxq 5
attn T=513 Tq=513 bwd d2: dq 120 lds 35072 | plain 72 lds 39424 | tail 24 lds 45568 | tail0 512 nxq 4
attn T=513 keep words 123120
attn T=393 Tq=393 fwd v1: blocks 96 threads 256 lds 34588 nkt2 8 wide 0
attn T=393 Tq=393 fwd v2: blocks 96 threads 128 lds 34588 nkt2 8 wide 0
attn T=393 Tq=393 bwd d1: dq 96 lds 34560 | plain 96 lds 38400 | tail 0 lds 44544 | tail0 0 nxq 4
attn T=393 Tq=393 bwd d2: dq 96 lds 34560 | plain 48 lds 38400 | tail 24 lds 44544 | tail0 384 nxq 3
attn T=393 keep words 75456
attn T=120 Tq=120 fwd v1: blocks 24 threads 256 lds 33288 nkt2 2 wide 0
attn T=120 Tq=120 fwd v2: blocks 24 threads 128 lds 33288 nkt2 2 wide 0
attn T=120 Tq=120 bwd d1: dq 24 lds 33280 | plain 24 lds 35840 | tail 0 lds 41984 | tail0 0 nxq 1
attn T=120 Tq=120 bwd d2: dq 24 lds 33280 | plain 24 lds 35840 | tail 0 lds 41984 | tail0 0 nxq 1
attn T=120 keep words 5760
attn T=144 Tq=144 fwd v1: blocks 48 threads 256 lds 33548 nkt2 4 wide 0
attn T=144 Tq=144 fwd v2: blocks 48 threads 128 lds 33548 nkt2 4 wide 0
attn T=144 Tq=144 bwd d1: dq 48 lds 33536 | plain 48 lds 36352 | tail 0 lds 42496 | tail0 0 nxq 2
attn T=144 Tq=144 bwd d2: dq 48 lds 33536 | plain 0 lds 36352 | tail 24 lds 42496 | tail0 128 nxq 1
attn T=144 keep words 13824
attn T=145 Tq=145 fwd v1: blocks 48 threads 256 lds 33548 nkt2 4 wide 0
attn T=145 Tq=145 fwd v2: blocks 48 threads 128 lds 33548 nkt2 4 wide 0
attn T=145 Tq=145 bwd d1: dq 48 lds 33536 | plain 48 lds 36352 | tail 0 lds 42496 | tail0 0 nxq 2
attn T=145 Tq=145 bwd d2: dq 48 lds 33536 | plain 48 lds 36352 | tail 0 lds 42496 | tail0 0 nxq 2
attn T=145 keep words 13920
attn T=513 Tq=171 fwd v1: blocks 48 threads 256 lds 35108 nkt2 10 wide 0
attn T=513 Tq=171 bwd d1: dq 48 lds 35072 | plain 120 lds 39424 | tail 0 lds 45568 | tail0 0 nxq 5
attn T=513 Tq=171 bwd d2: dq 48 lds 35072 | plain 72 lds 39424 | tail 24 lds 45568 | tail0 512 nxq 4
attn T=513 keep words 123120
embed_ln 1x1x4 scatter 1001 B: nb 1 ln 4 red 12 cs 20 scatter 20 total 271
embed_ln 3x7x100 scatter 1001 B: nb 1 ln 2100 red 2300 cs 2500 scatter 3700 total 3951
embed_ln 2x65x768 scatter 1001 B: nb 3 ln 99840 red 104448 cs 105984 scatter 204288 total 204539
embed_ln 257x2x4 scatter 1001 B: nb 9 ln 2056 red 2128 cs 2136 scatter 2148 total 2399
vit_embed 3x9x512: nb 1 ln 1536 red 2560 sp 3584 s0 7680 cs 8192 total 16384
vit_embed 257x3x320: nb 13 ln 82240 red 90560 sp 91200 s0 91840 cs 92160 total 94080
"""


def _host_cxx():
    for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    return None


def test_launch_plan(tmp_path):
    cxx = _host_cxx()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "launch_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC,
                    os.path.join(ROOT, "tests", "launch_plan_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:]
    lines = r.stdout.splitlines(keepends=True)
    assert lines[0].startswith("plans checked: 24912, failures: 0"), lines[0]
    assert "".join(lines[1:]) == EXPECTED
