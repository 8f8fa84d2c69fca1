"""The host layer of permuto_sdf_amd/csrc/encode.hip, checked without a GPU.

The arithmetic that sizes the encoding's launches -- the plan of the binned lattice-gradient path, one resident round of its
workgroups, the deal of that round over the levels -- lives in ONE header, csrc/encode_plan.h, which needs no HIP:
  * psdf_encode_backward_workspace_bytes (host only) returns, at every point of a grid of shapes, what the library returned
    before the header existed (tests/golden/encode_queue_plan.json, recorded from that library);
  * tests/host/encode_plan_check.cpp, a stand-alone program that includes nothing but the header, reproduces hand-derived deals,
    size classes and plans under the address and undefined-behaviour sanitizers;
  * the sources keep the shape the refactor gave them: one (P, F) ladder, no launch macros, no getenv outside the header."""
import ctypes
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "permuto_sdf_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "encode_queue_plan.json")
# compile-time tuning constants and the scan step: the only macros encode.hip keeps
TUNING = {"PSDF_ENC_QSPT", "PSDF_ENC_QWAVES", "PSDF_ENC_REDUCE_U", "PSDF_SCAN_STEP"}


def test_queue_plan_is_the_recorded_one_at_every_grid_point():
    switches = [k for k in os.environ if k.startswith("PSDF_ENC_QUEUE_")]
    assert not switches, "the fixture was recorded with the default switches; unset %s" % switches
    from permuto_sdf_amd import build
    fn = ctypes.CDLL(build.build(verbose=False)).psdf_encode_backward_workspace_bytes
    fn.restype = ctypes.c_int64
    g = json.load(open(GOLDEN))
    grid = [(P, F, N, L, T) for P, F in g["pf"] for N in g["n"] for L in g["levels"] for T in g["capacity"]]
    assert len(grid) == len(g["bytes"]) == 4 * 8 * 3 * 6
    assert 0 in g["bytes"] and any(g["bytes"])          # refused plans and accepted ones
    got = [int(fn(ctypes.c_int(P), ctypes.c_int(F), ctypes.c_int64(N), ctypes.c_int(L), ctypes.c_int(T))) for P, F, N, L, T in grid]
    wrong = [(point, want, have) for point, want, have in zip(grid, g["bytes"], got) if want != have]
    assert not wrong, "(P, F, N, L, T), recorded, returned: %r ... (%d of %d)" % (wrong[:5], len(wrong), len(grid))


def test_plan_and_deal_arithmetic_stand_alone_under_sanitizers(tmp_path):
    cxx = next((c for c in ("/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++", shutil.which("clang++"),
                            shutil.which("g++")) if c and os.path.exists(c)), None)
    if cxx is None:
        pytest.skip("neither ROCm's clang++ nor g++ is installed")
    exe = str(tmp_path / "encode_plan_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "host", "encode_plan_check.cpp"), "-o", exe]
    if not cxx.endswith("clang++"):     # clang links the sanitizer runtimes into the program by default, g++ on request
        cmd[1:1] = ["-static-libasan", "-static-libubsan"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, " ".join(cmd) + "\n" + r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr


def test_encode_plan_h_is_host_only():
    src = open(os.path.join(CSRC, "encode_plan.h")).read()
    assert set(re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", src)) <= {"cstdint", "cstdlib", "vector"}
    assert not re.search(r"\bhip[A-Z_]|__device__|__global__|__host__", src)
    assert '#include "encode_plan.h"' in open(os.path.join(CSRC, "encode.hip")).read()


def test_one_ladder_no_launch_macros_one_getenv():
    sources = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".h"))}
    # the supported (P, F) pairs are listed once, in dispatch_pf
    assert sum(src.count("pos_dim == 3 && nr_feat == 2") for src in sources.values()) == 1
    enc = sources["encode.hip"]
    assert re.search(r"int dispatch_pf\(int pos_dim, int nr_feat, Fn&& fn\)", enc)
    # no function-like macro but the scan step; no object-like one but the tuning constants
    assert re.findall(r"(?m)^\s*#\s*define\s+(\w+)\(.*\)", enc) == ["PSDF_SCAN_STEP"]
    assert set(re.findall(r"(?m)^\s*#\s*define\s+(\w+)", enc)) <= TUNING
    # the environment is read through env_int / env_long of the header
    assert "getenv" not in enc and "atoi" not in enc
    assert sources["encode_plan.h"].count("getenv(") == 2
    # the arithmetic that moved did not stay behind as a copy
    for moved in ("BAL_MIN_PER_LEVEL", "contrib / np", "bucket += 4"):
        assert [f for f, src in sources.items() if moved in src] == ["encode_plan.h"], moved
