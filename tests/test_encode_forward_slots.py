"""The slot plan of the paired encode forward (csrc/encode_plan.h: forward_slots), checked without a GPU.

tests/host/encode_slots_check.cpp is a stand-alone program that includes nothing but the header and walks every (levels,
pseudo-levels, pairs) it is asked about: every level sits in exactly one slot, a pair takes one member from each end, pairs = 0
is one level per slot in index order, a request beyond L // 2 is clamped.  Built and run under the address and
undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "permuto_sdf_amd", "csrc")


def test_slot_plan_stand_alone_under_sanitizers(tmp_path):
    cxx = next((c for c in ("/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++", shutil.which("clang++"),
                            shutil.which("g++")) if c and os.path.exists(c)), None)
    if cxx is None:
        pytest.skip("neither ROCm's clang++ nor g++ is installed")
    exe = str(tmp_path / "encode_slots_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "host", "encode_slots_check.cpp"), "-o", exe]
    if not cxx.endswith("clang++"):     # clang links the sanitizer runtimes into the program by default, g++ on request
        cmd[1:1] = ["-static-libasan", "-static-libubsan"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, " ".join(cmd) + "\n" + r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr


def test_the_library_declares_and_exports_the_setter():
    import ctypes
    from permuto_sdf_amd import build
    assert "int psdf_encode_set_forward_pairs(int pairs);" in open(os.path.join(ROOT, "include", "psdf.h")).read()
    fn = ctypes.CDLL(build.build(verbose=False)).psdf_encode_set_forward_pairs       # host only: no device needed
    fn.restype = ctypes.c_int
    assert fn(ctypes.c_int(-2)) == -1 and fn(ctypes.c_int(3)) == 0 and fn(ctypes.c_int(0)) == 0 and fn(ctypes.c_int(-1)) == 0
