"""The host side of sphere-traced frames (permuto_sdf_amd/render.py: render_traced; csrc/frame_trace.hip; csrc/sampling.hip:
trace_select_*), checked without a GPU.

  * tests/host/frame_trace_check.cpp runs the resolve kernel's own source on the CPU (tests/host/hip_on_host) under the address and
    undefined-behaviour sanitizers: the 7 x 13 frame and the chunk [77, 410) of the 40 x 48 frame against a float64 transcription
    with the bars of tests/test_gpu_frame_trace.py, canaries outside the chunk, and the argument refusals;
  * the header lists the two entries, each with the reference lines it replaces, and the library exports them; empty chunks and
    bad arguments return their codes with no GPU;
  * the select kernels share the occupancy lookup of check_occupancy_kernel and wait for no other workgroup;
  * the module's new surface refuses CPU tensors and unknown modes before it touches a device."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "permuto_sdf_amd", "csrc")


def _cxx():
    return next((c for c in ("/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++", shutil.which("clang++"),
                             shutil.which("g++")) if c and os.path.exists(c)), None)


def _build_and_run(tmp_path, name, extra):
    """exactly as tests/test_frame_host.py builds its programs"""
    cxx = _cxx()
    if cxx is None:
        pytest.skip("neither ROCm's clang++ nor g++ is installed")
    exe = str(tmp_path / name)
    cmd = [cxx] + extra + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tests", "host", name + ".cpp"), "-o", exe, "-lpthread"]
    if not cxx.endswith("clang++"):     # clang links the sanitizer runtimes into the program by default, g++ on request
        cmd[1:1] = ["-static-libasan", "-static-libubsan"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, " ".join(cmd) + "\n" + r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
    return r.stdout


def test_resolve_kernel_source_on_the_cpu_under_sanitizers(tmp_path):
    out = _build_and_run(tmp_path, "frame_trace_check",
                         ["-x", "c++", "-std=c++20", "-ffp-contract=off", "-Wno-unused-function", "-I",
                          os.path.join(ROOT, "tests", "host", "hip_on_host")])
    print(out)
    assert "7 x 13, pixels [0, 91)" in out and "40 x 48, pixels [77, 410)" in out and "worst error / bar" in out


def _code(name):
    src = open(os.path.join(CSRC, name)).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))


def test_the_kernels_keep_to_their_files_and_share_what_exists():
    # the resolve kernel's file and the header of the surface pixel stay compilable against hip_on_host: no cross-lane operation,
    # no LDS; the pixel is frame_device.h's, which calls normalize_eps for the normal and for the camera normal
    resolve, shared = _code("frame_trace.hip"), _code("frame_device.h")
    for code in (resolve, shared):
        assert not re.search(r"__shfl|__ballot|wave_sum|wave_incl|__builtin_amdgcn|__shared__|__syncthreads|atomic", code)
        assert "sqrtf" not in code and "fmaxf" not in code
    assert '#include "composite_device.h"' in shared and len(re.findall(r"\bnormalize_eps\s*\(", shared)) == 2
    assert "(q.x * d.x + q.y * d.y) + q.z * d.z" in shared
    assert '#include "frame_device.h"' in resolve and "normalize_eps" not in resolve
    assert len(re.findall(r"\bsurface_hit\s*\(", resolve)) == 1 and len(re.findall(r"\bst_surface\s*\(", resolve)) == 1
    # the select kernels live next to check_occupancy_kernel and use the one Grid: its lookup is defined once in the tree
    sampling = _code("sampling.hip")
    for f in os.listdir(CSRC):
        n = len(re.findall(r"\bint\s+pos_to_idx\s*\(", _code(f)))
        assert n == (2 if f == "sampling.hip" else 0), f            # Grid's and GridFast's
    count = sampling[sampling.index("trace_select_count_kernel("):sampling.index("trace_select_scatter_kernel(")]
    scatter = sampling[sampling.index("trace_select_scatter_kernel("):sampling.index("inline Grid mk_grid")]
    assert "g.pos_to_idx(" in count and "g.in_range(" in count and "__ballot(" in count and "__popcll(" in count
    assert "sqrtf(dot3(q, q)) < radius" in count
    # ray order by ballot ranks and a scan of the workgroup counts: no atomics, no loop that could wait for another workgroup
    for body in (count, scatter):
        assert not re.search(r"atomic|\bwhile\b|volatile|__threadfence", body)
    assert "__popcll(votes & ((1ull << lane) - 1ull))" in scatter
    entry = sampling[sampling.index("int psdf_trace_frame_select("):]
    entry = entry[:entry.index("\n}\n")]
    assert entry.count("hipLaunchKernelGGL(") == 3 and "scan_i32_kernel" in entry
    assert not re.search(r"hipMalloc|hipFree|Synchronize|hipMemcpy", entry + resolve)


@pytest.fixture(scope="module")
def lib():
    from permuto_sdf_amd import build
    return ctypes.CDLL(build.build(verbose=False))


def test_library_exports_the_trace_frame_entries_and_the_header_cites_the_reference(lib):
    header = open(os.path.join(ROOT, "include", "psdf.h")).read()
    names = sorted(set(re.findall(r"\b(psdf_trace_frame_[a-z0-9_]+)\s*\(", header)))
    assert names == ["psdf_trace_frame_resolve", "psdf_trace_frame_select"]
    assert not [n for n in names if not hasattr(lib, n)]
    for name in names:      # the comment right above each prototype names the reference lines it replaces
        comment = header[:header.index("int " + name + "(")].rsplit("/*", 1)[1]
        assert "replaces:" in comment and "train_permuto_sdf.py:2" in comment, name
    assert "void* stream);" in header[header.index("int psdf_trace_frame_select("):].split(";")[0] + ";"
    assert "void* stream);" in header[header.index("int psdf_trace_frame_resolve("):].split(";")[0] + ";"


def test_empty_chunks_return_before_any_pointer_check_and_bad_arguments_are_refused(lib):
    st, f = None, ctypes.c_float
    p, t = ctypes.c_void_p(4096), (ctypes.c_float * 3)(0, 0, 0)      # (never read: every call below returns before a launch)
    z = ctypes.c_int64(0)
    assert lib.psdf_trace_frame_select(0, 0, f(0), None, None, f(0), None, None, None, None, None, None, None, None, None, st) == 0
    assert lib.psdf_trace_frame_resolve(0, 0, None, None, None, None, None, None, None, 0, 0, z, None, None, None, None, None, st) == 0

    def select(R=8, n=32, tr=t, occ=p, centre=t, pts=p, dirs=p, no_hit=p, scratch=p, slot=p, pos=p, dirs_out=p, count=p):
        return lib.psdf_trace_frame_select(R, n, f(1.0), tr, occ, f(0.5), centre, pts, dirs, no_hit, scratch, slot, pos, dirs_out,
                                           count, st)

    assert select(R=-1) == -1 and select(n=0) == -1
    for k in ("tr", "occ", "centre", "pts", "dirs", "no_hit", "scratch", "slot", "pos", "dirs_out", "count"):
        assert select(**{k: None}) == -1, k

    def resolve(R=10, M=4, slot=p, o=p, d=p, pos=p, grad=p, rgb=p, rot=None, H=41, W=53, first=37, img=p, nrm=p, cam=None, ws=p,
                depth=p):
        return lib.psdf_trace_frame_resolve(R, M, slot, o, d, pos, grad, rgb, rot, H, W, ctypes.c_int64(first), img, nrm, cam, ws,
                                            depth, st)

    assert resolve(R=-1) == -1 and resolve(M=-1) == -1 and resolve(M=11) == -1
    for k in ("slot", "o", "d", "pos", "grad", "rgb", "img", "nrm", "ws", "depth"):
        assert resolve(**{k: None}) == -1, k
    assert resolve(cam=p, rot=None) == -1                     # camera normals without the rotation
    assert resolve(H=0) == -1 and resolve(W=-1) == -1 and resolve(first=-1) == -1
    assert resolve(first=41 * 53 - 9) == -1                   # the last ray lies one pixel past the frame
    assert resolve(H=65536, W=32768) == -2


def test_module_refuses_cpu_tensors_and_unknown_modes_before_it_touches_a_device():
    import dataclasses
    import inspect
    import types
    from permuto_sdf_amd import render
    from permuto_sdf_amd._lib import PsdfError
    assert [f.name for f in dataclasses.fields(render.TracedFrame)] == ["rgb", "normals", "normals_cam", "weights_sum", "depth"]
    sig = inspect.signature(render.FrameRenderer.render_traced)
    assert {k: v.default for k, v in sig.parameters.items() if k not in ("self", "frame")} == dict(
        it=None, nr_sphere_traces=15, sdf_multiplier=0.9, sdf_converged_tresh=2e-4, camera_normals=False,
        max_rays_per_chunk=render.OccupancyGrid.POOL)
    # one plan for both renderers: a traced frame is the existing plan with one sample per ray
    p = render.FramePlan(1080, 1920, 1, render.OccupancyGrid.POOL)
    assert (p.rays_per_chunk, p.nr_chunks, p.last_chunk) == (1080 * 1920, 1, 1080 * 1920)
    p = render.FramePlan(40, 48, 1, 256)
    assert p.chunks() == [(256 * i, 256) for i in range(7)] + [(1792, 128)]
    assert render.FramePlan(7, 13, 1, 100).chunks() == [(0, 64), (64, 27)]
    holder = types.SimpleNamespace(sdf=torch.nn.Linear(1, 1), rgb=None, bg=None, grid=None, sphere=None, hp=None, with_mask=False)
    rnd = render.FrameRenderer(holder)
    frame = render.Frame(torch.eye(3), torch.eye(4), 41, 53)
    with pytest.raises(PsdfError):          # a CPU frame: there is no CPU path
        rnd.render_traced(frame)
    with pytest.raises(ValueError):
        rnd.render_views([frame], mode="sphere")
    with pytest.raises(PsdfError):
        rnd.render_views([frame], mode="traced")
    z = torch.zeros(4, 3)
    with pytest.raises(PsdfError):
        render.trace_frame_resolve_raw(torch.zeros(4, dtype=torch.int32), 0, z, z, None, None, None, 2, 2, 0, z, z, z, z)
