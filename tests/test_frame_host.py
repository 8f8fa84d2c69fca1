"""The host side of the frame renderer (permuto_sdf_amd/render.py, csrc/frame_plan.h, csrc/frame_rays.hip,
csrc/frame_composite.hip), checked without a GPU.

  * tests/host/frame_plan_check.cpp, a stand-alone program that includes nothing but csrc/frame_plan.h, reproduces hand-derived
    chunkings under the address and undefined-behaviour sanitizers;
  * tests/host/frame_rays_check.cpp runs the ray kernel's own source on the CPU (tests/host/hip_on_host) under the same
    sanitizers, against a float64 transcription of the reference's create_rays_from_frame with bars derived from the operands;
  * the library's host-only plan entry agrees with the header; the header lists the new entries and the library exports them;
    empty batches and bad arguments return their codes with no GPU;
  * the module refuses CPU tensors."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "permuto_sdf_amd", "csrc")
POOL = 2097152          # the reference's sample pool (src/OccupancyGrid.cu:216)


def _cxx():
    return next((c for c in ("/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++", shutil.which("clang++"),
                             shutil.which("g++")) if c and os.path.exists(c)), None)


def _build_and_run(tmp_path, name, extra):
    """exactly as tests/test_image_eval_host.py builds its programs"""
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


def test_plan_arithmetic_stand_alone_under_sanitizers(tmp_path):
    _build_and_run(tmp_path, "frame_plan_check", ["-std=c++17", "-Wall", "-Wextra", "-Werror"])


def test_ray_kernel_source_on_the_cpu_under_sanitizers(tmp_path):
    """csrc/frame_rays.hip itself, compiled as C++ against tests/host/hip_on_host, over the 41 x 53 frame: the whole frame,
    pixels [50, 120), the last pixel alone and empty ranges, canaries around the outputs, every entry within its derived bar of
    float64 (tests/host/frame_rays_check.cpp states the derivation)"""
    out = _build_and_run(tmp_path, "frame_rays_check",
                         ["-x", "c++", "-std=c++20", "-ffp-contract=off", "-Wno-unused-function", "-I",
                          os.path.join(ROOT, "tests", "host", "hip_on_host")])
    print(out)
    assert "pixels [0, 2173)" in out and "pixels [50, 120)" in out and "pixels [2172, 2173)" in out and "pixels [0, 0)" in out


def test_frame_plan_h_is_host_only():
    src = open(os.path.join(CSRC, "frame_plan.h")).read()
    assert set(re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", src)) <= {"cmath", "cstdint"}
    assert not re.search(r"\bhip[A-Z_]|__device__|__global__|__host__", src)
    for name in ("frame_rays.hip", "frame_composite.hip"):
        assert '#include "frame_plan.h"' in open(os.path.join(CSRC, name)).read()
    # the ray kernel's file must stay compilable against hip_on_host: no cross-lane operation in it
    rays = open(os.path.join(CSRC, "frame_rays.hip")).read()
    assert not re.search(r"__shfl|__ballot|wave_sum|wave_incl|__builtin_amdgcn", rays)


@pytest.fixture(scope="module")
def lib():
    from permuto_sdf_amd import build
    return ctypes.CDLL(build.build(verbose=False))


def _plan(lib, H, W, cap=64, pool=POOL):
    out = (ctypes.c_int64 * 3)(-9, -9, -9)
    status = lib.psdf_frame_plan(H, W, cap, ctypes.c_int64(pool), out)
    return status, list(out)


def test_library_exports_the_frame_entries_and_its_plan_is_the_headers(lib):
    header = open(os.path.join(ROOT, "include", "psdf.h")).read()
    names = sorted(set(re.findall(r"\b(psdf_frame_[a-z0-9_]+)\s*\(", header)))
    assert names == ["psdf_frame_composite_nerf", "psdf_frame_composite_neus", "psdf_frame_plan", "psdf_frame_rays"]
    assert not [n for n in names if not hasattr(lib, n)]
    assert int(re.search(r"#define PSDF_FRAME_PLAN_FIELDS (\d+)", header).group(1)) == 3
    # every prototype cites the reference lines it replaces
    block = header[header.index("frame_rays.hip, frame_composite.hip"):]
    assert block.count("replaces:") == 4 and "train_permuto_sdf.py:174-176" in block and "nerf_utils.py:459-500" in block
    # the plans frame_plan_check.cpp derives by hand, through the entry Python calls
    assert _plan(lib, 1200, 1600) == (0, [32768, 59, 19456])
    assert _plan(lib, 40, 48) == (0, [1920, 1, 1920])                         # a frame smaller than one chunk
    assert _plan(lib, 41, 53, pool=64 * 256) == (0, [256, 9, 125])            # H W no multiple of 64
    assert _plan(lib, 40, 48, pool=64 * 256) == (0, [256, 8, 128])
    assert _plan(lib, 40, 48, pool=64 * 64) == (0, [64, 30, 64])              # a pool of exactly 64 * cap
    assert _plan(lib, 100, 100, cap=100, pool=99999) == (0, [960, 11, 400])
    # brute force over small cases: the largest multiple of 64 with rays * cap <= pool, at least 64, at most H W
    for H, W, cap, pool in ((7, 9, 3, 200), (30, 30, 5, 1000), (64, 64, 64, 64 * 64 * 3 + 5), (17, 300, 96, 70000)):
        want = min(max(r for r in range(64, pool // cap + 1, 64) if r * cap <= pool), H * W)
        chunks = -(-H * W // want)
        assert _plan(lib, H, W, cap, pool) == (0, [want, chunks, H * W - (chunks - 1) * want]), (H, W, cap, pool)
    # the refusals: out untouched
    for args in ((0, 48), (40, 0), (-3, 48)):
        assert _plan(lib, *args) == (-1, [-9, -9, -9])
    assert _plan(lib, 40, 48, cap=0)[0] == -1 and _plan(lib, 40, 48, cap=-1)[0] == -1
    assert _plan(lib, 40, 48, pool=64 * 64 - 1)[0] == -1 and _plan(lib, 40, 48, pool=0)[0] == -1
    assert _plan(lib, 65536, 32768)[0] == -2 and _plan(lib, 65535, 32768) == (0, [32768, 65535, 32768])
    assert lib.psdf_frame_plan(40, 48, 64, ctypes.c_int64(POOL), None) == -1
    from permuto_sdf_amd import render
    p = render.FramePlan(1200, 1600, 64, POOL)
    assert (p.rays_per_chunk, p.nr_chunks, p.last_chunk) == (32768, 59, 19456)
    assert p.chunks()[0] == (0, 32768) and p.chunks()[-1] == (58 * 32768, 19456) and sum(n for _, n in p.chunks()) == 1920000
    assert render.OccupancyGrid.POOL == POOL
    with pytest.raises(ValueError):
        render.FramePlan(40, 48, 64, 100)


def test_empty_batches_return_before_any_pointer_check_and_bad_arguments_are_refused(lib):
    st, f = None, ctypes.c_float
    z, p = ctypes.c_int64(0), ctypes.c_void_p(4096)          # (never read: every call below returns before a launch)
    assert lib.psdf_frame_rays(0, 0, None, None, z, 0, None, None, st) == 0
    assert lib.psdf_frame_composite_neus(0, None, 0, 0, 0, None, None, None, None, None, None, f(1.0), None, 0, 0, z, None, None,
                                         None, None, None, st) == 0
    assert lib.psdf_frame_composite_nerf(0, None, 0, 0, 0, None, None, None, None, 0, 0, z, None, None, st) == 0

    def rays(H=41, W=53, K=p, T=p, first=0, n=10, o=p, d=p):
        return lib.psdf_frame_rays(H, W, K, T, ctypes.c_int64(first), n, o, d, st)

    assert rays(K=None) == -1 and rays(T=None) == -1 and rays(o=None) == -1 and rays(d=None) == -1
    assert rays(H=0) == -1 and rays(W=-1) == -1 and rays(first=-1) == -1
    assert rays(first=41 * 53 - 9) == -1                     # the last ray lies one pixel past the frame
    assert rays(H=65536, W=32768) == -2

    def neus(R=10, se=p, equal=0, fixed=0, M=100, sdf=p, dirs=p, grads=p, dt=p, rgb=p, inv_s=p, rot=None, H=41, W=53, first=37,
             img=p, nrm=p, cam=None, ws=p, T=p):
        return lib.psdf_frame_composite_neus(R, se, equal, fixed, M, sdf, dirs, grads, dt, rgb, inv_s, f(1.0), rot, H, W,
                                             ctypes.c_int64(first), img, nrm, cam, ws, T, st)

    assert neus(se=None) == -1 and neus(inv_s=None) == -1 and neus(M=-1) == -1
    for k in ("sdf", "dirs", "grads", "dt", "rgb", "img", "nrm", "ws", "T"):
        assert neus(**{k: None}) == -1, k
    assert neus(cam=p, rot=None) == -1                       # camera normals without the rotation
    assert neus(H=0) == -1 and neus(first=-1) == -1 and neus(first=41 * 53 - 9) == -1 and neus(H=65536, W=32768) == -2
    assert neus(equal=1, fixed=-1, se=None) == -1

    def nerf(R=10, se=p, equal=0, fixed=0, M=100, raw=p, dt=p, rgb=p, T=p, H=41, W=53, first=37, img=p, bg=p):
        return lib.psdf_frame_composite_nerf(R, se, equal, fixed, M, raw, dt, rgb, T, H, W, ctypes.c_int64(first), img, bg, st)

    for k in ("se", "raw", "dt", "rgb", "T", "img", "bg"):
        assert nerf(**{k: None}) == -1, k
    assert nerf(W=0) == -1 and nerf(first=41 * 53 - 9) == -1 and nerf(M=-1) == -1 and nerf(H=65536, W=32768) == -2


def test_module_refuses_cpu_tensors_before_it_touches_a_device():
    import permuto_sdf_amd
    from permuto_sdf_amd import render
    from permuto_sdf_amd._lib import PsdfError
    assert permuto_sdf_amd.render is render and "render" in permuto_sdf_amd.__all__
    frame = render.Frame(torch.eye(3), torch.eye(4), 41, 53)
    assert frame.nr_pixels == 2173 and frame.K.dtype == torch.float32
    with pytest.raises(PsdfError):          # a CPU tensor: there is no CPU path
        render.frame_rays(frame)
    with pytest.raises(PsdfError):
        render.frame_rays(frame, 50, 70)
    with pytest.raises(ValueError):
        render.Frame(torch.eye(4), torch.eye(4), 41, 53)
    with pytest.raises(ValueError):
        render.Frame(torch.eye(3), torch.eye(4), 0, 53)

    class Reel:
        rgb_reel = torch.zeros(2, 3, 6, 8)
        K_reel = torch.eye(3).expand(2, 3, 3) * 2
        tf_world_cam_reel = torch.eye(4).expand(2, 4, 4)

    f1 = render.Frame.from_reel(Reel, 1)
    assert (f1.height, f1.width) == (6, 8) and f1.K[0, 0] == 2 and f1.K.is_contiguous()
    # the rotation of tf_cam_world is the transpose of tf_world_cam's
    tf = torch.eye(4)
    tf[:3, :3] = torch.tensor([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    tf[:3, 3] = torch.tensor([1.0, 2.0, 3.0])
    R = render.Frame(torch.eye(3), tf, 4, 4).rot_cam_world()
    assert torch.equal(R, torch.linalg.inv(tf)[:3, :3]) and R.is_contiguous()


def test_the_models_holder_has_every_field_the_trainers_sampling_path_reads():
    """FrameRenderer wraps models that come without a Trainer in a Trainer subclass whose __init__ sets by hand what the sampling
    path reads.  Every `self.<name>` in the source of the methods that path runs must exist on such a holder: a field added to
    the sampling path fails here, not in the middle of a render."""
    import inspect
    import types
    from permuto_sdf_amd import render
    from permuto_sdf_amd.train_step import Trainer
    holder = render.FrameRenderer(types.SimpleNamespace(sdf=torch.nn.Linear(1, 1), rgb=None, bg=None, grid=None, sphere=None,
                                                        hp=None, with_mask=False)).trainer
    assert isinstance(holder, Trainer) and holder.dev == torch.device("cpu") and holder._param_key() is None
    for method in ("_samples", "_samples_begin", "_pinned", "_params_ready"):
        names = set(re.findall(r"\bself\.([A-Za-z_]\w*)", inspect.getsource(getattr(Trainer, method))))
        missing = sorted(n for n in names if not hasattr(holder, n))
        assert not missing, (method, missing)
