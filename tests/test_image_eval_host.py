"""The host side of the image evaluation (permuto_sdf_amd/image_eval.py, csrc/image_eval.hip), checked without a GPU.

  * the yardstick of the GPU tests, tests/image_eval_reference.py, equals a float64 transcription of piq's published SSIM (the
    library the reference scores its views with; it is not installed here) up to the float32 rounding of piq's window, and gives
    the hand cases their closed forms;
  * the pooling factor of the plan header, of the library and of the yardstick are Python's own round(min_side / 256);
  * tests/host/image_eval_plan_check.cpp, a stand-alone program that includes nothing but csrc/image_eval_plan.h, reproduces
    hand-derived plans under the address and undefined-behaviour sanitizers;
  * tests/host/image_eval_kernels_check.cpp runs the kernels' own source on CPU threads (tests/host/hip_on_host) under the same
    sanitizers, against brute-force float64;
  * the library's host-only plan entry agrees with the header; empty batches and bad arguments return their codes with no GPU;
  * the yardstick tells the defaults from four wrong variants by more than the bar of the GPU tests."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import image_eval_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "permuto_sdf_amd", "csrc")
BAR = 1e-9          # the bar of tests/test_gpu_image_eval.py on every map entry and score

FACTORS = {383: 1, 384: 2, 385: 2, 639: 2, 640: 2, 641: 3, 895: 3, 896: 4, 897: 4, 1200: 5}


def piq_ssim_float64(x, y, data_range=1.0, kernel_size=11, kernel_sigma=1.5, k1=0.01, k2=0.03):
    """piq.ssim (piq/ssim.py: ssim, _ssim_per_channel; piq/functional/filters.py: gaussian_filter) for (N, C, H, W) inputs with
    reduction 'none', transcribed for float64 images: the window is built in float32, as piq builds it, and then cast to the
    images' dtype, as piq casts it -> (score [N], map [N, C, h', w'])"""
    x, y = torch.as_tensor(x, dtype=torch.float64) / data_range, torch.as_tensor(y, dtype=torch.float64) / data_range
    f = max(1, round(min(x.size()[-2:]) / 256))
    if f > 1:
        x, y = F.avg_pool2d(x, kernel_size=f), F.avg_pool2d(y, kernel_size=f)
    coords = torch.arange(kernel_size, dtype=torch.float32)
    coords -= (kernel_size - 1) / 2.0
    g = coords ** 2
    g = (-(g.unsqueeze(0) + g.unsqueeze(1)) / (2 * kernel_sigma ** 2)).exp()
    g /= g.sum()
    assert g.dtype == torch.float32
    C = x.size(1)
    kernel = g.unsqueeze(0).repeat(C, 1, 1, 1).to(x)
    c1, c2 = k1 ** 2, k2 ** 2
    mu_x, mu_y = F.conv2d(x, weight=kernel, stride=1, padding=0, groups=C), F.conv2d(y, weight=kernel, stride=1, padding=0, groups=C)
    mu_xx, mu_yy, mu_xy = mu_x ** 2, mu_y ** 2, mu_x * mu_y
    sigma_xx = F.conv2d(x ** 2, weight=kernel, stride=1, padding=0, groups=C) - mu_xx
    sigma_yy = F.conv2d(y ** 2, weight=kernel, stride=1, padding=0, groups=C) - mu_yy
    sigma_xy = F.conv2d(x * y, weight=kernel, stride=1, padding=0, groups=C) - mu_xy
    cs = (2.0 * sigma_xy + c2) / (sigma_xx + sigma_yy + c2)
    ss = (2.0 * mu_xy + c1) / (mu_xx + mu_yy + c1) * cs
    return ss.mean(dim=(-1, -2)).mean(1).numpy(), ss.numpy()


@pytest.fixture(scope="module")
def pair_384():
    return ref.scene(1, 1, 384, 390, seed=1)


@pytest.mark.parametrize("shape", [(2, 3, 48, 56), (1, 3, 11, 11), (1, 1, 384, 390), (1, 3, 641, 650)])
def test_reference_is_piqs_formula_up_to_the_float32_rounding_of_its_window(shape):
    """The two differ in the window's weights alone: float32 here (2^-24 relative each, four products deep) against float64.
    Worst case 3 x 4 x 2^-24 / c2 = 8e-4 per map entry; observed (LABNOTES): 6.1e-7 on a score, 1.4e-5 on a map entry."""
    x, y = ref.scene(*shape, seed=1)
    xf, yf = ref.as_f64(x), ref.as_f64(y)
    score, smap = ref.ssim(x, y)
    p_score, p_map = piq_ssim_float64(xf, yf)
    assert smap.shape == p_map.shape and score.shape == (shape[0],)
    d_score, d_map = np.abs(score - p_score).max(), np.abs(smap - p_map).max()
    print("reference vs piq's formula %s: score %.2e map %.2e" % (shape, d_score, d_map))
    assert d_score <= 1e-5 and d_map <= 1e-4
    # PSNR: piq.psnr is -10 log10(mean((x - y)^2 over C H W) + 1e-8) for data_range 1
    want = -10 * torch.log10(torch.mean((torch.as_tensor(xf) - torch.as_tensor(yf)) ** 2, dim=[1, 2, 3]) + 1e-8).numpy()
    assert np.abs(ref.psnr(x, y) - want).max() <= 1e-11


def test_hand_cases_have_their_closed_forms():
    c1 = 0.01 ** 2
    for a, b in ((0.25, 0.75), (1.0, 0.0), (0.5, 0.5), (0.1, 0.9)):
        x, y = np.full((2, 3, 20, 23), a), np.full((2, 3, 20, 23), b)
        score, smap = ref.ssim(x, y)
        want = (2 * a * b + c1) / (a * a + b * b + c1)
        # constant images: both variances vanish up to the rounding of (sum of weights) against its square, amplified by 1 / c2
        assert np.abs(smap - want).max() <= 1e-12 and np.abs(score - want).max() <= 1e-12
    x, y = ref.scene(2, 3, 30, 40, seed=3)
    score, smap = ref.ssim(x, x)
    assert np.abs(smap - 1.0).max() <= 1e-12 and np.abs(score - 1.0).max() <= 1e-12
    assert np.array_equal(ref.psnr(x, x), np.full(2, -10 * math.log10(1e-8))) and abs(ref.psnr(x, x)[0] - 80.0) <= 1e-12
    zero, one = np.zeros((1, 3, 12, 12)), np.ones((1, 3, 12, 12))
    assert abs(ref.psnr(zero, one)[0] - (-10 * math.log10(1 + 1e-8))) <= 1e-15
    # a mask of zeros hides every difference; data_range = 255 on unnormalised values is the same image
    assert ref.psnr(x, y, mask=np.zeros((2, 1, 30, 40)))[0] == ref.psnr(x, x)[0]
    xf, yf = x.astype(np.float32), y.astype(np.float32)
    assert np.abs(ref.ssim(xf, yf, data_range=255.0)[0] - ref.ssim(x, y)[0]).max() <= 1e-12
    # to_u8: ties to even
    ties = (np.arange(0, 256, dtype=np.float64) + 0.5) / 255
    assert ref.to_u8(np.array([0.0, 1.0, -0.2, 1.3, 0.5 / 255, 1.5 / 255, 2.5 / 255])).tolist() == [0, 255, 0, 255, 0, 2, 2]
    assert set((ref.to_u8(ties).astype(int) % 2).tolist()) <= {0, 1} and ref.to_u8(ties).max() == 255


def _cxx():
    return next((c for c in ("/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++", shutil.which("clang++"),
                             shutil.which("g++")) if c and os.path.exists(c)), None)


def _build_and_run(tmp_path, name, extra):
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
    _build_and_run(tmp_path, "image_eval_plan_check", ["-std=c++17", "-Wall", "-Wextra", "-Werror"])


def test_kernel_source_on_cpu_threads_under_sanitizers(tmp_path):
    """csrc/image_eval.hip itself, compiled as C++ against tests/host/hip_on_host (a stand-in for the HIP runtime header that runs
    a launch on CPU threads), driven like image_eval.py drives it and compared with brute-force float64 by
    tests/host/image_eval_kernels_check.cpp: a stand-alone program with its own main, under ASan and UBSan"""
    out = _build_and_run(tmp_path, "image_eval_kernels_check",
                         ["-x", "c++", "-std=c++20", "-ffp-contract=off", "-Wno-unused-function", "-I",
                          os.path.join(ROOT, "tests", "host", "hip_on_host")])
    print(out)


def test_image_eval_plan_h_is_host_only():
    src = open(os.path.join(CSRC, "image_eval_plan.h")).read()
    assert set(re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", src)) <= {"cmath", "cstdint"}
    assert not re.search(r"\bhip[A-Z_]|__device__|__global__|__host__", src)
    hip = open(os.path.join(CSRC, "image_eval.hip")).read()
    assert '#include "image_eval_plan.h"' in hip
    # the tile extents, the factor and the window did not stay behind as copies; no floating-point atomics
    assert "TILE_H =" not in hip and "/ 256" not in hip and "exp(" not in hip and "atomic" not in hip.replace("floating-point atomics", "")


@pytest.fixture(scope="module")
def lib():
    from permuto_sdf_amd import build
    return ctypes.CDLL(build.build(verbose=False))


def _plan(lib, N, C, H, W, k=11, down=1):
    out = (ctypes.c_int64 * 14)(*([-9] * 14))
    status = lib.psdf_image_eval_plan(ctypes.c_int64(N), C, H, W, k, down, out)
    return status, list(out)


def test_pooling_factor_is_pythons_round_in_the_header_the_library_and_the_reference(lib):
    for side, want in FACTORS.items():
        assert round(side / 256) == want
        assert ref.pooling_factor(side, side + 7) == want and ref.pooling_factor(4000, side) == want
        status, out = _plan(lib, 1, 3, side, side + 7)
        assert status == 0 and out[0] == want, (side, out)
        assert out[1:3] == [side // want, (side + 7) // want]
    for side in range(1, 3000, 7):
        assert _plan(lib, 1, 1, side, 3000, k=1)[1][0] == max(1, round(side / 256)) == ref.pooling_factor(3000, side)
    assert _plan(lib, 1, 3, 1200, 1600, down=0)[1][0] == 1


def test_library_exports_the_image_eval_entries_and_its_plan_is_the_headers(lib):
    header = open(os.path.join(ROOT, "include", "psdf.h")).read()
    names = sorted(set(re.findall(r"\b(psdf_image_[a-z0-9_]+)\s*\(", header)))
    assert names == ["psdf_image_eval_plan", "psdf_image_sq_diff", "psdf_image_sq_diff_partials", "psdf_image_ssim"]
    assert not [n for n in names if not hasattr(lib, n)]
    assert int(re.search(r"#define PSDF_IMAGE_EVAL_PLAN_FIELDS (\d+)", header).group(1)) == 14
    src = open(os.path.join(CSRC, "image_eval_plan.h")).read()
    th, tw = (int(v) for v in re.search(r"TILE_H = (\d+), TILE_W = (\d+);", src).groups())
    kmax = int(re.search(r"MAX_KERNEL = (\d+);", src).group(1))
    # the plans image_eval_plan_check.cpp derives by hand, through the entry Python calls
    status, out = _plan(lib, 4, 3, 1200, 1600)
    assert status == 0 and out == [5, 240, 320, 230, 310, th, tw, 15, 10, 4 * 450 * 8, 938, 4 * 938 * 8, kmax, out[13]]
    assert out[13] == (2 * (th + kmax - 1) * (tw + kmax - 1) + 5 * (th + kmax - 1) * tw + 256 + kmax) * 8 <= 80 * 1024
    assert _plan(lib, 1, 3, 641, 650)[1][:9] == [3, 213, 216, 203, 206, th, tw, 13, 7]
    assert _plan(lib, 0, 3, 64, 64)[0] == 0 and _plan(lib, 0, 3, 64, 64)[1][9] == 0
    lib.psdf_image_sq_diff_partials.restype = ctypes.c_int64
    assert lib.psdf_image_sq_diff_partials(1200, 1600) == 938 and lib.psdf_image_sq_diff_partials(0, 4) == -1
    # the refusals
    assert _plan(lib, 1, 3, 10, 100)[0] == -1 and _plan(lib, 1, 3, 100, 100, k=10)[0] == -1
    assert _plan(lib, 1, 3, 100, 100, k=kmax)[0] == 0 and _plan(lib, 1, 3, 100, 100, k=kmax + 2)[0] == -1
    assert _plan(lib, 2 ** 31, 1, 11, 11)[0] == -2 and _plan(lib, -1, 1, 11, 11)[0] == -1
    assert lib.psdf_image_eval_plan(ctypes.c_int64(1), 1, 11, 11, 11, 1, None) == -1


def test_empty_batches_return_before_any_pointer_check_and_bad_arguments_are_refused(lib):
    z, one, st = ctypes.c_int64(0), ctypes.c_int64(1), None
    d = ctypes.c_double
    assert lib.psdf_image_sq_diff(None, 0, None, None, 0, None, None, 0, None, z, 3, 64, 64, d(1.0), None, None, st) == 0
    assert lib.psdf_image_ssim(None, 0, None, None, 0, None, None, 0, None, z, 3, 64, 64, d(1.0), 11, d(1.5), d(0.01), d(0.03), 1,
                               None, None, None, st) == 0
    # argument errors, before any launch (the pointers are never read)
    p, s = ctypes.c_void_p(4096), (ctypes.c_int64 * 4)(3 * 64 * 64, 64 * 64, 64, 1)

    def ssim(pred=p, gt=p, H=64, W=64, k=11, sigma=1.5, data_range=1.0, ws=p, out=p, strides=s, N=one):
        return lib.psdf_image_ssim(pred, 0, strides, gt, 1, s, None, 0, None, N, 3, H, W, d(data_range), k, d(sigma), d(0.01),
                                   d(0.03), 1, ws, out, None, st)

    assert ssim(H=10) == -1 and ssim(W=10) == -1              # a pooled side shorter than the window
    assert ssim(k=10) == -1 and ssim(k=0) == -1               # an even window
    assert ssim(k=17) == -1                                   # a window above what the tile holds
    assert ssim(pred=None) == -1 and ssim(gt=None) == -1      # a null image
    assert ssim(ws=None) == -1 and ssim(out=None) == -1 and ssim(strides=None) == -1
    assert ssim(sigma=0.0) == -1 and ssim(data_range=0.0) == -1 and ssim(data_range=float("nan")) == -1
    assert ssim(strides=(ctypes.c_int64 * 4)(1, -1, 1, 1)) == -1
    assert ssim(N=ctypes.c_int64(-1)) == -1 and ssim(N=ctypes.c_int64(2 ** 31)) == -2
    # a mask without strides
    assert lib.psdf_image_ssim(p, 0, s, p, 0, s, p, 1, None, one, 3, 64, 64, d(1.0), 11, d(1.5), d(0.01), d(0.03), 1, p, p, None, st) == -1

    def sq(pred=p, gt=p, H=64, data_range=1.0, ws=p, out=p, N=one):
        return lib.psdf_image_sq_diff(pred, 1, s, gt, 0, s, None, 0, None, N, 3, H, 64, d(data_range), ws, out, st)

    assert sq(pred=None) == -1 and sq(gt=None) == -1 and sq(H=0) == -1 and sq(data_range=-1.0) == -1
    assert sq(ws=None) == -1 and sq(out=None) == -1 and sq(N=ctypes.c_int64(-1)) == -1 and sq(N=ctypes.c_int64(2 ** 31)) == -2


def test_module_refuses_what_it_cannot_score_before_it_touches_a_device():
    import permuto_sdf_amd
    from permuto_sdf_amd import image_eval as ie
    assert permuto_sdf_amd.image_eval is ie and "image_eval" in permuto_sdf_amd.__all__
    from permuto_sdf_amd._lib import PsdfError
    x = torch.zeros(1, 3, 16, 16)
    with pytest.raises(PsdfError):          # a CPU tensor: there is no CPU path
        ie.psnr(x, x)
    with pytest.raises(ValueError):
        ie.to_u8(torch.zeros(4, dtype=torch.int32))
    assert ie.to_u8(torch.tensor([0.0, 1.0, -0.2, 1.3, 0.5 / 255, 1.5 / 255, 2.5 / 255], dtype=torch.float64)).tolist() == \
        [0, 255, 0, 255, 0, 2, 2]
    s = ie.SceneScores("ours")
    s.update("dtu_scan24", [30.0, 32.0], torch.tensor([0.9, 0.8], dtype=torch.float64))
    s.update("dtu_scan24", 34.0, 0.7)
    s.update("dtu_scan37", torch.tensor(20.0, dtype=torch.float64), torch.tensor(0.5, dtype=torch.float64))
    assert s.scenes() == ["dtu_scan24", "dtu_scan37"]
    assert s.scene_mean("dtu_scan24") == (32.0, pytest.approx(0.8, abs=1e-15)) and s.scene_mean("dtu_scan37") == (20.0, 0.5)
    assert s.mean() == (26.0, pytest.approx(0.65, abs=1e-15))
    lines = s.table().split("\n")
    assert lines[1].split("ours")[1].split() == ["32.00", "&", "20.00", "&"] and lines[2].split("ours")[1].split() == ["0.800", "&", "0.500", "&"]
    assert lines[3].startswith("psnr_avg") and lines[3].endswith("26.0")
    with pytest.raises(ValueError):
        s.update("dtu_scan24", [1.0, 2.0], [0.5])
    assert math.isnan(ie.SceneScores().mean()[0])


@pytest.mark.parametrize("name, kw, measured", [("sigma 1.0", dict(kernel_sigma=1.0), 1.4e-2), ("k2 = 0.3", dict(k2=0.3), 2.2e-2),
                                                ("no pooling", dict(downsample=False), 1.5e-1),
                                                ("a 9-tap window", dict(kernel_size=9), 4.5e-4)])
def test_wrong_variants_lie_further_from_the_defaults_than_the_bar(pair_384, name, kw, measured):
    x, y = pair_384
    want = ref.ssim(x, y)[0]
    got = ref.ssim(x, y, **kw)[0]
    moved = float(np.abs(got - want).max())
    print("%s moves the score of the 384 x 390 pair by %.2e (bar %.0e)" % (name, moved, BAR))
    assert moved > BAR and moved > 0.2 * measured
