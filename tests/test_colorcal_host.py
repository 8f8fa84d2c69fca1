"""The host side of the NeRF trainer's colour calibration (permuto_sdf_amd/nerf_train.py, csrc/colorcal.hip), checked without a GPU.

  * the yardstick of the GPU tests, tests/colorcal_float64.py, equals torch autograd in float64 over
    train_step.Colorcal.calib_RGB_samples_packed + sigmoid (the per-sample ray index, a device kernel, restated in torch);
  * its bars admit a plain fp32 torch evaluation of that formula, and they bite: an error of a few bars is seen, and so is a
    calibration applied to the fixed image;
  * csrc/colorcal_plan.h is host-only arithmetic with a sanitized stand-alone check; colorcal.hip itself is compiled against
    tests/host/hip_on_host and its forward and fold run under the address and undefined-behaviour sanitizers;
  * the library exports exactly the three names the header declares; empty inputs and bad arguments return their codes with no
    GPU; the trainer refuses a bad image count before it touches a device."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

from tests import colorcal_float64 as ev
from tests.test_nerf_host import _cxx, _sanitized

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "permuto_sdf_amd", "csrc")
NAMES = ["psdf_colorcal_fold", "psdf_colorcal_sigmoid_backward", "psdf_colorcal_sigmoid_forward"]


def _ray_idx_torch(c):
    """RaySamplesPacked.compute_per_sample_ray_idx in torch: slots no ray owns point at ray 0 (they are kept out of every check)"""
    return lambda ray_start_end_idx, nr_samples: c["ray_of"].clamp_min(0).to(torch.int32)


def _chain(c, raw_fm, g_rgb, wd, bias, img_idx, dtype, monkeypatch, idx_fixed=ev.IDX_FIXED):
    """the reference's operator chain in `dtype` with torch autograd -> rgb [M, 3], g_raw_fm [3, M], g_weight_delta, g_bias"""
    from permuto_sdf_amd.bridge import RaySamplesPacked
    from permuto_sdf_amd.train_step import Colorcal
    monkeypatch.setattr(RaySamplesPacked, "compute_per_sample_ray_idx", staticmethod(_ray_idx_torch(c)))
    cc = Colorcal(ev.NR_IMAGES, idx_fixed).to(dtype)
    with torch.no_grad():
        cc.weight_delta.copy_(wd.to(dtype))
        cc.bias.copy_(bias.to(dtype))
    raw = raw_fm.to(dtype).t().contiguous().requires_grad_(True)
    rgb = torch.sigmoid(cc.calib_RGB_samples_packed(raw, img_idx, c["start_end"]))
    owned = (c["ray_of"] >= 0)[:, None].to(dtype)
    (rgb * g_rgb.to(dtype) * owned).sum().backward()
    return rgb.detach() * owned, raw.grad.t().contiguous(), cc.weight_delta.grad, cc.bias.grad


def _inside_tables(c):
    """the torch module cannot index outside its tables: rays of an image outside [0, I) are given the fixed image, which the
    evaluator treats the same way (identity, no gradient)"""
    img = c["img_idx"].clone()
    img[(img < 0) | (img >= ev.NR_IMAGES)] = ev.IDX_FIXED
    return img


@pytest.mark.parametrize("cname", ev.CONTAINERS)
def test_evaluator_is_torch_autograd_in_float64(cname, monkeypatch):
    c = ev.container(cname)
    raw_fm, g_rgb, wd, bias = ev.family(c)
    img = _inside_tables(c)
    rgb, g_raw_fm, g_wd, g_b = _chain(c, raw_fm, g_rgb, wd, bias, img, torch.float64, monkeypatch)
    for idx in (img, c["img_idx"]):               # ... and an image outside the tables IS the identity
        val, _ = ev.forward(c, raw_fm, idx, wd, bias)
        assert float((val - rgb).abs().max()) <= 1e-14
        back = ev.backward(c, g_rgb, rgb, raw_fm, idx, wd, bias)
        assert float((back["g_raw_fm"][0] - g_raw_fm).abs().max()) <= 1e-13 * max(1.0, float(g_raw_fm.abs().max()))
        folded = ev.fold(idx, [back["g_ray"]])
        for name, want in (("g_weight_delta", g_wd), ("g_bias", g_b)):
            assert float((folded[name][0] - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), name
        assert not bool(folded["g_weight_delta"][0][ev.IDX_FIXED].any()) and not bool(folded["g_bias"][0][3].any())
        # two branches: the sums of both
        two = ev.fold(idx, [back["g_ray"], back["g_ray"]])
        assert float((two["g_bias"][0] - 2 * g_b).abs().max()) <= 1e-12 * max(1.0, float(g_b.abs().max()))
    # rays that keep the identity, empty rays: zero rows
    g_ray = ev.backward(c, g_rgb, rgb, raw_fm, c["img_idx"], wd, bias)["g_ray"][0]
    keep = (c["img_idx"] == ev.IDX_FIXED) | (c["img_idx"] < 0) | (c["img_idx"] >= ev.NR_IMAGES) | (c["counts"] == 0)
    assert not bool(g_ray[keep].any())


def _outside(pairs):
    return {name for name, got, (val, bar) in pairs if bool(((got.double() - val).abs() > bar).any())}


@pytest.mark.parametrize("cname", ev.CONTAINERS)
def test_bars_admit_a_plain_fp32_torch_evaluation_and_bite(cname, monkeypatch):
    c = ev.container(cname)
    raw_fm, g_rgb, wd, bias = ev.family(c, seed=1)
    img = _inside_tables(c)
    rgb, g_raw_fm, g_wd, g_b = _chain(c, raw_fm, g_rgb, wd, bias, img, torch.float32, monkeypatch)
    fwd = ev.forward(c, raw_fm, c["img_idx"], wd, bias)
    back = ev.backward(c, g_rgb, rgb, raw_fm, c["img_idx"], wd, bias)        # (handed the fp32 rgb, as the kernel is)
    folded = ev.fold(c["img_idx"], [back["g_ray"]])
    pairs = [("rgb", rgb, fwd), ("g_raw_fm", g_raw_fm, back["g_raw_fm"]), ("g_weight_delta", g_wd, folded["g_weight_delta"]),
             ("g_bias", g_b, folded["g_bias"])]
    assert not _outside(pairs), _outside(pairs)
    worst = max(float(((got.double() - val).abs() / bar.clamp_min(1e-300)).max()) for _, got, (val, bar) in pairs)
    print("fp32 torch against the bars, %s: worst error / bar %.3f" % (cname, worst))
    # the bars bite: an error of three bars on one entry is seen, in every output
    for name, got, (val, bar) in pairs:
        at = int(bar.reshape(-1).argmax())
        if float(bar.reshape(-1)[at]) == 0.0:
            continue
        off = val.clone().reshape(-1)
        off[at] += 3 * bar.reshape(-1)[at]
        assert _outside([(name, off.reshape(val.shape), (val, bar))]) == {name}
        assert float((bar / val.abs().clamp_min(1e-30))[bar > 0].median()) < 1e-4, name       # and they are tight: 1e-4 of the entry
    if cname in ("rows", "equal32"):
        # a calibration applied to the fixed image too lands outside, forward and backward
        wrong = _chain(c, raw_fm, g_rgb, wd, bias, img, torch.float32, monkeypatch, idx_fixed=3)
        out = _outside([("rgb", wrong[0], fwd), ("g_raw_fm", wrong[1], back["g_raw_fm"]), ("g_bias", wrong[3], folded["g_bias"])])
        assert out == {"rgb", "g_raw_fm", "g_bias"}, out


# ------------------------------------------------------------------------------------------------------- the native side
def test_plan_header_under_sanitizers(tmp_path):
    """csrc/colorcal_plan.h alone, as plain C++17: tests/host/colorcal_plan_check.cpp, a program with its own main"""
    _sanitized(tmp_path, "colorcal_plan_check.cpp", "c++17", [])


def test_forward_and_fold_source_on_the_cpu_under_sanitizers(tmp_path):
    """csrc/colorcal.hip itself, compiled as C++ against tests/host/hip_on_host: the forward and the fold run on the containers
    of the GPU file in buffers of exactly the declared extents, the backward (a butterfly over lanes) with empty batches and bad
    arguments only; tests/host/colorcal_kernels_check.cpp, a stand-alone program with its own main, under ASan and UBSan"""
    if _cxx() is not None and not _cxx().endswith("clang++"):
        pytest.skip("the stand-in header is written for clang")
    _sanitized(tmp_path, "colorcal_kernels_check.cpp", "c++20", ["-I", os.path.join(ROOT, "tests", "host", "hip_on_host")])


def test_plan_header_is_host_only_and_the_kernels_hold_no_atomics():
    src = open(os.path.join(CSRC, "colorcal_plan.h")).read()
    assert set(re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", src)) <= {"cstdint"}
    assert not re.search(r"\bhip[A-Z_]|__device__|__global__|__host__", src)
    hip = open(os.path.join(CSRC, "colorcal.hip")).read()
    code = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", hip, flags=re.S))
    assert '#include "colorcal_plan.h"' in hip and '#include "composite_device.h"' in hip
    assert "atomic" not in code and "asm" not in code and "hipMalloc" not in code and "Synchronize" not in code
    assert "1.0f / (1.0f + expf(-z))" in code and "RayIndex" in code


@pytest.fixture(scope="module")
def lib():
    from permuto_sdf_amd import build
    return ctypes.CDLL(build.build(verbose=False))


def test_library_exports_exactly_the_declared_colorcal_entries(lib):
    header = open(os.path.join(ROOT, "include", "psdf.h")).read()
    start = header.index("/* ---- colorcal.hip ---- */")
    section = header[start:header.index("/* ---- ", start + 10)]
    assert sorted(set(re.findall(r"\bint (psdf_[a-z0-9_]+)\s*\(", section))) == NAMES
    assert not [n for n in NAMES if not hasattr(lib, n)]
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    if os.path.exists(nm):
        out = subprocess.run([nm, "-D", "--defined-only", lib._name], capture_output=True, text=True).stdout
        assert sorted(set(re.findall(r"\b(psdf_colorcal[a-z0-9_]*)\b", out))) == NAMES
    from permuto_sdf_amd import nerf_train
    assert nerf_train.COLORCAL_COLS == int(re.search(r"COLS = (\d+);", open(os.path.join(CSRC, "colorcal_plan.h")).read()).group(1))


def test_empty_inputs_return_before_any_pointer_check_and_bad_arguments_are_refused(lib):
    i64, st = ctypes.c_int64, None
    p = ctypes.c_void_p(4096)          # never read: every call below returns before a launch
    assert lib.psdf_colorcal_sigmoid_forward(0, None, 0, 0, 0, i64(7), None, None, 0, 0, None, None, None, st) == 0
    assert lib.psdf_colorcal_sigmoid_forward(5, None, 0, 0, 0, i64(0), None, None, 0, 0, None, None, None, st) == 0
    assert lib.psdf_colorcal_sigmoid_backward(0, None, 0, 0, 0, i64(7), None, None, None, None, 0, 0, None, None, None, None, st) == 0
    assert lib.psdf_colorcal_fold(0, None, 0, 0, None, None, None, None, st) == 0

    def fwd(se=p, M=1, raw=p, img=p, I=4, fixed=0, wd=p, b=p, rgb=p, R=1):
        return lib.psdf_colorcal_sigmoid_forward(R, se, 0, 1, 1, i64(M), raw, img, I, fixed, wd, b, rgb, st)

    assert fwd(se=None) == -1 and fwd(raw=None) == -1 and fwd(img=None) == -1 and fwd(wd=None) == -1 and fwd(b=None) == -1
    assert fwd(rgb=None) == -1 and fwd(M=-1) == -1 and fwd(I=0) == -1 and fwd(fixed=-1) == -1 and fwd(fixed=4) == -1
    assert fwd(M=2 ** 31 // 3 + 1) == -2 and fwd(I=2 ** 24 + 1) == -2 and fwd(R=2 ** 31 - 1) == -2

    def bwd(se=p, M=1, g=p, y=p, raw=p, img=p, I=4, fixed=0, wd=p, b=p, g_raw=p, g_ray=p):
        return lib.psdf_colorcal_sigmoid_backward(1, se, 0, 1, 1, i64(M), g, y, raw, img, I, fixed, wd, b, g_raw, g_ray, st)

    assert bwd(se=None) == -1 and bwd(g=None) == -1 and bwd(y=None) == -1 and bwd(raw=None) == -1 and bwd(img=None) == -1
    assert bwd(wd=None) == -1 and bwd(b=None) == -1 and bwd(g_raw=None) == -1 and bwd(g_ray=None) == -1
    assert bwd(M=-1) == -1 and bwd(I=0) == -1 and bwd(fixed=4) == -1 and bwd(M=2 ** 31 // 3 + 1) == -2 and bwd(I=2 ** 24 + 1) == -2

    def fold(img=p, I=4, fixed=0, a=p, b=p, g_wd=p, g_b=p):
        return lib.psdf_colorcal_fold(1, img, I, fixed, a, b, g_wd, g_b, st)

    assert fold(img=None) == -1 and fold(a=None) == -1 and fold(g_wd=None) == -1 and fold(g_b=None) == -1
    assert fold(I=0) == -1 and fold(fixed=-1) == -1 and fold(fixed=4) == -1 and fold(I=2 ** 24 + 1) == -2


def test_trainer_refuses_a_bad_image_count_before_it_touches_a_device():
    from permuto_sdf_amd import nerf_train as nt
    from permuto_sdf_amd._lib import PsdfError
    for kw in (dict(nr_images=0), dict(nr_images=-3), dict(nr_images=4, idx_with_fixed_calib=4), dict(nr_images=4, idx_with_fixed_calib=-1)):
        with pytest.raises(ValueError):
            nt.NerfTrainer("cuda:0", **kw)
    with pytest.raises(NotImplementedError, match="nr_images="):      # the old keyword names the new one
        nt.NerfTrainer("cuda:0", colorcal=object())
    c = ev.container("one")
    raw_fm, g_rgb, wd, bias = ev.family(c)
    from permuto_sdf_amd.train_step import Colorcal
    with pytest.raises(PsdfError):                # CPU tensors: there is no CPU path
        nt.colorcal_sigmoid_raw(None, raw_fm, c["img_idx"], Colorcal(4, 0))
    with pytest.raises(PsdfError):
        nt.colorcal_fold_raw(c["img_idx"], Colorcal(4, 0), torch.zeros(1, 6))
    # NerfNet.forward has the reference's signature
    import inspect
    assert list(inspect.signature(nt.NerfNet.forward).parameters)[1:] == ["pos", "dirs", "it", "colorcal", "img_indices", "ray_start_end_idx"]
