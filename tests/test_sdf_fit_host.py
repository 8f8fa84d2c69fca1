"""The host side of SDF fitting (permuto_sdf_amd/sdf_fit.py, csrc/sdf_fit.hip), checked without a GPU.

  * the yardstick of the GPU tests, tests/sdf_fit_float64.py, equals torch autograd in float64 on the same formula written in
    torch operators -- which pins the clamps of the cosine to the installed torch's F.cosine_similarity;
  * its bars admit a plain fp32 torch evaluation of that formula, and they bite: a wrong weight, a sign arm of 1 at 0 and a
    Gaussian weight that is differentiated each land outside them;
  * in the training-like family at most 1 % of the rows have an undecided sign of |g| - 1;
  * csrc/sdf_fit_plan.h is host-only arithmetic; tests/host/sdf_fit_kernels_check.cpp runs the kernels' own source on CPU
    threads (tests/host/hip_on_host) under the address and undefined-behaviour sanitizers, against brute-force float64;
  * the library exports exactly the psdf_sdf_fit_* names the header declares; empty batches and bad arguments return their codes
    with no GPU; the module refuses what it cannot run before it touches a device."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import pytest
import torch

from oracle.composite_float64 import U, _f32
from tests import sdf_fit_float64 as ev64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "permuto_sdf_amd", "csrc")
SHAPES = [(0, 5), (5, 0), (1, 1), (63, 65), (257, 1000)]
GRID = [(P, ns, no, fam, clamp) for P in (3, 4) for ns, no in SHAPES for fam in ev64.FAMILIES for clamp in ev64.CLAMPS]


def _autograd(s, G, n, n_surf, dtype, clamp, **kw):
    """torch autograd of tests.sdf_fit_float64.torch_formula in `dtype` -> (loss, terms, d loss / d s, d loss / d G)"""
    s, G, n = s.to(dtype).requires_grad_(True), G.to(dtype).requires_grad_(True), n.to(dtype)
    weights = kw.pop("weights", tuple(_f32(w) for w in ev64.REFERENCE_WEIGHTS))
    loss, terms = ev64.torch_formula(s, G, n, n_surf, weights=weights, sharpness=_f32(1e2), eik_clamp=None if clamp is None else _f32(clamp),
                                     scale=_f32(1.0 / 30000.0), **kw)
    gs, gG = torch.autograd.grad(loss, (s, G), allow_unused=True)
    gs = torch.zeros_like(s) if gs is None else gs
    return loss.detach(), terms.detach(), gs, gG


@pytest.mark.parametrize("P, n_surf, n_off, family, clamp", GRID)
def test_evaluator_is_torch_autograd_in_float64(P, n_surf, n_off, family, clamp):
    s, G, n = ev64.cases(P, n_surf, n_off, family, seed=1)
    ev = ev64.evaluate(s, G, n, n_surf, eik_clamp=clamp)
    loss, terms, gs, gG = _autograd(s, G, n, n_surf, torch.float64, clamp)
    assert abs(ev["loss"] - float(loss)) <= 1e-13 * max(1.0, abs(float(loss)))
    assert float((ev["terms"] - terms).abs().max()) <= 1e-13
    # gradients: relative to the largest entry of the row's own scale (|g| = 1e-9 gives entries of 1e8 C_1)
    for got, want in ((ev["grad_sdf"], gs), (ev["grad_gradients"], gG)):
        assert got.shape == want.shape
        assert float(((got - want).abs() / want.abs().clamp_min(1e-6)).max()) <= 1e-11
    if P == 4:
        assert not bool(ev["grad_gradients"][:, 3].any()) and not bool(gG[:, 3].any())


def _fp32_mean_allowance(ev, n_surf, n_off):
    counts = [n_surf + n_off, n_surf, n_surf, n_off]
    return torch.tensor([(math.ceil(math.log2(max(c, 1))) + 2) * U for c in counts], dtype=torch.float64) * ev["terms"].abs()


def _fp32_loss_allowance(ev, allow):
    sw = [_f32(1.0 / 30000.0) * _f32(w) for w in ev64.REFERENCE_WEIGHTS]
    return sum(abs(w) * float(a) for w, a in zip(sw, allow)) + 8 * U * sum(abs(w) * float(t) for w, t in zip(sw, ev["terms"]))


@pytest.mark.parametrize("P, n_surf, n_off, family, clamp", GRID)
def test_bars_admit_a_plain_fp32_torch_evaluation(P, n_surf, n_off, family, clamp):
    s, G, n = ev64.cases(P, n_surf, n_off, family, seed=2)
    ev = ev64.evaluate(s, G, n, n_surf, eik_clamp=clamp)
    loss, terms, gs, gG = _autograd(s, G, n, n_surf, torch.float32, clamp)
    # torch's fp32 .mean() adds in fp32 (pairwise), the kernel in double: the mean of count non-negative fp32 values is within
    # (ceil(log2 count) + 2) u of itself on top of the rows' own bars; the weighted sum of four products, three additions and
    # the scale, all fp32, within 8 u of the sum of its terms' sizes
    allow = _fp32_mean_allowance(ev, n_surf, n_off)
    assert bool(((terms.double() - ev["terms"]).abs() <= ev["terms_bar"] + allow).all()), (terms, ev["terms"], ev["terms_bar"])
    assert abs(float(loss) - ev["loss"]) <= ev["loss_bar"] + _fp32_loss_allowance(ev, allow)
    err = (gs.double() - ev["grad_sdf"]).abs()
    assert bool((err <= ev["grad_sdf_bar"]).all()), float((err / ev["grad_sdf_bar"].clamp_min(1e-300)).max())
    worst, bad = ev64.check_gradients(gG, ev)
    print("fp32 torch against the bars, P %d %d + %d %s clamp %s: worst error / bar %.3f, %d ambiguous rows"
          % (P, n_surf, n_off, family, clamp, worst, int(ev["ambiguous"].sum())))
    assert not bad, bad[:10]


def _outside(ev, loss, terms, gs, gG):
    """which outputs of an evaluation lie outside the evaluator's bars"""
    out = set()
    allow = _fp32_mean_allowance(ev, 63, 65)
    if abs(float(loss) - ev["loss"]) > ev["loss_bar"] + _fp32_loss_allowance(ev, allow):
        out.add("loss")
    if bool(((terms.double() - ev["terms"]).abs() > ev["terms_bar"] + allow).any()):
        out.add("terms")
    if bool(((gs.double() - ev["grad_sdf"]).abs() > ev["grad_sdf_bar"]).any()):
        out.add("grad_sdf")
    if ev64.check_gradients(gG, ev)[1]:
        out.add("grad_gradients")
    return out


@pytest.mark.parametrize("P", [3, 4])
def test_bars_bite(P):
    n_surf, n_off, clamp = 63, 65, 0.05
    s, G, n = ev64.cases(P, n_surf, n_off, "ill", seed=3)
    ev = ev64.evaluate(s, G, n, n_surf, eik_clamp=clamp)
    assert not _outside(ev, *_autograd(s, G, n, n_surf, torch.float32, clamp))
    # a wrong weight: the normal term at 1.01 of its weight moves the loss and the surface rows' gradients, not the terms
    w = [_f32(x) for x in ev64.REFERENCE_WEIGHTS]
    out = _outside(ev, *_autograd(s, G, n, n_surf, torch.float32, clamp, weights=(w[0], _f32(1.01 * w[1]), w[2], w[3])))
    assert {"loss", "grad_gradients"} <= out and "terms" not in out, out
    # the sign arm at 0: |x| written as a select whose derivative at 0 is 1 -- seen at the rows with s = 0 (a row with |g| = 1
    # exactly lies within the error bound of |g| - 1 and may take either arm: the one exclusion of the evaluator)
    out = _outside(ev, *_autograd(s, G, n, n_surf, torch.float32, clamp, abs_fn=lambda x: torch.where(x >= 0, x, -x)))
    assert out == {"grad_sdf"}, out
    # the Gaussian weight differentiated: the eikonal term reaches grad_sdf
    out = _outside(ev, *_autograd(s, G, n, n_surf, torch.float32, clamp, detach_weight=False))
    assert out == {"grad_sdf"}, out


def test_training_like_rows_are_rarely_ambiguous():
    for P in (3, 4):
        for clamp in ev64.CLAMPS:
            s, G, n = ev64.cases(P, 3000, 30000, "training", seed=4)
            amb = ev64.evaluate(s, G, n, 3000, eik_clamp=clamp)["ambiguous"]
            assert float(amb.double().mean()) <= 0.01, float(amb.double().mean())
    s, G, n = ev64.cases(3, 63, 65, "ill", seed=4)
    amb = ev64.evaluate(s, G, n, 63)["ambiguous"]
    assert bool(amb[0]) and bool(amb[1]) and not bool(amb[2])       # |g| = 1 exactly is undecided by construction, g = 0 is not


# ------------------------------------------------------------------------------------------------------- the native side
def _cxx():
    return next((c for c in ("/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++", shutil.which("clang++"),
                             shutil.which("g++")) if c and os.path.exists(c)), None)


def test_kernel_source_on_cpu_threads_under_sanitizers(tmp_path):
    """csrc/sdf_fit.hip itself, compiled as C++ against tests/host/hip_on_host (a stand-in for the HIP runtime header that runs a
    launch on CPU threads), driven like sdf_fit.py drives it and compared with brute-force float64 by
    tests/host/sdf_fit_kernels_check.cpp: a stand-alone program with its own main, under ASan and UBSan"""
    cxx = _cxx()
    if cxx is None:
        pytest.skip("neither ROCm's clang++ nor g++ is installed")
    exe = str(tmp_path / "sdf_fit_kernels_check")
    cmd = [cxx, "-x", "c++", "-std=c++20", "-ffp-contract=off", "-Wno-unused-function", "-I", os.path.join(ROOT, "tests", "host", "hip_on_host"),
           "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
           os.path.join(ROOT, "tests", "host", "sdf_fit_kernels_check.cpp"), "-o", exe, "-lpthread"]
    if not cxx.endswith("clang++"):     # clang links the sanitizer runtimes into the program by default, g++ on request
        cmd[1:1] = ["-static-libasan", "-static-libubsan"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, " ".join(cmd) + "\n" + r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
    print(r.stdout)


def test_sdf_fit_plan_h_is_host_only():
    src = open(os.path.join(CSRC, "sdf_fit_plan.h")).read()
    assert set(re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", src)) <= {"cmath", "cstdint"}
    assert not re.search(r"\bhip[A-Z_]|__device__|__global__|__host__", src)
    hip = open(os.path.join(CSRC, "sdf_fit.hip")).read()
    assert '#include "sdf_fit_plan.h"' in hip
    # the grid cap did not stay behind as a copy; no atomics of any kind, no inline assembly
    assert "MAX_GRID =" not in hip and "512" not in hip
    assert "atomic" not in hip.replace("floating-point atomics", "") and "asm" not in hip


@pytest.fixture(scope="module")
def lib():
    from permuto_sdf_amd import build
    return ctypes.CDLL(build.build(verbose=False))


def test_library_exports_exactly_the_declared_sdf_fit_entries(lib):
    header = open(os.path.join(ROOT, "include", "psdf.h")).read()
    assert "/* ---- sdf_fit.hip ---- */" in header
    names = sorted(set(re.findall(r"\b(psdf_sdf_fit_[a-z0-9_]+)\s*\(", header)))
    assert names == ["psdf_sdf_fit_batch", "psdf_sdf_fit_loss", "psdf_sdf_fit_plan"]
    assert not [n for n in names if not hasattr(lib, n)]
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    if os.path.exists(nm):
        out = subprocess.run([nm, "-D", "--defined-only", lib._name], capture_output=True, text=True).stdout
        assert sorted(set(re.findall(r"\b(psdf_sdf_fit_[a-z0-9_]+)\b", out))) == names
    assert int(re.search(r"#define PSDF_SDF_FIT_PLAN_FIELDS (\d+)", header).group(1)) == 4
    src = open(os.path.join(CSRC, "sdf_fit_plan.h")).read()
    block, cap = int(re.search(r"BLOCK = (\d+);", src).group(1)), int(re.search(r"MAX_GRID = (\d+);", src).group(1))
    from permuto_sdf_amd import sdf_fit
    assert sdf_fit.PLAN_FIELDS == 4
    assert sdf_fit.plan(3000, 30000) == (129, 129 * 4 * 8, block * cap, 129)
    assert sdf_fit.plan(0, 0) == (0, 0, block * cap, 0)
    assert sdf_fit.plan(1, block * cap) == (cap, cap * 4 * 8, block * cap, cap + 1)


def test_empty_batches_return_before_any_pointer_check_and_bad_arguments_are_refused(lib):
    z, one, two, st = ctypes.c_int64(0), ctypes.c_int64(1), ctypes.c_int64(2), None
    f = ctypes.c_float
    p, w = ctypes.c_void_p(4096), (ctypes.c_float * 4)(5e1, 1e2, 3e3, 1e2)
    out = (ctypes.c_int64 * 4)()
    assert lib.psdf_sdf_fit_plan(ctypes.c_int64(-1), z, out) == -1 and lib.psdf_sdf_fit_plan(z, z, None) == -1
    assert lib.psdf_sdf_fit_plan(ctypes.c_int64(2 ** 31), z, out) == -2
    assert lib.psdf_sdf_fit_plan(ctypes.c_int64(2 ** 30), ctypes.c_int64(2 ** 30), out) == -2
    assert lib.psdf_sdf_fit_batch(3, z, z, z, None, None, None, None, None, None, None, None, st) == 0
    assert lib.psdf_sdf_fit_loss(3, z, z, None, None, None, None, f(1e2), f(0), f(1), None, None, None, None, None, st) == 0

    # argument errors, before any launch (the device pointers are never read)
    def batch(P=3, M=two, n_surf=one, n_off=one, cp=p, cn=p, idx=p, u=p, lo=w, hi=w, pts=p, nrm=p):
        return lib.psdf_sdf_fit_batch(P, M, n_surf, n_off, cp, cn, idx, u, lo, hi, pts, nrm, st)

    assert batch(P=2) == -1 and batch(P=5) == -1 and batch(M=z) == -1 and batch(M=ctypes.c_int64(-1)) == -1
    assert batch(cp=None) == -1 and batch(cn=None) == -1 and batch(idx=None) == -1 and batch(u=None) == -1
    assert batch(lo=None) == -1 and batch(hi=None) == -1 and batch(pts=None) == -1 and batch(nrm=None) == -1
    assert batch(n_surf=ctypes.c_int64(-1)) == -1 and batch(n_off=ctypes.c_int64(-1)) == -1
    assert batch(n_surf=ctypes.c_int64(2 ** 31)) == -2 and batch(M=ctypes.c_int64(2 ** 31)) == -2

    def loss(P=3, n_surf=one, n_off=one, sdf=p, g=p, n=p, wts=w, sharp=1e2, clamp=0.0, scale=1.0, ws=p, terms=p, acc=p, gs=p, gg=p):
        return lib.psdf_sdf_fit_loss(P, n_surf, n_off, sdf, g, n, wts, f(sharp), f(clamp), f(scale), ws, terms, acc, gs, gg, st)

    nan = float("nan")
    assert loss(P=2) == -1 and loss(sdf=None) == -1 and loss(g=None) == -1 and loss(n=None) == -1 and loss(wts=None) == -1
    assert loss(ws=None) == -1 and loss(terms=None) == -1
    assert loss(gs=None) == -1 and loss(gg=None) == -1                      # both gradients or none
    assert loss(sharp=nan) == -1 and loss(clamp=nan) == -1 and loss(scale=nan) == -1
    assert loss(wts=(ctypes.c_float * 4)(1, nan, 1, 1)) == -1
    assert loss(n_surf=ctypes.c_int64(-1)) == -1 and loss(n_off=ctypes.c_int64(2 ** 31)) == -2


def test_module_refuses_what_it_cannot_run_before_it_touches_a_device():
    import permuto_sdf_amd
    from permuto_sdf_amd import sdf_fit
    from permuto_sdf_amd._lib import PsdfError
    assert permuto_sdf_amd.sdf_fit is sdf_fit and "sdf_fit" in permuto_sdf_amd.__all__
    s, G, n = ev64.cases(3, 5, 7, "training")
    with pytest.raises(PsdfError):          # CPU tensors: there is no CPU path
        sdf_fit.sdf_fit_loss_raw(s, G, n, 5)
    cloud = sdf_fit.OrientedCloud(torch.zeros(4, 3), torch.ones(4, 3))
    with pytest.raises(PsdfError):
        sdf_fit.sdf_fit_batch_raw(cloud, torch.zeros(2, dtype=torch.int64), torch.zeros(3, 3), [0, 0, 0], [1, 1, 1])
    with pytest.raises(ValueError):
        sdf_fit.OrientedCloud(torch.zeros(4, 2), torch.ones(4, 3))
    with pytest.raises(ValueError):
        sdf_fit.OrientedCloud.stack_in_time([cloud])
    with pytest.raises(ValueError):
        sdf_fit.SdfFitNet(pos_dim=2)
    # the torch form of the loss is tests/sdf_fit_float64.py's formula
    a, ta = sdf_fit.sdf_fit_loss_torch(s.double(), G.double(), n.double(), 5, eik_clamp=0.05)
    b, tb = ev64.torch_formula(s.double(), G.double(), n.double(), 5, eik_clamp=0.05)
    assert float(a) == float(b) and torch.equal(ta, tb)
    # set-up helpers: area-weighted vertex normals of an octahedron point outwards along the axes; clouds stack in time
    V = torch.tensor([[1.0, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]])
    Fc = torch.tensor([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]])
    oc = sdf_fit.OrientedCloud.from_mesh(V, Fc)
    assert float((oc.normals - V).abs().max()) <= 1e-6
    st = sdf_fit.OrientedCloud.stack_in_time([oc, oc, oc])
    assert st.points.shape == (18, 4) and st.points[:, 3].tolist() == [0.0] * 6 + [0.5] * 6 + [1.0] * 6 and st.normals.shape == (18, 3)
