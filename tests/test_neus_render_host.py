"""The host side of the masked training step's render and loss tail (csrc/neus_render.hip, permuto_sdf_amd/neus.py), checked
without a GPU.

  * the yardstick of the GPU tests, tests/neus_render_float64.py, equals torch autograd in float64 of
    VolumeRenderingNeus.compute_weights + integrate and the two loss lines of train_permuto_sdf.py restated in torch operators,
    for every non-empty subset of the three upstream gradients; its float64 family keeps every 1 - alpha + 1e-7 above 1e-4 (the
    backward's floor is inactive there) and every true_cos off the relu kinks;
  * its bars admit a plain fp32 torch evaluation of that formula, and they bite: a dropped g_weights_sum, a weight sum replaced by
    1 - bg (on the rays where the two differ by more than the bar: see the test), a cross entropy without the clip and a missing
    hit mask each land outside them;
  * csrc/neus_render_plan.h is host-only arithmetic with a sanitized stand-alone check; the loss tail runs as the kernel's own
    source on CPU threads (tests/host/hip_on_host) under the address and undefined-behaviour sanitizers, as a program of its own;
  * the library exports exactly the new names the header declares; empty inputs and bad arguments return their codes with no GPU;
    the wrappers of neus.py refuse mismatched shapes before they touch a device."""
import ctypes
import math
import os
import re
import shutil
import subprocess
from types import SimpleNamespace

import pytest
import torch

from tests import neus_render_float64 as ev64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "permuto_sdf_amd", "csrc")
CONTAINERS = ["borders", "equal1", "equal65", "equal129"]
NAMES = ["psdf_neus_mask_loss", "psdf_neus_render_backward", "psdf_neus_render_forward", "psdf_neus_render_plan"]
OUTPUTS = ("pred", "weights_sum", "bg", "g_sdf", "g_gradients", "g_rgb", "g_inv_s")


def _up(c, subset, seed=0):
    g = ev64.upstream(c, seed)
    return [t if on else None for t, on in zip(g, subset)]


def _autograd(rays, fam, ups, dtype, **kw):
    """torch autograd of the restated render in `dtype` for the upstream gradients `ups` -> the seven OUTPUTS"""
    sdf, dirs, grad, dt, rgb, inv_s = fam
    leaves = [t.to(dtype).requires_grad_(True) for t in (sdf, grad, rgb, inv_s)]
    pred, ws, bg = ev64.render_torch(rays, leaves[0], dirs, leaves[1], dt, leaves[2], leaves[3], dtype=dtype, **kw)
    total = leaves[0].sum() * 0
    for out, g in zip((pred, ws, bg), ups):
        if g is not None:
            total = total + (out * g.to(dtype).reshape(out.shape)).sum()
    gs = [torch.zeros_like(l) if g is None else g for l, g in zip(leaves, torch.autograd.grad(total, leaves, allow_unused=True))]
    return pred.detach(), ws.detach(), bg.detach(), gs[0].reshape(-1), gs[1], gs[2], gs[3].reshape(1)


def _render(rays, fam, ups, **kw):
    sdf, dirs, grad, dt, rgb, inv_s = fam
    return ev64.render(rays, sdf, dirs, grad, dt, rgb, inv_s, g_pred=ups[0], g_ws=ups[1], g_bg=ups[2], **kw)


@pytest.mark.parametrize("cname", CONTAINERS)
def test_render_evaluator_is_torch_autograd_in_float64(cname):
    c = ev64.container(cname)
    rays = ev64.rays_of(c)
    fam = ev64.family(c, "float64")
    assert len(ev64.SUBSETS) == 7
    for subset in ev64.SUBSETS:
        ups = _up(c, subset)
        ev = _render(rays, fam, ups)
        assert ev["min_om"] > 1e-4                      # the floor max(om, 1e-6) of the backward is inactive in this family
        assert not bool(ev["kink"].any())               # and no sample sits on a relu kink of section()
        for name, want in zip(OUTPUTS, _autograd(rays, fam, ups, torch.float64)):
            got = ev[name][0]
            assert got.shape == want.shape, name
            assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), (name, subset)
    # rays the kernels skip: 0, 0, 1, and no sample of theirs is touched
    skipped = ~rays.valid
    if bool(skipped.any()):
        ev = _render(rays, fam, list(ev64.upstream(c)))
        assert not bool(ev["pred"][0][skipped].any()) and not bool(ev["weights_sum"][0][skipped].any())
        assert bool((ev["bg"][0][skipped] == 1).all())
        assert not bool(ev["g_sdf"][0][~rays.touched(c["N"])].any()) and not bool(ev["g_gradients"][0][~rays.touched(c["N"])].any())


def _outside_render(ev, got):
    out = set()
    for name, g in zip(OUTPUTS, got):
        val, bar = ev[name]
        if bool(((g.double() - val).abs() > bar).any()):
            out.add(name)
    return out


@pytest.mark.parametrize("cname", CONTAINERS)
def test_render_bars_admit_a_plain_fp32_torch_evaluation_and_bite(cname):
    c = ev64.container(cname)
    rays = ev64.rays_of(c)
    fam = ev64.family(c, "float64", seed=1)
    worst = 0.0
    for subset in ev64.SUBSETS:
        ups = _up(c, subset, seed=1)
        ev = _render(rays, fam, ups)
        got = _autograd(rays, fam, ups, torch.float32)
        assert not _outside_render(ev, got), (subset, _outside_render(ev, got))
        for name, g in zip(OUTPUTS, got):
            val, bar = ev[name]
            worst = max(worst, float(((g.double() - val).abs() / bar.clamp_min(1e-300)).max()))
        # the bars bite: three quarters of the non-zero gradient entries at least are held to better than 1e-3 of themselves
        # (g_alpha = g_w T - g_om cancels on the rest: there the bar is that of the two parts), none is lost in its bar.  Asserted
        # where g_pred arrives without g_weights_sum: the weight sum's own part telescopes (d sum w / d alpha_i = T_i - sum_{j > i} w_j / om_i, which is the
        # ray's last transmittance up to the 1e-7 terms), so behind many samples its gradient is a difference of two nearly equal
        # numbers and no fp32 evaluation holds it to 1e-3: those shares are printed
        b, sat = ev64.c64.bites(ev["g_sdf"][0], ev["g_sdf"][1])
        if subset[0] and not subset[1]:
            assert b >= 0.75 and sat <= 0.01, (subset, b, sat)
        else:
            print("  %s upstream %s: bites %.2f, saturated %.2f" % (cname, subset, b, sat))
    print("fp32 torch against the bars, %s: worst error / bar %.3f" % (cname, worst))
    # a backward that drops g_weights_sum lands outside, in everything behind g_alpha (g_rgb does not depend on it)
    ups = _up(c, (True, True, True), seed=1)
    ev = _render(rays, fam, ups)
    out = _outside_render(ev, _autograd(rays, fam, ups, torch.float32, drop_ws=True))
    # (g_inv_s is one total over all samples under the bar of a sum of that many terms: it may or may not show there)
    assert {"g_sdf", "g_gradients"} <= out and not out & {"pred", "weights_sum", "bg", "g_rgb"}, out
    # and the reference's channel quirk is seen when it is not asked for
    quirk = _render(rays, fam, ups, compat=True)
    assert bool(((quirk["g_sdf"][0] - ev["g_sdf"][0]).abs() > ev["g_sdf"][1]).any())
    # a weight sum replaced by 1 - bg.  The two differ by the LAST sample's weight (sum_i a_i T_i telescopes to 1 - T_n with the
    # last factor in it, bg is T_{n-1}) and by 1e-7 sum T_i: the bars tell them apart on a ray if, and only if, that difference
    # exceeds the entry's bar plus what fp32 loses forming 1 - bg (u, and the bar of bg).  Behind a few dozen samples of this
    # family the last weight can lie below the bar of a sum of that many terms: there the replacement is invisible to any fp32
    # test, and the test prints the ray lengths at which that happens.
    pred, ws_bg, bg = [t.detach() for t in ev64.render_torch(rays, *fam, dtype=torch.float32, ws_from_bg=True)]
    val, bar = ev["weights_sum"]
    told = (ws_bg.double() - val).abs() > bar
    must = ((1 - ev["bg"][0]) - val).abs() > bar + ev["bg"][1] + 2 * ev64.U
    cannot = rays.valid & ~((1 - ev["bg"][0] - val).abs() > bar)
    assert bool((told | ~must).all()) and not bool((told & ~rays.valid).any())
    assert bool(must[rays.cnt == 1].all())          # a ray of one sample: weights_sum = alpha against 1 - bg = 0, always told apart
    assert bool(told.any()) == bool(must.any())
    print("weights_sum against 1 - bg, %s: told apart on %d of %d rays; indistinguishable within the bar at ray lengths %s"
          % (cname, int(told.sum()), int(rays.valid.sum()), sorted(set(rays.cnt[cannot].tolist()))))


def _loss_fp32(pred, gt, hit, ws, gm, **kw):
    p, w = pred.clone().requires_grad_(True), ws.clone().requires_grad_(True)
    loss, terms = ev64.mask_loss_torch(p, gt, hit, w, gm, **kw)
    gp, gw = torch.autograd.grad(loss, (p, w))
    return loss.detach(), terms, gp, gw


def _outside_loss(ev, loss, terms, gp, gw, R):
    # torch's fp32 .mean() adds in fp32 (pairwise), the kernel in double: (ceil(log2 count) + 2) u of the mean on top
    allow = torch.tensor([(math.ceil(math.log2(3 * R)) + 2) * ev64.U, (math.ceil(math.log2(max(R, 2))) + 2) * ev64.U],
                         dtype=torch.float64) * ev["terms"][0].abs()
    out = set()
    if bool(((terms.double() - ev["terms"][0]).abs() > ev["terms"][1] + allow).any()):
        out.add("terms")
    if abs(float(loss) - float(ev["loss"][0])) > float(ev["loss"][1]) + float(allow[0]) + 0.1 * float(allow[1]):
        out.add("loss")
    if bool(((gp.double() - ev["g_pred"][0]).abs() > ev["g_pred"][1]).any()):
        out.add("g_pred")
    if bool(((gw.double() - ev["g_ws"][0]).abs() > ev["g_ws"][1]).any()):
        out.add("g_ws")
    return out


@pytest.mark.parametrize("R", [1, 63, 257])
@pytest.mark.parametrize("hit_mode", [None, "zero", "mixed"])
def test_loss_evaluator_is_torch_autograd_in_float64(R, hit_mode):
    pred, gt, hit, ws, gm = ev64.mask_loss_cases(R, hit_mode)
    ev = ev64.mask_loss(pred, gt, hit, ws, gm)
    p, w = pred.double().requires_grad_(True), ws.double().requires_grad_(True)
    loss, terms = ev64.mask_loss_torch(p, gt.double(), hit, w, gm.double())
    gp, gw = torch.autograd.grad(loss, (p, w))
    assert abs(float(ev["loss"][0]) - float(loss.detach())) <= 1e-13 * max(1.0, abs(float(loss.detach())))
    assert float((ev["terms"][0] - terms).abs().max()) <= 1e-13 * max(1.0, float(terms.abs().max()))
    assert float((ev["g_pred"][0] - gp).abs().max()) <= 1e-12 * max(float(gp.abs().max()), 1e-300)
    assert float((ev["g_ws"][0] - gw).abs().max()) <= 1e-12 * float(gw.abs().max())
    if hit_mode == "zero":
        assert float(ev["terms"][0][0]) == 0.0 and not bool(ev["g_pred"][0].any())
    # the inclusive rule: a weight sum AT a bound passes its gradient, one step outside does not
    lo, hi = torch.tensor(1e-3), torch.tensor(1.0 - 1e-3)
    for b, out in ((lo, torch.nextafter(lo, lo * 0)), (hi, torch.nextafter(hi, hi + 1))):
        e2 = ev64.mask_loss(pred[:1].expand(2, 3), gt[:1].expand(2, 3), None, torch.stack([b, out]), torch.tensor([1.0, 0.0]))
        assert float(e2["g_ws"][0][0]) != 0.0 and float(e2["g_ws"][0][1]) == 0.0


@pytest.mark.parametrize("R", [63, 257])
def test_loss_bars_admit_a_plain_fp32_torch_evaluation_and_bite(R):
    pred, gt, hit, ws, gm = ev64.mask_loss_cases(R, "mixed", seed=1)
    ev = ev64.mask_loss(pred, gt, hit, ws, gm)
    assert not _outside_loss(ev, *_loss_fp32(pred, gt, hit, ws, gm), R)
    # a missing hit mask: the colour term and its gradient
    out = _outside_loss(ev, *_loss_fp32(pred, gt, hit, ws, gm, use_hit=False), R)
    assert {"terms", "loss", "g_pred"} <= out and "g_ws" not in out, out
    # a cross entropy without the clip: the mask term, and a gradient where the clip should have stopped it
    out = _outside_loss(ev, *_loss_fp32(pred, gt, hit, ws, gm, clip=False), R)
    assert {"terms", "g_ws"} <= out and "g_pred" not in out, out


# ------------------------------------------------------------------------------------------------------- the native side
def _cxx():
    return next((c for c in ("/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++", shutil.which("clang++"),
                             shutil.which("g++")) if c and os.path.exists(c)), None)


def _sanitized(tmp_path, source, std, extra):
    """a stand-alone program with its own main, the sanitizers linked into it: nothing is preloaded, no Python-loaded code runs
    under a sanitizer"""
    cxx = _cxx()
    if cxx is None:
        pytest.skip("neither ROCm's clang++ nor g++ is installed")
    exe = str(tmp_path / source[:-4])
    cmd = [cxx, "-x", "c++", "-std=" + std, "-ffp-contract=off", "-Wno-unused-function", "-O1", "-g", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", CSRC] + extra + [os.path.join(ROOT, "tests", "host", source), "-o", exe, "-lpthread"]
    if not cxx.endswith("clang++"):     # clang links the sanitizer runtimes into the program by default, g++ on request
        cmd[1:1] = ["-static-libasan", "-static-libubsan"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, " ".join(cmd) + "\n" + r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
    print(r.stdout)


def test_plan_header_under_sanitizers(tmp_path):
    """csrc/neus_render_plan.h alone, as plain C++17: tests/host/neus_render_plan_check.cpp"""
    _sanitized(tmp_path, "neus_render_plan_check.cpp", "c++17", [])


def test_loss_tail_source_on_cpu_threads_under_sanitizers(tmp_path):
    """csrc/neus_render.hip itself, compiled as C++ against tests/host/hip_on_host, its loss tail driven like neus.py drives it and
    compared with brute-force float64 by tests/host/neus_mask_loss_check.cpp: values at R in {1, 255, 256, 257, limit, limit + 1}
    with the weight sums on, beside and between the clip bounds, hit null / all zero / mixed; a non-zero accumulator is added to;
    two calls give the same bits"""
    _sanitized(tmp_path, "neus_mask_loss_check.cpp", "c++20", ["-I", os.path.join(ROOT, "tests", "host", "hip_on_host")])


def test_plan_header_is_host_only_and_the_file_follows_the_single_home_rules():
    src = open(os.path.join(CSRC, "neus_render_plan.h")).read()
    assert set(re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", src)) <= {"cstdint"}
    assert not re.search(r"\bhip[A-Z_]|__device__|__global__|__host__", src)
    hip = open(os.path.join(CSRC, "neus_render.hip")).read()
    code = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", hip, flags=re.S))
    for inc in ("composite_device.h", "neus_render_plan.h"):
        assert '#include "%s"' % inc in hip
    # the grid cap, the single-group limit and the chunk borders did not stay behind as copies; no inline assembly
    assert "MAX_GRID =" not in code and "512" not in code and "128" not in code and "8192" not in code and "asm" not in code
    # the loss tail holds no atomic: the only one of the file is the inv_s gradient's, one per wave as in composite_fused.hip
    assert len(re.findall(r"\batomic\w*\s*\(", code)) == 1 and "atomicAdd(g_inv_s" in code
    tail = code[code.index("struct LossArgs"):code.index('extern "C"')]
    assert "atomic" not in tail and "double acc[TERMS]" in tail and "__syncthreads" in tail
    for text in ("1e-7f", "1e-5f", "1e-12f", "0x7fc00000", "den * den", "log1pf(expf(", "dispatch_chunks(", "wave_incl_scan_mul"):
        assert text not in code, text
    for helper in ("section(", "section_backward(", "clip01(", "sweep(", "sweep_chunk(", "Transmittance", "SuffixStep", "poison_ray(", "RayIndex"):
        assert helper in code, helper
    # composite_fused.hip and composite_device.h are as they were: the new file is a caller, not an edit
    fused = open(os.path.join(CSRC, "composite_fused.hip")).read()
    assert "neus_render" not in fused and "weights_sum" not in fused


@pytest.fixture(scope="module")
def lib():
    from permuto_sdf_amd import build
    return ctypes.CDLL(build.build(verbose=False))


def test_library_exports_exactly_the_declared_neus_render_entries(lib):
    header = open(os.path.join(ROOT, "include", "psdf.h")).read()
    assert "/* ---- neus_render.hip ---- */" in header
    start = header.index("/* ---- neus_render.hip ---- */")
    section = header[start:header.index("/* ---- ", start + 10)]
    assert sorted(set(re.findall(r"\bint (psdf_[a-z0-9_]+)\s*\(", section))) == NAMES
    assert not [n for n in NAMES if not hasattr(lib, n)]
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    if os.path.exists(nm):
        out = subprocess.run([nm, "-D", "--defined-only", lib._name], capture_output=True, text=True).stdout
        got = sorted(set(re.findall(r"\b(psdf_neus_(?:render|mask)[a-z0-9_]*)\b", out)))
        assert got == NAMES, got
    assert int(re.search(r"#define PSDF_NEUS_RENDER_PLAN_FIELDS (\d+)", header).group(1)) == 4
    src = open(os.path.join(CSRC, "neus_render_plan.h")).read()
    block, cap = int(re.search(r"BLOCK = (\d+);", src).group(1)), int(re.search(r"MAX_GRID = (\d+);", src).group(1))
    per = int(re.search(r"RAYS_PER_THREAD_SINGLE = (\d+);", src).group(1))
    from permuto_sdf_amd import neus
    lim = block * per
    assert neus.NEUS_RENDER_PLAN_FIELDS == 4 and lim >= 8192          # the trainer's ray cap (train_step.py, _refresh_and_adapt)
    assert neus.neus_render_plan(512, 64) == (1, 1, 0, lim)
    assert neus.neus_render_plan(0, 65) == (2, 0, 0, lim)
    assert neus.neus_render_plan(lim, 128) == (2, 1, 0, lim)
    assert neus.neus_render_plan(lim + 1, 129) == (4, lim // block + 1, (lim // block + 1) * 16, lim)
    assert neus.neus_render_plan(block * cap + 1, 256) == (4, cap, cap * 16, lim)


def test_empty_inputs_return_before_any_pointer_check_and_bad_arguments_are_refused(lib):
    i64, f, st = ctypes.c_int64, ctypes.c_float, None
    p = ctypes.c_void_p(4096)          # never read: every call below returns before a launch
    out = (ctypes.c_int64 * 4)()
    assert lib.psdf_neus_render_plan(i64(-1), 64, out) == -1 and lib.psdf_neus_render_plan(i64(1), 0, out) == -1
    assert lib.psdf_neus_render_plan(i64(1), 64, None) == -1
    assert lib.psdf_neus_render_plan(i64(2 ** 31 // 3 + 1), 64, out) == -2 and lib.psdf_neus_render_plan(i64(1), 257, out) == -2
    assert lib.psdf_neus_render_forward(0, None, 0, 0, 0, None, None, None, None, None, None, f(0.5), None, None, None, st) == 0
    assert lib.psdf_neus_render_backward(0, None, 0, 0, 0, 999, None, None, None, None, None, None, None, None, None, f(0.5), 0, None,
                                         None, None, None, st) == 0
    assert lib.psdf_neus_mask_loss(i64(0), None, None, None, None, None, f(1.0), f(1.0), None, None, None, None, st) == 0

    def fwd(se=p, equal=0, sdf=p, dirs=p, grad=p, dt=p, rgb=p, inv=p, pred=p, ws=p, bg=p):
        return lib.psdf_neus_render_forward(1, se, equal, 1, 1, sdf, dirs, grad, dt, rgb, inv, f(0.5), pred, ws, bg, st)

    assert fwd(se=None) == -1 and fwd(sdf=None) == -1 and fwd(dirs=None) == -1 and fwd(grad=None) == -1 and fwd(dt=None) == -1
    assert fwd(rgb=None) == -1 and fwd(inv=None) == -1 and fwd(pred=None, ws=None, bg=None) == -1

    def bwd(se=p, mpr=64, gp=p, gw=p, gb=p, sdf=p, dirs=p, grad=p, dt=p, rgb=p, inv=p, g_sdf=p):
        return lib.psdf_neus_render_backward(1, se, 0, 1, 1, mpr, gp, gw, gb, sdf, dirs, grad, dt, rgb, inv, f(0.5), 0, g_sdf, p, p, p, st)

    assert bwd(se=None) == -1 and bwd(gp=None, gw=None, gb=None) == -1 and bwd(sdf=None) == -1 and bwd(dirs=None) == -1
    assert bwd(grad=None) == -1 and bwd(dt=None) == -1 and bwd(rgb=None) == -1 and bwd(inv=None) == -1 and bwd(g_sdf=None) == -1
    assert bwd(mpr=0) == -1 and bwd(mpr=257) == -2

    def loss(R=1, pred=p, gt=p, ws=p, gm=p, a=1.0, b=1.0, work=p, acc=p):
        return lib.psdf_neus_mask_loss(i64(R), pred, gt, p, ws, gm, f(a), f(b), work, acc, p, p, st)

    assert loss(pred=None) == -1 and loss(gt=None) == -1 and loss(ws=None) == -1 and loss(gm=None) == -1 and loss(acc=None) == -1
    assert loss(a=float("nan")) == -1 and loss(b=float("nan")) == -1
    assert loss(R=8193, work=None) == -1                # above the single-group limit the partial sums need their workspace
    assert loss(R=2 ** 31 // 3 + 1) == -2


def _fake_container(R, N):
    """what the wrappers read of a RaySamplesPacked before a launch, on the CPU"""
    return SimpleNamespace(ray_start_end_idx=torch.zeros(R, 2, dtype=torch.int32), samples_dirs=torch.zeros(N, 3), samples_dt=torch.zeros(N, 1),
                           rays_have_equal_nr_of_samples=False, fixed_nr_of_samples_per_ray=0, max_nr_samples=N)


def test_wrappers_refuse_mismatched_shapes_before_touching_a_device():
    from permuto_sdf_amd import neus
    from permuto_sdf_amd._lib import PsdfError
    R, N = 4, 10
    rs = _fake_container(R, N)
    sdf, grad, rgb, inv = torch.zeros(N, 1), torch.zeros(N, 3), torch.zeros(N, 3), torch.ones(1)
    with pytest.raises(ValueError):
        neus.neus_render_forward_raw(rs, sdf, grad[:-1], rgb, inv, 0.5)
    with pytest.raises(ValueError):
        neus.neus_render_forward_raw(rs, sdf, grad, rgb[:, :2], inv, 0.5)
    with pytest.raises(ValueError):
        neus.neus_render_forward_raw(rs, sdf, grad, rgb, torch.ones(2), 0.5)
    with pytest.raises(ValueError):
        neus.neus_render_forward_raw(rs, sdf, grad, rgb, inv, 0.5, want_pred=False, want_weights_sum=False, want_bg=False)
    with pytest.raises(ValueError):
        neus.neus_render_forward_raw(_fake_container(R, N - 1), sdf, grad, rgb, inv, 0.5)
    gp, gw = torch.zeros(R, 3), torch.zeros(R, 1)
    with pytest.raises(ValueError):
        neus.neus_render_backward_raw(rs, 64, None, None, None, sdf, grad, rgb, inv, 0.5)
    with pytest.raises(ValueError):
        neus.neus_render_backward_raw(rs, 64, gp[:-1], gw, None, sdf, grad, rgb, inv, 0.5)
    with pytest.raises(ValueError):
        neus.neus_render_backward_raw(rs, 64, gp, gw[:-1], None, sdf, grad, rgb, inv, 0.5)
    with pytest.raises(ValueError):
        neus.neus_render_backward_raw(rs, 64, gp, gw, None, sdf, grad[:, :2], rgb, inv, 0.5)
    pred, gt, hit, ws, gm = ev64.mask_loss_cases(7)
    with pytest.raises(ValueError):
        neus.neus_mask_loss_raw(pred, gt[:-1], hit, ws, gm, 0.1)
    with pytest.raises(ValueError):
        neus.neus_mask_loss_raw(pred, gt, hit[:-1], ws, gm, 0.1)
    with pytest.raises(ValueError):
        neus.neus_mask_loss_raw(pred, gt, hit, ws[:-1], gm, 0.1)
    with pytest.raises(ValueError):
        neus.neus_mask_loss_raw(pred, gt, hit, ws, gm[:-1], 0.1)
    # well-formed CPU tensors: there is no CPU path, and the refusal still comes before any launch
    with pytest.raises(PsdfError):
        neus.neus_render_forward_raw(rs, sdf, grad, rgb, inv, 0.5)
    with pytest.raises(PsdfError):
        neus.neus_render_backward_raw(rs, 64, gp, gw, None, sdf, grad, rgb, inv, 0.5)
    with pytest.raises(PsdfError):
        neus.neus_mask_loss_raw(pred, gt, hit, ws, gm, 0.1)


def test_the_hand_written_step_accepts_masked_runs_on_the_foreground_bound_alone():
    """`_hand_written_step_applies` reads the hyper-parameters and the mask switch only: no device"""
    from permuto_sdf_amd.train_manual import ManualTrainer
    from permuto_sdf_amd.train_step import HyperParams
    def applies(with_mask, **over):
        hp = HyperParams()
        for k, v in over.items():
            setattr(hp, k, v)
        return ManualTrainer._hand_written_step_applies(SimpleNamespace(hp=hp, with_mask=with_mask))
    assert applies(True) and applies(False)
    assert applies(True, nr_samples_bg=1000) and not applies(False, nr_samples_bg=1000)      # no background under a mask
    assert not applies(True, max_nr_samples_per_ray=256) and not applies(False, max_nr_samples_per_ray=256)
