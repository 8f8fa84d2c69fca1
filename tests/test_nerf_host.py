"""The host side of NeRF training (permuto_sdf_amd/nerf_train.py, csrc/nerf_render.hip), checked without a GPU.

  * the yardstick of the GPU tests, tests/nerf_render_float64.py, equals torch autograd in float64 of
    VolumeRenderingNerf.compute_weights + integrate and the two loss lines of train_nerf.py restated in torch operators, and its
    float64 family keeps every 1 - alpha + 1e-7 above 1e-4 (the backward's floor is inactive there);
  * its bars admit a plain fp32 torch evaluation of that formula, and they bite: a dropped g_weights_sum, a dropped background
    term, a missing hit mask and a cross entropy without the clip each land outside them;
  * csrc/nerf_render_plan.h is host-only arithmetic with a sanitized stand-alone check; the loss tail and the head join run as the
    kernels' own source on CPU threads (tests/host/hip_on_host) under the address and undefined-behaviour sanitizers;
  * the library exports exactly the new names the header declares; empty inputs and bad arguments return their codes with no GPU;
    the module refuses what it cannot run before it touches a device."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

from tests import nerf_render_float64 as ev64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "permuto_sdf_amd", "csrc")
CONTAINERS = ["borders", "equal1", "equal65", "equal129"]
NAMES = ["psdf_nerf_head_join", "psdf_nerf_head_join_backward", "psdf_nerf_loss", "psdf_nerf_render_backward",
         "psdf_nerf_render_forward", "psdf_nerf_render_plan"]


def _up(c, subset, seed=0):
    g = ev64.upstream(c, seed)
    return [t if on else None for t, on in zip(g, subset)]


def _autograd(rays, raw, dt, rgb, ups, dtype, **kw):
    """torch autograd of the restated render in `dtype` for the upstream gradients `ups` -> (pred, ws, bg, g_raw, g_rgb)"""
    raw_g, rgb_g = raw.to(dtype).requires_grad_(True), rgb.to(dtype).requires_grad_(True)
    pred, ws, bg = ev64.render_torch(rays, raw_g, dt, rgb_g, dtype, **kw)
    total = raw_g.sum() * 0
    for out, g in zip((pred, ws, bg), ups):
        if g is not None:
            total = total + (out * g.to(dtype).reshape(out.shape)).sum()
    g_raw, g_rgb = torch.autograd.grad(total, (raw_g, rgb_g), allow_unused=True)
    g_rgb = torch.zeros_like(rgb_g) if g_rgb is None else g_rgb
    return pred.detach(), ws.detach(), bg.detach(), g_raw, g_rgb


@pytest.mark.parametrize("cname", CONTAINERS)
def test_render_evaluator_is_torch_autograd_in_float64(cname):
    c = ev64.container(cname)
    rays = ev64.rays_of(c)
    raw, dt, rgb = ev64.family(c, "float64")
    for subset in ev64.SUBSETS:
        ups = _up(c, subset)
        ev = ev64.render(rays, raw, dt, rgb, *ups)
        assert ev["min_om"] > 1e-4                      # the floor max(om, 1e-6) of the backward is inactive in this family
        pred, ws, bg, g_raw, g_rgb = _autograd(rays, raw, dt, rgb, ups, torch.float64)
        for name, want in (("pred", pred), ("weights_sum", ws), ("bg", bg), ("g_raw", g_raw), ("g_rgb", g_rgb)):
            got = ev[name][0]
            assert got.shape == want.shape, name
            assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), (name, subset)
    # rays the kernels skip: 0, 0, 1, and no sample of theirs is touched
    skipped = ~rays.valid
    if bool(skipped.any()):
        ev = ev64.render(rays, raw, dt, rgb, *ev64.upstream(c))
        assert not bool(ev["pred"][0][skipped].any()) and not bool(ev["weights_sum"][0][skipped].any())
        assert bool((ev["bg"][0][skipped] == 1).all())
        assert not bool(ev["g_raw"][0][~rays.touched(c["N"])].any())


@pytest.mark.parametrize("R", [1, 63, 257])
@pytest.mark.parametrize("with_hit", [True, False])
@pytest.mark.parametrize("with_mask", [True, False])
def test_loss_evaluator_is_torch_autograd_in_float64(R, with_hit, with_mask):
    pred, gt, hit, ws, gm = ev64.loss_cases(R)
    hit = hit if with_hit else None
    ev = ev64.loss(pred, gt, hit, ws if with_mask else None, gm if with_mask else None)
    p, w = pred.double().requires_grad_(True), ws.double().requires_grad_(True)
    # (the weight of the mask term is the fp32 0.1 the kernel is handed)
    loss, terms = ev64.loss_torch(p, gt.double(), hit, w if with_mask else None, gm.double() if with_mask else None, mask_weight=ev64._f32(0.1))
    loss = loss.detach() if not loss.requires_grad else loss
    gp, gw = torch.autograd.grad(loss, (p, w), allow_unused=True)
    assert abs(float(ev["loss"][0]) - float(loss.detach())) <= 1e-13 * max(1.0, abs(float(loss.detach())))
    assert float((ev["terms"][0] - terms).abs().max()) <= 1e-13
    assert float((ev["g_pred"][0] - gp).abs().max()) <= 1e-12 * float(gp.abs().max())
    if with_mask:
        assert float((ev["g_ws"][0] - gw).abs().max()) <= 1e-12 * float(gw.abs().max())
        # the inclusive rule: a weight sum AT a bound passes its gradient, one step outside does not
        lo, hi = torch.tensor(1e-3), torch.tensor(1.0 - 1e-3)
        for b, out in ((lo, torch.nextafter(lo, lo * 0)), (hi, torch.nextafter(hi, hi + 1))):
            e2 = ev64.loss(pred[:2], gt[:2], None, torch.stack([b, out]), torch.tensor([1.0, 0.0]))
            assert float(e2["g_ws"][0][0]) != 0.0 and float(e2["g_ws"][0][1]) == 0.0
    else:
        assert "g_ws" not in ev and float(ev["terms"][0][1]) == 0.0


def _outside_render(ev, pred, ws, bg, g_raw, g_rgb):
    out = set()
    for name, got in (("pred", pred), ("weights_sum", ws), ("bg", bg), ("g_raw", g_raw), ("g_rgb", g_rgb)):
        val, bar = ev[name]
        if bool(((got.double() - val).abs() > bar).any()):
            out.add(name)
    return out


@pytest.mark.parametrize("cname", CONTAINERS)
def test_render_bars_admit_a_plain_fp32_torch_evaluation_and_bite(cname):
    c = ev64.container(cname)
    rays = ev64.rays_of(c)
    raw, dt, rgb = ev64.family(c, "float64", seed=1)
    worst = 0.0
    for subset in ev64.SUBSETS:
        ups = _up(c, subset, seed=1)
        ev = ev64.render(rays, raw, dt, rgb, *ups)
        got = _autograd(rays, raw, dt, rgb, ups, torch.float32)
        assert not _outside_render(ev, *got), (subset, _outside_render(ev, *got))
        for name, g in zip(("pred", "weights_sum", "bg", "g_raw", "g_rgb"), got):
            val, bar = ev[name]
            worst = max(worst, float(((g.double() - val).abs() / bar.clamp_min(1e-300)).max()))
        # the bars bite: three quarters of the non-zero gradient entries at least are held to better than 1e-3 of themselves
        # (g_alpha = g_w T - g_om cancels on the rest: there the bar is that of the two parts), none is lost in its bar
        b, sat = ev64.c64.bites(ev["g_raw"][0], ev["g_raw"][1])
        assert not bool(ev["g_raw"][0].any()) or (b >= 0.75 and sat <= 0.01), (subset, b, sat)
    print("fp32 torch against the bars, %s: worst error / bar %.3f" % (cname, worst))
    # a backward that drops g_weights_sum / the background term lands outside, in the density's gradient alone
    ups = _up(c, (True, True, True), seed=1)
    ev = ev64.render(rays, raw, dt, rgb, *ups)
    assert _outside_render(ev, *_autograd(rays, raw, dt, rgb, ups, torch.float32, drop_ws=True)) == {"g_raw"}
    if c["max_per_ray"] > 1:        # (a ray of one sample has nothing in front of its background)
        assert _outside_render(ev, *_autograd(rays, raw, dt, rgb, ups, torch.float32, drop_bg=True)) == {"g_raw"}
    # and the reference's channel quirk is seen when it is not asked for
    quirk = ev64.render(rays, raw, dt, rgb, *ups, compat=True)
    assert bool(((quirk["g_raw"][0] - ev["g_raw"][0]).abs() > ev["g_raw"][1]).any())


def _loss_fp32(pred, gt, hit, ws, gm, **kw):
    p, w = pred.clone().requires_grad_(True), ws.clone().requires_grad_(True)
    loss, terms = ev64.loss_torch(p, gt, hit, w, gm, **kw)
    gp, gw = torch.autograd.grad(loss, (p, w))
    return loss.detach(), terms, gp, gw


def _outside_loss(ev, loss, terms, gp, gw, R):
    # torch's fp32 .mean() adds in fp32 (pairwise), the kernel in double: (ceil(log2 count) + 2) u of the mean on top
    import math
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


@pytest.mark.parametrize("R", [63, 257])
def test_loss_bars_admit_a_plain_fp32_torch_evaluation_and_bite(R):
    pred, gt, hit, ws, gm = ev64.loss_cases(R, seed=1)
    ev = ev64.loss(pred, gt, hit, ws, gm)
    assert not _outside_loss(ev, *_loss_fp32(pred, gt, hit, ws, gm), R)
    # a missing hit mask: the colour term and its gradient
    out = _outside_loss(ev, *_loss_fp32(pred, gt, hit, ws, gm, use_hit=False), R)
    assert {"terms", "loss", "g_pred"} <= out and "g_ws" not in out, out
    # a cross entropy without the clip: the mask term, and a gradient where the clip should have stopped it
    out = _outside_loss(ev, *_loss_fp32(pred, gt, hit, ws, gm, clip=False), R)
    assert {"terms", "g_ws"} <= out and "g_pred" not in out, out


def test_gelu_bars_admit_an_fp32_evaluation_of_the_kernels_formula():
    """gelu_erf of gelu_device.h step by step in fp32 (every product rounded once, the two fmas fused) around an erf and an
    exponential that are correctly rounded: inside the bars, which stay below 1e-5 everywhere"""
    z = torch.cat([torch.randn(4000, generator=torch.Generator().manual_seed(3)) * 3, torch.tensor([0.0, -10.0, 10.0, -6.5, 6.5, 1e-20])])
    (val, bar_val), (der, bar_der) = ev64.gelu_bars(z)
    f = lambda t: t.float().double()                               # one fp32 rounding of a float64 intermediate
    zd = z.double()
    erf = f(torch.erf(f(zd * ev64._f32(0.70710678118654752440))))
    cdf = f(0.5 * erf + 0.5)
    pdf = f(ev64._f32(0.3989422804014327) * f(torch.exp(f(f(-0.5 * zd) * zd))))
    assert bool(((f(zd * cdf) - val).abs() <= bar_val).all())
    assert bool(((f(zd * pdf + cdf) - der).abs() <= bar_der).all())
    assert float(bar_val.max()) < 1e-5 and float(bar_der.max()) < 1e-5


# ------------------------------------------------------------------------------------------------------- the native side
def _cxx():
    return next((c for c in ("/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++", shutil.which("clang++"),
                             shutil.which("g++")) if c and os.path.exists(c)), None)


def _sanitized(tmp_path, source, std, extra):
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
    """csrc/nerf_render_plan.h alone, as plain C++17: tests/host/nerf_render_plan_check.cpp, a program with its own main"""
    _sanitized(tmp_path, "nerf_render_plan_check.cpp", "c++17", [])


def test_loss_tail_and_head_join_source_on_cpu_threads_under_sanitizers(tmp_path):
    """csrc/nerf_render.hip itself, compiled as C++ against tests/host/hip_on_host, its loss tail and head join driven like
    nerf_train.py drives them and compared with brute-force float64 by tests/host/nerf_tail_kernels_check.cpp: a stand-alone
    program with its own main, under ASan and UBSan"""
    if _cxx() is not None and not _cxx().endswith("clang++"):
        pytest.skip("gelu_device.h is written in clang's vector extensions")
    _sanitized(tmp_path, "nerf_tail_kernels_check.cpp", "c++20", ["-I", os.path.join(ROOT, "tests", "host", "hip_on_host")])


def test_plan_header_is_host_only_and_the_file_follows_the_single_home_rules():
    src = open(os.path.join(CSRC, "nerf_render_plan.h")).read()
    assert set(re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", src)) <= {"cstdint"}
    assert not re.search(r"\bhip[A-Z_]|__device__|__global__|__host__", src)
    hip = open(os.path.join(CSRC, "nerf_render.hip")).read()
    code = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", hip, flags=re.S))
    for inc in ("composite_device.h", "gelu_device.h", "nerf_render_plan.h"):
        assert '#include "%s"' % inc in hip
    # the grid cap and the chunk borders did not stay behind as copies; no atomics, no inline assembly
    assert "MAX_GRID =" not in code and "512" not in code and "128" not in code
    assert "atomic" not in code and "asm" not in code
    for text in ("1e-7f", "1e-12f", "0x7fc00000", "den * den", "log1pf(expf(", "dispatch_chunks("):
        assert text not in code, text
    for helper in ("nerf_alpha(", "nerf_alpha_backward(", "sweep(", "sweep_chunk(", "Transmittance", "SuffixStep", "poison_ray(", "RayIndex", "gelu_erf("):
        assert helper in code, helper


@pytest.fixture(scope="module")
def lib():
    from permuto_sdf_amd import build
    return ctypes.CDLL(build.build(verbose=False))


def test_library_exports_exactly_the_declared_nerf_entries(lib):
    header = open(os.path.join(ROOT, "include", "psdf.h")).read()
    assert "/* ---- nerf_render.hip ---- */" in header
    section = header[header.index("/* ---- nerf_render.hip ---- */"):header.index("/* ---- sdf_fit.hip ---- */")]
    assert sorted(set(re.findall(r"\bint (psdf_[a-z0-9_]+)\s*\(", section))) == NAMES
    assert not [n for n in NAMES if not hasattr(lib, n)]
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    if os.path.exists(nm):
        out = subprocess.run([nm, "-D", "--defined-only", lib._name], capture_output=True, text=True).stdout
        got = sorted(set(re.findall(r"\b(psdf_nerf_(?:render|loss|head)[a-z0-9_]*)\b", out)))
        assert got == NAMES, got
    assert int(re.search(r"#define PSDF_NERF_RENDER_PLAN_FIELDS (\d+)", header).group(1)) == 4
    src = open(os.path.join(CSRC, "nerf_render_plan.h")).read()
    block, cap = int(re.search(r"BLOCK = (\d+);", src).group(1)), int(re.search(r"MAX_GRID = (\d+);", src).group(1))
    from permuto_sdf_amd import nerf_train
    assert nerf_train.PLAN_FIELDS == 4
    assert nerf_train.plan(512, 64) == (2, 32, block * cap, 1)
    assert nerf_train.plan(0, 65) == (0, 0, block * cap, 2)
    assert nerf_train.plan(block * cap + 1, 256) == (cap, cap * 16, block * cap, 4)


def test_empty_inputs_return_before_any_pointer_check_and_bad_arguments_are_refused(lib):
    i64, f, st = ctypes.c_int64, ctypes.c_float, None
    p = ctypes.c_void_p(4096)          # never read: every call below returns before a launch
    out = (ctypes.c_int64 * 4)()
    assert lib.psdf_nerf_render_plan(i64(-1), 64, out) == -1 and lib.psdf_nerf_render_plan(i64(1), 0, out) == -1
    assert lib.psdf_nerf_render_plan(i64(1), 64, None) == -1
    assert lib.psdf_nerf_render_plan(i64(2 ** 31 // 3 + 1), 64, out) == -2 and lib.psdf_nerf_render_plan(i64(1), 257, out) == -2
    assert lib.psdf_nerf_render_forward(0, None, 0, 0, 0, None, None, None, None, None, None, st) == 0
    assert lib.psdf_nerf_render_backward(0, None, 0, 0, 0, 999, None, None, None, None, None, None, 0, None, None, st) == 0
    assert lib.psdf_nerf_loss(i64(0), None, None, None, None, None, f(0.1), None, None, None, None, None, st) == 0
    assert lib.psdf_nerf_head_join(i64(0), None, None, None, st) == 0
    assert lib.psdf_nerf_head_join_backward(i64(0), None, None, None, None, st) == 0

    def fwd(se=p, equal=0, raw=p, dt=p, rgb=p, pred=p, ws=p, bg=p):
        return lib.psdf_nerf_render_forward(1, se, equal, 1, 1, raw, dt, rgb, pred, ws, bg, st)

    assert fwd(se=None) == -1 and fwd(raw=None) == -1 and fwd(dt=None) == -1 and fwd(rgb=None) == -1
    assert fwd(pred=None, ws=None, bg=None) == -1

    def bwd(se=p, mpr=64, gp=p, gw=p, gb=p, raw=p, dt=p, rgb=p, g_raw=p, g_rgb=p):
        return lib.psdf_nerf_render_backward(1, se, 0, 1, 1, mpr, gp, gw, gb, raw, dt, rgb, 0, g_raw, g_rgb, st)

    assert bwd(se=None) == -1 and bwd(gp=None, gw=None, gb=None) == -1 and bwd(raw=None) == -1 and bwd(dt=None) == -1
    assert bwd(rgb=None) == -1 and bwd(g_raw=None) == -1 and bwd(mpr=0) == -1 and bwd(mpr=257) == -2

    def loss(R=1, pred=p, gt=p, ws=p, gm=p, w=0.1, work=p, terms=p):
        return lib.psdf_nerf_loss(i64(R), pred, gt, p, ws, gm, f(w), work, terms, p, p, p, st)

    assert loss(pred=None) == -1 and loss(gt=None) == -1 and loss(ws=None) == -1 and loss(gm=None) == -1
    assert loss(work=None) == -1 and loss(terms=None) == -1 and loss(w=float("nan")) == -1
    assert loss(R=2 ** 31 // 3 + 1) == -2
    assert lib.psdf_nerf_head_join(i64(-1), p, p, p, st) == -1 and lib.psdf_nerf_head_join(i64(1), None, p, p, st) == -1
    assert lib.psdf_nerf_head_join(i64(1), p, None, p, st) == -1 and lib.psdf_nerf_head_join(i64(1), p, p, None, st) == -1
    assert lib.psdf_nerf_head_join(i64(2 ** 31), p, p, p, st) == -2
    assert lib.psdf_nerf_head_join_backward(i64(1), None, p, p, p, st) == -1 and lib.psdf_nerf_head_join_backward(i64(1), p, None, p, p, st) == -1
    assert lib.psdf_nerf_head_join_backward(i64(1), p, p, None, p, st) == -1 and lib.psdf_nerf_head_join_backward(i64(1), p, p, p, None, st) == -1
    assert lib.psdf_nerf_head_join_backward(i64(2 ** 31), p, p, p, p, st) == -2


def test_module_refuses_what_it_cannot_run_before_it_touches_a_device():
    import permuto_sdf_amd
    from permuto_sdf_amd import nerf_train as nt
    from permuto_sdf_amd._lib import PsdfError
    from permuto_sdf_amd.train_step import BgNet
    assert permuto_sdf_amd.nerf_train is nt and "nerf_train" in permuto_sdf_amd.__all__
    with pytest.raises(NotImplementedError):      # colour calibration is left out; no device is needed to say so
        nt.NerfTrainer("cuda:0", colorcal=object())
    pred, gt, hit, ws, gm = ev64.loss_cases(7)
    with pytest.raises(PsdfError):                # CPU tensors: there is no CPU path
        nt.nerf_loss_raw(pred, gt, hit, ws, gm)
    with pytest.raises(PsdfError):
        nt.nerf_head_join_raw(torch.zeros(65, 3), torch.zeros(3, 16))
    with pytest.raises(ValueError):
        nt.NerfNet(pos_dim=2)
    # the torch form of the loss is the helper's formula
    a, ta = nt.nerf_loss_torch(pred.double(), gt.double(), hit, ws.double(), gm.double())
    b, tb = ev64.loss_torch(pred.double(), gt.double(), hit, ws.double(), gm.double(), lo=1e-3, hi=1.0 - 1e-3)
    assert float(a) == float(b) and torch.equal(ta, tb)
    # NerfNet: BgNet's layers and parameter names in 3 and 4 dimensions, the reference's window
    torch.manual_seed(0)
    ref = BgNet()
    for dim in (3, 4):
        net = nt.NerfNet(dim, nr_iters_for_c2f=10000)
        assert isinstance(net, BgNet) and net.encoding.cfg.pos_dim == dim
        assert [k for k in net.state_dict()] == [k for k in ref.state_dict()]
        shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
        want = {k: tuple(v.shape) for k, v in ref.state_dict().items()}
        if dim == 4:
            assert shapes == want
        assert shapes["mlp_feat_and_density.layers.3.weight"] == (65, 64) and shapes["mlp_rgb.layers.0.weight"] == (64, 80)
        w0, w1 = net.window(0), net.window(10000)
        assert float(w1.min()) == 1.0 and float(w0.sum()) < 24 * 0.31 + 1 and float(w0[0]) == 1.0
    assert float(nt.NerfNet(3, 1).window(1).min()) == 1.0
