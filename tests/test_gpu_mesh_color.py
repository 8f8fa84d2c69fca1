"""Coloured meshes on the GPU (permuto_sdf_amd/mesh_color.py, csrc/mesh_color.hip): real networks, `SdfNet(hp)` and `RgbNet(hp)`
seeded; points uniform in the ball of radius 0.5.

  1. the input assembly: after the colour encode and `psdf_mesh_color_inputs`, x_fm is bit for bit the torch.cat of the operators
     `ManualTrainer._fg_forward` uses, over one wave, its edges and more than one workgroup, with a zero gradient, a gradient
     below the eps and (camera mode) a vertex at the eye;
  2. the whole chain: `colors(points)` is bit for bit the chain of the existing raw operators run on the same chunks, three
     chunks with a partial last one and a single chunk; different chunkings are NOT compared with each other;
  3. against float64 (tests/mlp_float64.py over the float64 Lipschitz normalisation of oracle/lipshitz_float64.py, on the fp32
     x_fm): the worst entry of the new rgb errs at most twice as far as the worst entry of `RgbNet.forward` -- two fp32
     evaluations of one net with different summation orders: errors of one size, not of one value.  Both numbers go to
     profiles/mesh_color_gpu_tests.txt; no 8-bit channel differs from the module chain's by more than one level (how many differ
     is recorded, not bounded);
  4. end to end on a net fitted to a sphere: `colored_mesh`, `filter_vertices`, `save_ply` and back, a camera against "normal";
  5. the edges: no vertices, points on another device, a chunk larger than any launch, `fast=True`.
"""
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(ROOT, "profiles", "mesh_color_gpu_tests.txt")
N_CHAIN, CHUNK = 600, 256


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _within_one_ulp(a, b):
    ia, ib = _bits(a).long(), _bits(b).long()
    return bool(((((ia - ib).abs() <= 1) & ((ia < 0) == (ib < 0))) | ((a == 0) & (b == 0))).all())


def _ball(n, seed, dev):
    g = torch.Generator().manual_seed(seed)
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=1)
    return (d * 0.5 * torch.rand(n, 1, generator=g) ** (1.0 / 3.0)).to(dev).contiguous()


@pytest.fixture(scope="module")
def nets(dev):
    from permuto_sdf_amd.train_step import HyperParams, RgbNet, SdfNet
    hp = HyperParams()
    torch.manual_seed(11)
    sdf, rgb = SdfNet(hp).to(dev), RgbNet(hp).to(dev)
    with torch.no_grad():       # a colour lattice that says something (1e-5 at initialisation), biases that are not all zero
        rgb.encoding.lattice_values.mul_(1e3)
        for b in rgb.mlp.biases_per_layer:
            b.normal_(0.0, 0.1)
    return types.SimpleNamespace(sdf=sdf, rgb=rgb, hp=hp)


def _sdf_stage(nets, p):
    """the SDF net on a chunk, by the raw operators of ManualTrainer._fg_forward -> (y [1 + g, n], gradient [n, 3])"""
    from permuto_sdf_amd.mlp import mlp_forward_raw, pack_params
    from permuto_sdf_amd.net_eval import enc_forward, net_params, sdf_gradient
    from permuto_sdf_amd.mesh_color import _IT_WINDOW_OPEN
    sdf = nets.sdf
    dims, _, ws, bs = net_params(sdf.mlp_sdf)
    net = types.SimpleNamespace(dims=dims, ws=ws, bs=bs, win=sdf.window(_IT_WINDOW_OPEN).contiguous(), packed=pack_params(dims, ws, bs))
    feat = enc_forward(sdf.encoding, p, net.win, train=False)
    y = mlp_forward_raw(dims, feat, net.packed)
    grad, _, _ = sdf_gradient(sdf.encoding, feat, p, net)
    return y, grad


def _x_of(nets, p, y, grad, dirs=None):
    """x_rgb as _fg_forward assembles it (dirs None: -normalize(grad))"""
    from permuto_sdf_amd.bridge import PermutoSDF
    from permuto_sdf_amd.net_eval import enc_forward
    from permuto_sdf_amd.train_manual import _normalize3
    feat2 = enc_forward(nets.rgb.encoding, p, nets.rgb._win, train=False)
    nn = _normalize3(grad)
    sh = PermutoSDF.spherical_harmonics(-nn if dirs is None else dirs, 5)
    return torch.cat([feat2, sh.t(), nn.t(), y[1:]], 0), nn


def _operator_chain(nets, pts, chunk):
    """the yardstick of (2) and (3): the existing raw operators on the chunks `colors` takes -> rgb, normals, gradients, x_fm per
    chunk"""
    from permuto_sdf_amd.mlp import lipshitz_normalize_all_raw, mlp_forward_raw, pack_params
    from permuto_sdf_amd.neus import sigmoid_rows_raw
    m = nets.rgb.mlp
    wn = lipshitz_normalize_all_raw(m.weights_per_layer, m.lipshitz_bound_per_layer)
    packed = pack_params(m.dims, wn, [b.detach() for b in m.biases_per_layer])
    rgb, normals, grads, xs, ys = [], [], [], [], []
    for a in range(0, pts.shape[0], chunk):
        p = pts[a:a + chunk].contiguous()
        y, grad = _sdf_stage(nets, p)
        x, nn = _x_of(nets, p, y, grad)
        rgb.append(sigmoid_rows_raw(mlp_forward_raw(m.dims, x, packed)))
        normals.append(nn), grads.append(grad), xs.append(x), ys.append(y)
    return types.SimpleNamespace(rgb=torch.cat(rgb), normals=torch.cat(normals), grads=torch.cat(grads), xs=xs, ys=ys)


@pytest.fixture(scope="module")
def points(dev):
    return _ball(N_CHAIN, 5, dev)


@pytest.fixture(scope="module")
def yard(nets, points):
    """computed once, shared by (2), (3) and (5), never written"""
    with torch.no_grad():
        return {CHUNK: _operator_chain(nets, points, CHUNK), 1 << 18: _operator_chain(nets, points, 1 << 18)}


# ------------------------------------------------------------------------------------------------ 1. the input assembly
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@torch.no_grad()
def test_input_rows_are_the_operators_bit_for_bit(dev, nets, points, n):
    from permuto_sdf_amd import _lib as L
    from permuto_sdf_amd.bridge import PermutoSDF
    from permuto_sdf_amd.mesh_color import MODE_CAMERA, MODE_NORMAL, ColorPlan
    from permuto_sdf_amd.net_eval import enc_forward
    p = points[:n].contiguous()
    y, grad = _sdf_stage(nets, p)
    grad = grad.clone()
    grad[0] = 0.0                                                         # a zero gradient
    if n > 1:
        grad[n - 1] = torch.tensor([1e-20, -2e-20, 0.5e-20], device=dev)   # below the eps, at the end of the batch
    g, C = y.shape[0] - 1, nets.rgb.mlp.dims[0]
    plan = ColorPlan(nets.rgb.encoding.cfg.channels, g, C, n, n)
    assert (plan.C, plan.c_geom - plan.c_normal, plan.nr_chunks, plan.last_chunk) == (C, g, 1, n)
    eye = p[min(2, n - 1)].clone()                                        # a vertex equal to the eye
    for mode in (MODE_NORMAL, MODE_CAMERA):
        x_fm = torch.full((C, n), float("nan"), device=dev)
        dirs, normals = torch.full((n, 3), float("nan"), device=dev), torch.full((n, 3), float("nan"), device=dev)
        enc_forward(nets.rgb.encoding, p, nets.rgb._win, train=False, out=x_fm[:plan.c_enc])
        L.call("psdf_mesh_color_inputs", L.c_l(n), L.ptr(p), L.ptr(grad), L.ptr(y), L.c_i(g), L.c_i(mode), L.ptr(eye), L.ptr(x_fm),
               L.c_i(C), L.c_i(plan.c_enc), L.ptr(dirs), L.ptr(normals), L.stream())
        if mode == MODE_NORMAL:
            want, nn = _x_of(nets, p, y, grad)
            assert _same_bits(dirs, -nn)
        else:
            # the eps-normalised difference restated in torch, one rounding per operation in the kernel's order
            df = p - eye
            den = torch.sqrt(df[:, 0] * df[:, 0] + df[:, 1] * df[:, 1] + df[:, 2] * df[:, 2]).clamp_min(1e-12)
            assert _within_one_ulp(dirs, df / den[:, None])
            assert not bool(dirs[min(2, n - 1)].any())
            want, nn = _x_of(nets, p, y, grad, dirs=dirs)                 # SH of the kernel's own directions, bit for bit
            assert _same_bits(x_fm[plan.c_enc:plan.c_sh], PermutoSDF.spherical_harmonics(dirs, 5).t())
        assert _same_bits(normals, nn) and not bool(normals[0].any())
        assert _same_bits(x_fm, want), [r for r in range(C) if not _same_bits(x_fm[r], want[r])]
    # NULL side outputs: the same rows
    again = torch.full((C, n), float("nan"), device=dev)
    enc_forward(nets.rgb.encoding, p, nets.rgb._win, train=False, out=again[:plan.c_enc])
    L.call("psdf_mesh_color_inputs", L.c_l(n), L.ptr(p), L.ptr(grad), L.ptr(y), L.c_i(g), L.c_i(MODE_CAMERA), L.ptr(eye), L.ptr(again),
           L.c_i(C), L.c_i(plan.c_enc), None, None, L.stream())
    assert _same_bits(again, x_fm)


# --------------------------------------------------------------------------------------------------- 2. the whole chain
@pytest.mark.parametrize("chunk", [CHUNK, 1 << 18])
def test_colors_are_the_operator_chain_bit_for_bit(dev, nets, points, yard, chunk):
    from permuto_sdf_amd import image_eval
    from permuto_sdf_amd.mesh_color import MeshColorizer
    got = MeshColorizer(nets.sdf, nets.rgb).colors(points, chunk=chunk)
    want = yard[chunk]
    assert got.rgb.shape == (N_CHAIN, 3) and got.rgb.dtype == torch.float32 and got.rgb_u8.dtype == torch.uint8
    assert _same_bits(got.normals, want.normals)
    assert _same_bits(got.rgb, want.rgb), "entries that differ: %d" % int((_bits(got.rgb) != _bits(want.rgb)).sum())
    assert torch.equal(got.rgb_u8, image_eval.to_u8(want.rgb))
    assert float(got.rgb.min()) > 0.0 and float(got.rgb.max()) < 1.0
    # the points are not written, a second call gives the same bits
    assert _same_bits(MeshColorizer(nets.sdf, nets.rgb).colors(points, chunk=chunk).rgb, got.rgb)


# ------------------------------------------------------------------------------------------------- 3. against float64
def _arbiter(nets, x_fm):
    """the colour MLP and the sigmoid in float64 on the fp32 x_fm [C, n], over the float64 Lipschitz normalisation -> [n, 3]"""
    from oracle import lipshitz_float64 as l64
    from tests import mlp_float64 as m64
    m = nets.rgb.mlp
    lin = [types.SimpleNamespace(weight=l64.forward(w.detach().cpu(), c.detach().cpu())["Wn"], bias=b.detach().cpu())
           for w, c, b in zip(m.weights_per_layer, m.lipshitz_bound_per_layer, m.biases_per_layer)]
    x = x_fm.detach().cpu().t().contiguous()
    y = m64._f64_trace(lin, x, torch.zeros(x.shape[0], m.dims[-1]))[0]
    return torch.sigmoid(y)


def _module_chain(nets, pts):
    """the old way: FrameRenderer._sdf_and_gradient + RgbNet.forward + image_eval.to_u8, looking along -normal"""
    from permuto_sdf_amd import image_eval, render
    from permuto_sdf_amd.mesh_color import _IT_WINDOW_OPEN
    holder = types.SimpleNamespace(sdf=nets.sdf, rgb=nets.rgb, bg=None, grid=None, sphere=None, hp=nets.hp, with_mask=True)
    rnd = render.FrameRenderer(holder)
    _, grad, feat = rnd._sdf_and_gradient(pts, _IT_WINDOW_OPEN)
    dirs = -torch.nn.functional.normalize(grad, dim=1)
    with torch.no_grad():
        rgb = nets.rgb(pts, dirs, grad, feat).detach().float()
    return rgb, image_eval.to_u8(rgb)


def _record(lines):
    os.makedirs(os.path.dirname(RECORD), exist_ok=True)
    old = open(RECORD).read().splitlines() if os.path.exists(RECORD) else []
    keys = {l.split(":")[0] for l in lines}
    with open(RECORD, "w") as fh:
        fh.write("\n".join([l for l in old if l.split(":")[0] not in keys] + lines) + "\n")


def test_error_against_float64_is_of_the_size_of_the_modules(dev, nets, points, yard, capsys):
    from permuto_sdf_amd.mesh_color import MeshColorizer
    got = MeshColorizer(nets.sdf, nets.rgb).colors(points, chunk=1 << 18)
    ref = _arbiter(nets, yard[1 << 18].xs[0])
    module_rgb, module_u8 = _module_chain(nets, points)
    err_new = float((got.rgb.double().cpu() - ref).abs().max())
    err_module = float((module_rgb.double().cpu() - ref).abs().max())
    levels = (got.rgb_u8.int() - module_u8.int()).abs()
    lines = ["float64 n=%d: worst |rgb - f64| of MeshColorizer.colors %.3e, of RgbNet.forward %.3e (bar: twice the latter)" % (N_CHAIN, err_new, err_module),
             "8 bits n=%d: channels that differ from the module chain's to_u8: %d of %d, largest difference %d level(s)"
             % (N_CHAIN, int((levels > 0).sum()), levels.numel(), int(levels.max()))]
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    _record(lines)
    assert err_module > 0.0 and err_new <= 2.0 * err_module
    assert int(levels.max()) <= 1


# ---------------------------------------------------------------------------------------------------------- 4. end to end
@pytest.fixture(scope="module")
def fitted(dev):
    """tests/test_gpu_sphere_trace.py: fit_sphere_sdf, restated for an SdfNet (channel 0 of its head) -> FrameRenderer"""
    from permuto_sdf_amd import render
    from permuto_sdf_amd.optim import FusedAdamW
    from permuto_sdf_amd.train_step import HyperParams, RgbNet, SdfNet
    hp = HyperParams()
    torch.manual_seed(0)
    sdf, rgb = SdfNet(hp).to(dev), RgbNet(hp).to(dev)
    enc, mlp = sdf.encoding, sdf.mlp_sdf
    opt = FusedAdamW(list(enc.parameters())[:1] + list(mlp.parameters()), lr=5e-3)
    win = torch.ones(24, device=dev)
    for _ in range(300):
        x = torch.rand(16384, 3, device=dev) - 0.5
        loss = ((mlp(enc(x, win))[:, 0:1] - (x.norm(dim=1, keepdim=True) - 0.3)) ** 2).mean()
        for p in opt.param_groups[0]["params"]:
            p.grad = None
        loss.backward()
        opt.step()
    with torch.no_grad():
        rgb.encoding.lattice_values.mul_(1e3)
    holder = types.SimpleNamespace(sdf=sdf, rgb=rgb, bg=None, grid=None, sphere=None, hp=hp, with_mask=True)
    return render.FrameRenderer(holder)


def test_colored_mesh_filter_and_ply_round_trip(dev, fitted, tmp_path):
    from permuto_sdf_amd import mesh_clean
    from permuto_sdf_amd.render import Frame
    mesh = fitted.colored_mesh(32)
    nV = mesh.V.shape[0]
    assert nV >= 100 and mesh.C.shape == (nV, 3) and mesh.C.dtype == torch.uint8 and mesh.C.device == mesh.V.device
    colorizer = fitted.mesh_colorizer()
    plain = colorizer.colors(mesh.V)
    assert torch.equal(mesh.C, plain.rgb_u8)
    # every third vertex dropped: the colours of the kept ones, in their order
    keep = torch.ones(nV, dtype=torch.bool, device=dev)
    keep[::3] = False
    cut = mesh_clean.filter_vertices(mesh, keep)
    assert cut.V.shape[0] == int(keep.sum()) and torch.equal(cut.C, mesh.C[keep]) and torch.equal(cut.V, mesh.V[keep])
    # save_ply and back
    path = str(tmp_path / "coloured.ply")
    mesh.save_ply(path)
    data = open(path, "rb").read()
    body = data[data.index(b"end_header\n") + 11:]
    assert b"property uchar red\nproperty uchar green\nproperty uchar blue\nelement face" in data
    assert len(body) == 27 * nV + 13 * mesh.F.shape[0]
    rec = np.frombuffer(body[:27 * nV], dtype=[("v", "<f4", (3,)), ("n", "<f4", (3,)), ("c", "u1", (3,))])
    faces = np.frombuffer(body[27 * nV:], dtype=[("k", "u1"), ("i", "<i4", (3,))])
    assert np.array_equal(rec["v"], mesh.V.cpu().numpy()) and np.array_equal(rec["n"], mesh.NV.cpu().numpy())
    assert np.array_equal(rec["c"], mesh.C.cpu().numpy()) and np.array_equal(faces["i"], mesh.F.cpu().numpy())
    # a camera against "normal": other colours somewhere, the same normals
    tf = torch.eye(4)
    tf[:3, 3] = torch.tensor([0.2, -1.5, 0.7])
    seen = colorizer.colors(mesh.V, view=Frame(torch.eye(3), tf, 8, 8))
    assert _same_bits(seen.normals, plain.normals) and not torch.equal(seen.rgb, plain.rgb)
    assert torch.equal(colorizer.colors(mesh.V, view=[0.2, -1.5, 0.7]).rgb, seen.rgb)


# -------------------------------------------------------------------------------------------------------------- 5. edges
def test_no_vertices_another_device_and_bad_arguments(dev, nets, points, yard):
    from permuto_sdf_amd._lib import PsdfError
    from permuto_sdf_amd.mesh_color import MeshColorizer
    colorizer = MeshColorizer(nets.sdf, nets.rgb)
    # a chunk beyond what one launch takes is one chunk of all the vertices
    assert _same_bits(colorizer.colors(points, chunk=1 << 40).rgb, yard[1 << 18].rgb)
    none = colorizer.colors(points[:0])
    assert none.rgb.shape == (0, 3) and none.rgb_u8.shape == (0, 3) and none.normals.shape == (0, 3)
    assert none.rgb_u8.dtype == torch.uint8 and none.rgb.device == points.device
    with pytest.raises(PsdfError):
        colorizer.colors(points.cpu())
    if torch.cuda.device_count() > 1:
        with pytest.raises(PsdfError):
            colorizer.colors(points.to("cuda:1"))
    with pytest.raises(ValueError):
        colorizer.colors(points, chunk=0)
    with pytest.raises(ValueError):
        colorizer.colors(points, view="camera")
    with pytest.raises(ValueError):
        colorizer.colors(points, view=[1.0, 2.0])
    with pytest.raises(ValueError):
        colorizer.colors(points[:, :2])


def test_fast_is_within_the_bar_or_takes_the_fallback(dev, nets, points, yard, capsys):
    from permuto_sdf_amd.mesh_color import MeshColorizer
    colorizer = MeshColorizer(nets.sdf, nets.rgb)
    got = colorizer.colors(points, chunk=1 << 18, fast=True)
    ref = _arbiter(nets, yard[1 << 18].xs[0])
    module_rgb, _ = _module_chain(nets, points)
    err_fast = float((got.rgb.double().cpu() - ref).abs().max())
    err_module = float((module_rgb.double().cpu() - ref).abs().max())
    took = "the wide fp16 kernel" if colorizer.last_used_wide_f16 else "the fallback (the library declined)"
    line = "fast n=%d: %s; worst |rgb - f64| %.3e, of RgbNet.forward %.3e" % (N_CHAIN, took, err_fast, err_module)
    with capsys.disabled():
        print("\n" + line)
    _record([line])
    assert colorizer.last_used_wide_f16 in (True, False)
    if colorizer.last_used_wide_f16:
        assert err_fast <= 2.0 * err_module
    else:                                      # the fallback: the default path, whose bar is test (3)'s
        assert _same_bits(got.rgb, yard[1 << 18].rgb)
    assert colorizer.colors(points[:5]).rgb.shape == (5, 3) and colorizer.last_used_wide_f16 is None
