"""The frame renderer on the GPU (permuto_sdf_amd/render.py, csrc/frame_rays.hip, csrc/frame_composite.hip).

  * rays: bit-for-bit the rays psdf_random_rays_from_reel draws for the same pixels, and every entry within the float64 bar that
    tests/host/frame_rays_check.cpp derives (restated below);
  * foreground composite: radiance, transmittance, weight sum and normals bit-for-bit what the existing kernels give for the
    containers of oracle/composite_cases.py, written at a pixel offset with canaries around; normals also against float64;
  * background composite: bit-for-bit the existing fused forward, rgb_bg = t * pred_bg with one rounding;
  * whole frame: bit-for-bit the operator chain the tree already had, on the same rays in the same chunks; two chunkings agree to
    within twice what that chain itself moves between them;
  * rendering leaves a training run as it was; rendered views go straight into image_eval.evaluate_views.

The second chunking of the 40 x 48 frame has eight chunks, seven of 256 rays and one of 128: a chunk is a multiple of 64 rays,
and ceil(1920 / r) = 7 would need 275 <= r < 320, so no pool gives seven."""
import math
import types

import pytest
import torch

from oracle import composite_cases as cc
from oracle import composite_float64 as c64
from tests.float64_check import check, show

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
CANARY = -77.25
RATIO = 0.6                 # cos_anneal_ratio of the composite cases: both relu branches of the section point count
FIRST = 37                  # pixel offset of the composite cases
FH, FW = 13, 17             # their frame: 221 pixels, more than 37 + 160


# ================================================================================================================ rays
def _camera(dev):
    """the 41 x 53 frame of tests/host/frame_rays_check.cpp: fx != fy, cx != W / 2, the camera at distance 1.5"""
    from permuto_sdf_amd.render import Frame
    K = torch.tensor([[63.6, 0.0, 24.25], [0.0, 61.0, 21.5], [0.0, 0.0, 1.0]], dtype=torch.float64)
    c = torch.tensor([0.3, -0.5, 0.8], dtype=torch.float64)
    c = 1.5 * c / c.norm()
    z = -c / c.norm()
    x = torch.linalg.cross(torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64), z)
    x = x / x.norm()
    y = torch.linalg.cross(z, x)
    tf = torch.eye(4, dtype=torch.float64)
    tf[:3, 0], tf[:3, 1], tf[:3, 2], tf[:3, 3] = x, y, z, c
    return Frame(K.float().to(dev), tf.float().to(dev), 41, 53)


def _rays_float64(frame, first, count):
    """create_rays_from_frame in float64 (K^-1 by float64 inversion, R cam + t - t, normalise) and the bar of every entry:
    e_c = 10u A_c + 2u |t_c| on d0 (A_c = sum_j |R_cj| |pc_j|; the + t - t round trip is the 2u |t_c|), |e|_2 / |d0| + 6u on the
    direction -- the derivation is in tests/host/frame_rays_check.cpp"""
    K, T = frame.K.cpu().double(), frame.tf_world_cam.cpu().double()
    pix = torch.arange(first, first + count, dtype=torch.int64)
    p = torch.stack([(pix % frame.width).double() + 0.5, (pix // frame.width).double() + 0.5, torch.ones(count, dtype=torch.float64)], 1)
    pc = p @ torch.linalg.inv(K).t()
    R, t = T[:3, :3], T[:3, 3]
    d0 = (pc @ R.t() + t) - t
    A = pc.abs() @ R.abs().t()
    e = 10 * U * A + 2 * U * t.abs()
    n = d0.norm(dim=1, keepdim=True)
    return t.expand(count, 3), d0 / n, (e.norm(dim=1, keepdim=True) / n + 6 * U).expand(count, 3)


RANGES = [(0, 41 * 53), (50, 70), (41 * 53 - 1, 1), (0, 0)]


@pytest.mark.parametrize("first,count", RANGES)
def test_rays_are_the_training_rays_bit_for_bit_and_within_their_float64_bars(dev, first, count):
    from permuto_sdf_amd import _lib as L
    from permuto_sdf_amd import render
    frame = _camera(dev)
    H, W, pad = frame.height, frame.width, 64
    o = torch.full((count + 2 * pad, 3), CANARY, device=dev)
    d = torch.full((count + 2 * pad, 3), CANARY, device=dev)
    L.call("psdf_frame_rays", L.c_i(H), L.c_i(W), L.ptr(frame.K), L.ptr(frame.tf_world_cam), L.c_l(first), L.c_i(count),
           L.ptr(o[pad:]) if count else None, L.ptr(d[pad:]) if count else None, L.stream())
    for buf in (o, d):
        assert bool((buf[:pad] == CANARY).all()) and bool((buf[pad + count:] == CANARY).all())
    o, d = o[pad:pad + count], d[pad:pad + count]
    o2, d2 = render.frame_rays(frame, first, count)
    assert o2.shape == (count, 3) and torch.equal(o2, o) and torch.equal(d2, d)
    if count == 0:
        return
    # the kernel training draws its rays with, on a one-image reel, for the same pixels
    f = dict(dtype=torch.float32, device=dev)
    rgb = torch.zeros((1, 3, H, W), **f)
    ro, rd, gt, gm = (torch.empty((count, c), **f) for c in (3, 3, 3, 1))
    pix = torch.arange(first, first + count, dtype=torch.int32, device=dev)
    img = torch.zeros(count, dtype=torch.int32, device=dev)
    L.call("psdf_random_rays_from_reel", L.c_i(count), L.c_i(1), L.c_i(H), L.c_i(W), L.ptr(rgb), L.ptr(rgb), L.ptr(frame.K.view(1, 3, 3)),
           L.ptr(frame.tf_world_cam.view(1, 4, 4)), L.ptr(pix), L.ptr(img), L.c_i(0), L.ptr(ro), L.ptr(rd), L.ptr(gt), L.ptr(gm), L.stream())
    assert torch.equal(o, ro) and torch.equal(d, rd)
    want_o, want_d, bar = _rays_float64(frame, first, count)
    assert torch.equal(o.cpu().double(), want_o)
    out = []
    check(out, "dirs", d, want_d, bar)
    show("rays [%d, %d)" % (first, first + count), out)


# ================================================================================================ foreground composite
def make_rs(c, dev, dirs=None, dt=None):
    from permuto_sdf import RaySamplesPacked
    rs = RaySamplesPacked(c["R"], c["N"], device=dev)
    rs.ray_start_end_idx = c["start_end"].to(dev)
    if c["equal"]:
        rs.rays_have_equal_nr_of_samples, rs.fixed_nr_of_samples_per_ray = True, c["fixed"]
    if dirs is not None:
        rs.samples_dirs = dirs.to(dev)
    if dt is not None:
        rs.samples_dt = dt.to(dev).view(-1, 1).contiguous()
    rs.cur_nr_samples.fill_(min(c["N"], c["total"]))
    return rs


def _planes(dev, c):
    return torch.full((c, FH, FW), CANARY, device=dev)


def _rotation(dev):
    """a rotation that is no permutation: 50 degrees about (1, 2, 3) / sqrt(14), float64 rounded to float32"""
    a = torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64)
    a = a / a.norm()
    Kx = torch.tensor([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]], dtype=torch.float64)
    th = math.radians(50.0)
    R = torch.eye(3, dtype=torch.float64) + math.sin(th) * Kx + (1 - math.cos(th)) * (Kx @ Kx)
    return R.float().contiguous().to(dev)


def _inside(img, R):
    """[C, H, W] -> the [R, C] rows of the pixels [FIRST, FIRST + R), and a mask of the others"""
    flat = img.reshape(img.shape[0], -1)
    outside = torch.ones(flat.shape[1], dtype=torch.bool, device=img.device)
    outside[FIRST:FIRST + R] = False
    return flat[:, FIRST:FIRST + R].t().contiguous(), flat[:, outside]


@pytest.mark.parametrize("inv_s", [20.0, 64.0, 512.0])
@pytest.mark.parametrize("family", ["cross", "grazing", "noise"])
@pytest.mark.parametrize("cname", ["overflow", "cap64", "equal65", "equal256"])
def test_foreground_composite_is_the_existing_kernels_bit_for_bit_in_planes(dev, cname, family, inv_s):
    from permuto_sdf import VolumeRendering as VR
    from permuto_sdf_amd import render
    from permuto_sdf_amd.neus import neus_composite_forward_raw, normalize3
    c = cc.container(cname)
    R, N = c["R"], c["N"]
    assert FIRST + R < FH * FW
    sdf, dirs, grad, dt = cc.neus_family(c, family)
    rgb, _, _ = cc.upstream(c, "dense")
    rs = make_rs(c, dev, dirs, dt)
    inv = torch.tensor([inv_s], device=dev)
    sdf_d, grad_d, rgb_d = sdf.to(dev), grad.to(dev), rgb.to(dev)
    # the existing kernels
    pred, bg, w = neus_composite_forward_raw(rs, sdf_d, grad_d, rgb_d, inv, RATIO, want_weights=True)
    w_sum, _ = VR.sum_over_each_ray(rs, w)
    G32 = VR.integrate_with_weights(rs, grad_d, w)
    nrm = normalize3(G32)
    # the new one, into canary-filled planes at pixel 37
    rot = _rotation(dev)
    img, nimg, cimg, wimg = _planes(dev, 3), _planes(dev, 3), _planes(dev, 3), _planes(dev, 1)
    T = torch.full((R + 8,), CANARY, device=dev)
    render.frame_composite_neus_raw(rs, sdf_d, grad_d, rgb_d, inv, RATIO, FH, FW, FIRST, img, nimg, wimg, T, cimg, rot)
    got = {}
    for name, plane in (("rgb", img), ("normals", nimg), ("normals_cam", cimg), ("weights_sum", wimg)):
        got[name], outside = _inside(plane, R)
        assert bool((outside == CANARY).all()), name
    assert bool((T[R:] == CANARY).all())
    assert torch.equal(got["rgb"], pred)
    assert torch.equal(T[:R].view(-1, 1), bg)
    assert torch.equal(got["weights_sum"], w_sum)
    assert torch.equal(got["normals"], nrm)
    # without camera normals the other outputs are the same bits
    img2, nimg2, wimg2, T2 = _planes(dev, 3), _planes(dev, 3), _planes(dev, 1), torch.empty(R, device=dev)
    render.frame_composite_neus_raw(rs, sdf_d, grad_d, rgb_d, inv, RATIO, FH, FW, FIRST, img2, nimg2, wimg2, T2)
    assert torch.equal(img2, img) and torch.equal(nimg2, nimg) and torch.equal(wimg2, wimg) and torch.equal(T2, T[:R])
    # empty and overflowed rays: 0 / 0 / 0 / 1
    rays = c64.Rays(c["start_end"], N, c["equal"], c["fixed"], R)
    skipped = ~rays.valid
    if cname in ("overflow", "cap64"):
        assert int(skipped.sum()) >= 4
    sk = skipped.to(dev)
    for name in ("rgb", "normals", "normals_cam", "weights_sum"):
        assert bool((got[name][sk] == 0).all()), name
    assert bool((T[:R][sk] == 1).all())
    # normals against float64: G and its bar from the evaluator on the existing kernel's weights; no ray is excluded
    out = []
    q = c64.op_integrate(rays, grad, w)
    G, bar_G = q.val, c64.error_bar(q, c64.R_OP_INTEGRATE)
    live = rays.valid
    Gn = G.norm(dim=1, keepdim=True)
    assert float((Gn[live] / bar_G.norm(dim=1, keepdim=True)[live]).min()) > 1e3         # (2.9e3 at worst: no ill-conditioned normal)
    want = torch.where(live[:, None], G / Gn.clamp_min(1e-300), torch.zeros_like(G))
    bar = (2 * bar_G.norm(dim=1, keepdim=True) / Gn.clamp_min(1e-300) + 4 * U).expand(-1, 3)
    check(out, "normals", got["normals"], want, bar, keep=live)
    # camera normals against normalize(R n) in float64 of the kernel's own fp32 normal: three products and two sums per entry
    # (at most 4u A_c, A_c = sum_j |R_cj| |n_j|), then the normalisation as above: |e|_2 / |c| + 4u
    n64, R64 = got["normals"].cpu().double(), rot.cpu().double()
    cam = n64 @ R64.t()
    cn = cam.norm(dim=1, keepdim=True)
    e = 4 * U * (n64.abs() @ R64.abs().t())
    want_c = torch.where(live[:, None], cam / cn.clamp_min(1e-300), torch.zeros_like(cam))
    bar_c = (e.norm(dim=1, keepdim=True) / cn.clamp_min(1e-300) + 4 * U).expand(-1, 3)
    check(out, "normals_cam", got["normals_cam"], want_c, bar_c, keep=live)
    assert float((got["normals_cam"][~sk] - got["normals"][~sk]).abs().max()) > 0.1       # the rotation did rotate
    show("frame composite %s / %s / %g" % (cname, family, inv_s), out)


def test_a_container_without_samples_renders_the_empty_values_from_null_pointers(dev):
    from permuto_sdf_amd import _lib as L
    c = cc.container("cap64")
    R = c["R"]
    se = c["start_end"].to(dev)
    inv = torch.tensor([64.0], device=dev)
    for equal, fixed in ((0, 0), (1, 64), (1, 0)):
        img, nimg, cimg, wimg = _planes(dev, 3), _planes(dev, 3), _planes(dev, 3), _planes(dev, 1)
        T = torch.full((R + 8,), CANARY, device=dev)
        L.call("psdf_frame_composite_neus", L.c_i(R), L.ptr(se), L.c_i(equal), L.c_i(fixed), L.c_i(0), None, None, None, None, None,
               L.ptr(inv), L.c_f(RATIO), L.ptr(_rotation(dev)), L.c_i(FH), L.c_i(FW), L.c_l(FIRST), L.ptr(img), L.ptr(nimg), L.ptr(cimg),
               L.ptr(wimg), L.ptr(T), L.stream())
        for plane in (img, nimg, cimg, wimg):
            inside, outside = _inside(plane, R)
            assert bool((inside == 0).all()) and bool((outside == CANARY).all())
        assert bool((T[:R] == 1).all()) and bool((T[R:] == CANARY).all())


# ================================================================================================ background composite
def test_background_composite_is_the_existing_forward_bit_for_bit_in_planes(dev):
    from permuto_sdf_amd import render
    from permuto_sdf_amd.neus import nerf_composite_forward_raw
    c = cc.container("equal32")
    R = c["R"]
    raw, dt = cc.nerf_family(c)
    rgb, _, _ = cc.upstream(c, "dense")
    rs = make_rs(c, dev, None, dt)
    g = torch.Generator().manual_seed(7)
    fg, t = torch.rand(R, 3, generator=g).to(dev), torch.rand(R, 1, generator=g).to(dev)
    t[::9] = 1.0
    t[4::9] = 0.0
    raw_d, rgb_d = raw.to(dev), rgb.to(dev)
    pred_bg, pred = nerf_composite_forward_raw(rs, raw_d, rgb_d, fg, t)
    img, bimg = _planes(dev, 3), _planes(dev, 3)
    img.view(3, -1)[:, FIRST:FIRST + R] = fg.t()
    T = t.view(-1).contiguous()
    render.frame_composite_nerf_raw(rs, raw_d, rgb_d, T, FH, FW, FIRST, img, bimg)
    got, outside = _inside(img, R)
    got_bg, outside_bg = _inside(bimg, R)
    assert bool((outside == CANARY).all()) and bool((outside_bg == CANARY).all())
    assert torch.equal(got, pred)
    assert torch.equal(got_bg, t * pred_bg)              # one fp32 product: one rounding
    assert float(pred_bg.abs().max()) > 0.1 and torch.equal(T, t.view(-1))


# ========================================================================================================= whole frame
H, W = 40, 48
POOL_CHUNKED = 64 * 256         # 256 rays per chunk: seven chunks of 256 and one of 128


@pytest.fixture(scope="module")
def trained(dev):
    """a trainer past its sphere fit: 60 iterations of it, 8 of the main phase (one occupancy refresh)"""
    from permuto_sdf_amd.train_step import HyperParams, SyntheticReel, Trainer
    hp = HyperParams()
    hp.nr_iter_sphere_fit = 60
    reel = SyntheticReel(dev, nr_images=4, height=H, width=W)
    tr = Trainer(dev, hp=hp, reference_schedule=True, nr_images=4)
    for _ in range(60 + 8):
        tr.step(reel)
    torch.cuda.synchronize()
    return tr, reel


def _yardstick(tr, frame, pool, with_mask=False):
    """the operator chain the tree already had, on the same rays in the same chunks: _samples, sdf_and_gradient, the colour net,
    neus_weights + _Integrate, normalize3, the background chain, cat and transposes -> rgb, rgb_bg, normals, weights_sum"""
    from permuto_sdf_amd import render
    from permuto_sdf_amd.neus import normalize3
    from permuto_sdf_amd.train_step import BgNet, _Integrate
    hp, dev = tr.hp, tr.dev
    plan = render.FramePlan(frame.height, frame.width, hp.max_nr_samples_per_ray, pool)
    keep_inv_s, keep_pool = tr.rgb.last_inv_s, tr.grid.max_nr_samples
    tr.grid.max_nr_samples = pool
    rows = {k: [] for k in ("rgb", "rgb_bg", "normals", "weights_sum")}
    with torch.no_grad():
        for first, count in plan.chunks():
            o, d = render.frame_rays(frame, first, count)
            fg, bg = tr._samples(o, d, 9999999, jitter=False)
            if fg.samples_pos.shape[0] == 0:
                pred, nrm = torch.zeros(count, 3, device=dev), torch.zeros(count, 3, device=dev)
                w_sum, bgT = torch.zeros(count, 1, device=dev), torch.ones(count, 1, device=dev)
            else:
                sdf, grad, feat = tr.sdf.sdf_and_gradient(fg.samples_pos, 9999999)
                sdf, grad, feat = sdf.detach(), grad.detach(), feat.detach()
                rgb = tr.rgb(fg.samples_pos, fg.samples_dirs, grad, feat)
                w, w_sum, bgT = tr.rgb.neus_weights(fg, sdf, grad, 1.0, hp.forced_variance_finish)
                pred = _Integrate.apply(fg, rgb, w)
                nrm = normalize3(_Integrate.apply(fg, grad, w))
            if not with_mask:
                rgb_bg, dens = tr.bg(bg.samples_pos_4d, bg.samples_dirs)
                pred_bg = bgT.view(-1, 1) * _Integrate.apply(bg, rgb_bg, BgNet.nerf_weights(bg, dens.view(-1, 1)))
                pred = pred + pred_bg
                rows["rgb_bg"].append(pred_bg)
            rows["rgb"].append(pred)
            rows["normals"].append(nrm)
            rows["weights_sum"].append(w_sum)
    tr.rgb.last_inv_s, tr.grid.max_nr_samples = keep_inv_s, keep_pool
    return {k: torch.cat(v, 0).t().reshape(-1, frame.height, frame.width).contiguous() if v else None for k, v in rows.items()}


def _moved(a, b):
    return max(float((a[k] - b[k]).abs().max()) for k in ("rgb", "normals", "weights_sum") if a[k] is not None)


def test_whole_frame_is_the_operator_chain_bit_for_bit_in_two_chunkings(dev, trained):
    from permuto_sdf_amd import render
    tr, reel = trained
    frame = render.Frame.from_reel(reel, 1)
    assert (frame.height, frame.width) == (H, W)
    rnd = render.FrameRenderer(tr)
    got, yard = {}, {}
    for pool, chunks in ((render.OccupancyGrid.POOL, 1), (POOL_CHUNKED, 8)):
        plan = render.FramePlan(H, W, tr.hp.max_nr_samples_per_ray, pool)
        assert plan.nr_chunks == chunks and (chunks == 1 or plan.last_chunk != plan.rays_per_chunk)
        out = rnd.render(frame, pool_samples=pool)
        got[chunks] = dict(rgb=out.rgb, rgb_bg=out.rgb_bg, normals=out.normals, weights_sum=out.weights_sum)
        yard[chunks] = _yardstick(tr, frame, pool)
        assert out.normals_cam is None
        for k, v in got[chunks].items():
            assert v.dtype == torch.float32 and v.is_cuda and v.shape == ((1 if k == "weights_sum" else 3), H, W), k
        if chunks == 1:       # the scene is not trivial
            ws = out.weights_sum
            print("weights_sum: %.1f%% of the pixels above 0.5, %.1f%% below 0.01" % (100 * float((ws > 0.5).float().mean()),
                                                                                  100 * float((ws < 0.01).float().mean())))
            assert int((ws > 0.5).sum()) > 0 and int((ws < 0.01).sum()) > 0
        for k in ("rgb", "rgb_bg", "normals", "weights_sum"):
            assert bool(torch.isfinite(got[chunks][k]).all()), k
            assert torch.equal(got[chunks][k], yard[chunks][k]), (chunks, k, float((got[chunks][k] - yard[chunks][k]).abs().max()))
    # two chunkings need not agree to the bit (the MLP dispatch picks kernel forms by batch size): the operator chain sets the bar
    d_code, d_yard = _moved(got[1], got[8]), _moved(yard[1], yard[8])
    print("one chunk against eight: the renderer moves by %.3e, the operator chain by %.3e" % (d_code, d_yard))
    assert d_code <= 2 * d_yard
    # camera normals: the same other planes, and the world normals rotated by the rotation of tf_cam_world
    cam = rnd.render(frame, camera_normals=True)
    assert torch.equal(cam.rgb, got[1]["rgb"]) and torch.equal(cam.normals, got[1]["normals"])
    Rcw = frame.tf_world_cam[:3, :3].t().double()
    hit = (cam.normals.abs().sum(0) > 0).reshape(-1).cpu()
    assert bool((cam.normals_cam.reshape(3, -1)[:, ~hit.to(dev)] == 0).all())
    # the bar of the composite test: three products and two sums per entry (4u A_c), then the normalisation: |e|_2 / |c| + 4u
    n64, R64 = cam.normals.double().reshape(3, -1).t().cpu(), Rcw.cpu()
    c = n64 @ R64.t()
    cn = c.norm(dim=1, keepdim=True)
    e = 4 * U * (n64.abs() @ R64.abs().t())
    want = torch.where(hit[:, None], c / cn.clamp_min(1e-300), torch.zeros_like(c))
    bar = (e.norm(dim=1, keepdim=True) / cn.clamp_min(1e-300) + 4 * U).expand(-1, 3)
    out = []
    check(out, "normals_cam", cam.normals_cam.reshape(3, -1).t().contiguous(), want, bar, keep=hit)
    show("whole frame", out)
    # a frame on another device than the models is refused before any launch
    from permuto_sdf_amd._lib import PsdfError
    with pytest.raises(PsdfError):
        rnd.render(render.Frame(frame.K.cpu(), frame.tf_world_cam.cpu(), H, W))


def test_with_mask_renders_the_foreground_alone(dev, trained):
    from permuto_sdf_amd import render
    tr, reel = trained
    frame = render.Frame.from_reel(reel, 2)
    holder = types.SimpleNamespace(sdf=tr.sdf, rgb=tr.rgb, bg=tr.bg, grid=tr.grid, sphere=tr.sphere, hp=tr.hp, with_mask=True)
    out = render.FrameRenderer(holder).render(frame, pool_samples=POOL_CHUNKED)
    assert out.rgb_bg is None
    keep = tr.with_mask
    tr.with_mask = True           # (the trainer's sampling path then makes no background samples)
    try:
        yard = _yardstick(tr, frame, POOL_CHUNKED, with_mask=True)
    finally:
        tr.with_mask = keep
    assert yard["rgb_bg"] is None
    for k in ("rgb", "normals", "weights_sum"):
        assert torch.equal(getattr(out, k), yard[k]), k
    full = render.FrameRenderer(tr).render(frame, pool_samples=POOL_CHUNKED)
    assert torch.equal(full.weights_sum, out.weights_sum) and not torch.equal(full.rgb, out.rgb)


def test_rendering_leaves_a_training_run_as_it_was(dev, trained):
    from permuto_sdf_amd import render
    tr, reel = trained
    lattices = [m.encoding.lattice_values for m in (tr.sdf, tr.rgb, tr.bg)]
    dense = [p for p in tr.params if not any(p is l for l in lattices)]
    assert tr.rgb.last_inv_s is not None and any(p.grad is not None for p in dense)

    def snapshot():
        torch.cuda.synchronize()
        return dict(dense=[p.detach().clone() for p in dense],
                    lattices=[(int(l.detach().view(torch.int32).sum(dtype=torch.int64)), float(l.detach().double().abs().sum())) for l in lattices],
                    grads=[None if p.grad is None else p.grad.detach().clone() for p in tr.params],
                    grad_ids=[None if p.grad is None else id(p.grad) for p in tr.params],
                    it=tr.iter, nr_rays=tr.nr_rays, inv_s=tr.rgb.last_inv_s.clone(), inv_s_id=id(tr.rgb.last_inv_s),
                    rng=torch.cuda.get_rng_state(dev), pool=tr.grid.max_nr_samples,
                    modes=[m.training for m in (tr.sdf, tr.rgb, tr.bg)])

    before = snapshot()
    out = render.FrameRenderer(tr).render(render.Frame.from_reel(reel, 0), pool_samples=POOL_CHUNKED, camera_normals=True)
    assert bool(torch.isfinite(out.rgb).all())
    after = snapshot()
    assert all(torch.equal(a, b) for a, b in zip(before["dense"], after["dense"]))
    assert before["lattices"] == after["lattices"]
    assert before["grad_ids"] == after["grad_ids"]
    assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(before["grads"], after["grads"]))
    assert (before["it"], before["nr_rays"], before["pool"], before["modes"]) == (after["it"], after["nr_rays"], after["pool"], after["modes"])
    assert before["inv_s_id"] == after["inv_s_id"] and torch.equal(before["inv_s"], after["inv_s"])
    assert torch.equal(before["rng"], after["rng"])
    # and the run goes on
    loss = tr.step(reel)
    assert math.isfinite(float(loss))


def test_rendered_views_go_straight_into_the_scores(dev, trained):
    from permuto_sdf_amd import image_eval, render
    tr, reel = trained
    rnd = render.FrameRenderer(tr)
    views = rnd.render_views([render.Frame.from_reel(reel, i) for i in (0, 3)])
    assert views.shape == (2, 3, H, W) and views.dtype == torch.float32 and views.is_cuda
    assert float(views.min()) >= 0.0 and float(views.max()) <= 1.0 and not torch.equal(views[0], views[1])
    psnr, ssim = image_eval.evaluate_views(views, views)
    assert psnr.shape == (2,) and ssim.shape == (2,)
    assert float((psnr - 80.0).abs().max()) <= 1e-9 and float((ssim - 1.0).abs().max()) <= 1e-9
    with pytest.raises(ValueError):
        rnd.render_views([])


def test_a_checkpoint_renders_what_its_trainer_renders(dev, trained, tmp_path):
    from permuto_sdf_amd import render
    tr, reel = trained
    frame = render.Frame.from_reel(reel, 1)
    tr.sync_parameters()
    tr.save_checkpoint(str(tmp_path))
    a = render.FrameRenderer(tr).render(frame)
    b = render.FrameRenderer.from_checkpoint(str(tmp_path), dev).render(frame)
    for k in ("rgb", "rgb_bg", "normals", "weights_sum"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
