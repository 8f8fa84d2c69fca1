"""GPU: grid-free sphere tracing in a box (permuto_sdf_amd/box_trace.py, csrc/box_trace.hip) on small fitted 3-D and 4-D SDF
nets, against a line-by-line restatement, in this test, of the reference's `occupancy_grid=None` loop
(permuto_sdf_py/utils/sdf_utils.py:120-218) with boolean-mask compaction over `Box.ray_intersection` and the product's own
forward -- same kernels per point, so end points, flags and SDF must be bit-identical on the rays that hit the box; against a
float32 numpy replay of the loop fed the SDF values the GPU used; the normals against autograd; the traced surface against the
analytic one; graph replay against eager; and whole frames against the restated chain of
experiments/visualization/vis_4d_sdf.py:105-118."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
R_RAYS = 4099
T_VAL = 0.37
CAMERA = (0.2, -0.3, -1.6)


def centre(t):
    """c(t) of the moving sphere |x - c(t)| - 0.25"""
    return 0.2 * (t - 0.5)


def fit_sdf(dev, P, iters=300):
    """the recipe of fit_sphere_sdf (tests/test_gpu_sphere_trace.py): a small encoded SDF fitted to |x| - 0.3 inside the unit
    cube (P = 3), or to |x - c(t)| - 0.25, c(t) = (0.2 (t - 0.5), 0, 0), t in [0, 1) (P = 4)"""
    from permuto_sdf_amd import FusedMLP, PermutoEncoding
    from permuto_sdf_amd.optim import FusedAdamW
    torch.manual_seed(0)
    enc = PermutoEncoding(P, 2 ** 16, 8, 2, np.geomspace(1.0, 0.02, 8), concat_points=True, concat_points_scaling=1.0,
                          init_scale=1e-3).to(dev)
    mlp = FusedMLP([enc.output_dims(), 64, 64, 64, 1]).to(dev)
    opt = FusedAdamW(list(enc.parameters())[:1] + list(mlp.parameters()), lr=5e-3)
    win = torch.ones(8, device=dev)
    for _ in range(iters):
        x = torch.rand(16384, P, device=dev)
        x[:, :3] -= 0.5
        loss = ((mlp(enc(x, win)) - analytic(x)) ** 2).mean()
        for p in opt.param_groups[0]["params"]:
            p.grad = None
        loss.backward()
        opt.step()
    loss = float(loss.detach())
    print("fitted the %d-D net: loss %.2e" % (P, loss))
    return types.SimpleNamespace(enc=enc, mlp=mlp, win=win, loss=loss, P=P, encoding=enc, mlp_sdf=mlp, window=lambda it: win)


def analytic(x):
    """[N, 1]: the field a net of fit_sdf was fitted to, at points [N, 3] (the still sphere) or [N, 4]"""
    if x.shape[1] == 3:
        return x.norm(dim=1, keepdim=True) - 0.3
    c = torch.zeros_like(x[:, :3])
    c[:, 0] = 0.2 * (x[:, 3] - 0.5)
    return (x[:, :3] - c).norm(dim=1, keepdim=True) - 0.25


@pytest.fixture(scope="module")
def net3(dev):
    return fit_sdf(dev, 3)


@pytest.fixture(scope="module")
def net4(dev):
    return fit_sdf(dev, 4)


@pytest.fixture(scope="module")
def unit_box():
    from permuto_sdf_amd.box_trace import Box
    return Box([1.0, 1.0, 1.0], [0.0, 0.0, 0.0])


def fan(R, dev, camera=CAMERA, spread=0.9, seed=3):
    """R rays from one camera outside the unit box towards targets spread over [-spread, spread]^2 x [-0.3, 0.3]: wide enough
    that some miss the box; R = 1 is the ray through the centre"""
    rng = np.random.default_rng(seed)
    o = np.tile(np.asarray(camera, np.float32), (R, 1))
    target = np.concatenate([rng.uniform(-spread, spread, (R, 2)), rng.uniform(-0.3, 0.3, (R, 1))], 1).astype(np.float32)
    if R == 1:
        target[:] = 0.0
    d = target - o
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    return torch.from_numpy(np.ascontiguousarray(o)).to(dev), torch.from_numpy(np.ascontiguousarray(d)).to(dev)


def with_time(p, time_val):
    """sdf_utils.py:160-164 / :189-192: the time appended as a column"""
    if time_val is None:
        return p
    time_tensor = torch.empty((p.shape[0], 1), device=p.device)
    time_tensor.fill_(time_val)
    return torch.cat([p, time_tensor], 1)


def reference_style_trace(n_iter, o, d, sdf_fn, mult, thr, box, time_val=None):
    """restatement of sdf_utils.sphere_trace, the branch without an occupancy grid, with boolean-mask compaction
    -> (pts, final sdf, converged, hit)"""
    pe, te, px, tx, hit = box.ray_intersection(o, d)                   # :122
    pos, dirs = pe, d                                                   # :136-141: one sample per ray at the entry point
    pts = pos.clone()
    conv = torch.zeros_like(pos)[:, 0:1].bool()
    for _ in range(n_iter):
        sel = torch.logical_not(conv)
        pu = pts[sel.repeat(1, 3)].view(-1, 3)
        du = dirs[sel.repeat(1, 3)].view(-1, 3)
        if pu.shape[0] == 0:
            break
        sdf = sdf_fn(with_time(pu, time_val))
        pu = pu + du * sdf * mult
        newly = sdf.abs() < thr
        conv[sel] = torch.logical_or(conv[sel], newly.view(-1))
        conv = conv.view(-1, 1)
        within = box.check_point_inside_primitive(pu)
        conv[sel] = torch.logical_or(conv[sel], torch.logical_not(within.view(-1)))
        conv = conv.view(-1, 1)
        pts[sel.repeat(1, 3)] = pu.view(-1)
    return pts, sdf_fn(with_time(pts, time_val)), conv, hit.view(-1)


def forward_of(net):
    def sdf_fn(p):
        with torch.no_grad():
            return net.mlp(net.enc(p.contiguous(), net.win))
    return sdf_fn


def classes(box, pts, sdf, conv, miss, thr):
    inside = box.check_point_inside_primitive(pts).view(-1)
    hit = ~miss
    on_surface = hit & conv.view(-1) & inside & (sdf.view(-1).abs() < thr)
    left = hit & ~inside
    return {"hit": int(hit.sum()), "miss": int(miss.sum()), "converged on the surface": int(on_surface.sum()),
            "left the box": int(left.sum())}


def check_against_the_loop(net, box, R, dev, time_val):
    from permuto_sdf_amd.box_trace import BoxTracer
    n_iter, mult, thr = 20, 0.9, 2e-4
    o, d = fan(R, dev)
    ref_pts, ref_sdf, ref_conv, hit = reference_style_trace(n_iter, o, d, forward_of(net), mult, thr, box, time_val)
    tracer = BoxTracer(net.enc, net.mlp, box, net.win)
    pts, sdf, grads, conv = tracer.trace(o, d, n_iter, mult, thr, time_val=time_val, return_gradients=True)
    assert pts.shape == (R, 3) and sdf.shape == (R, 1) and grads.shape == (R, 3) and conv.shape == (R, 1) and conv.dtype == torch.bool
    miss = tracer.no_hit
    assert torch.equal(miss, ~hit)
    assert torch.equal(pts[hit], ref_pts[hit]) and torch.equal(conv[hit], ref_conv[hit]) and torch.equal(sdf[hit], ref_sdf[hit])
    # rays that miss the box: as SphereTracer reports rays that met no occupancy
    assert torch.equal(pts[miss], o[miss]) and bool((sdf[miss] == 0).all()) and bool((grads[miss] == 0).all()) and bool(conv[miss].all())
    sizes = classes(box, pts, sdf, conv, miss, thr)
    print("R = %d, %d-D: %s" % (R, net.P, sizes))
    if R > 1:
        assert all(v > 0 for v in sizes.values()), sizes
    else:
        assert sizes["hit"] == 1
    return tracer, (o, d), (pts, sdf, grads, conv)


@pytest.mark.parametrize("R", [R_RAYS, 1])
def test_trace_equals_the_references_loop_bit_for_bit_3d(dev, net3, unit_box, R):
    assert net3.loss < 1e-4
    check_against_the_loop(net3, unit_box, R, dev, None)


@pytest.mark.parametrize("R", [R_RAYS, 1])
def test_trace_equals_the_references_loop_bit_for_bit_4d(dev, net4, unit_box, R):
    check_against_the_loop(net4, unit_box, R, dev, T_VAL)


def _numpy_intersection(box, o, d):
    """aabb.py:47-100 in float32 numpy, where by where"""
    f32 = np.float32
    bb_min, bb_max = box.bb_min.astype(f32), box.bb_max.astype(f32)
    lo = -np.ones((len(o), 1), f32) * f32(1e10)
    hi = np.ones((len(o), 1), f32) * f32(1e10)
    invalid = np.zeros((len(o), 1), bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(3):
            dim_lo = ((bb_min[i] - o[:, i]) / d[:, i]).astype(f32)[:, None]
            dim_hi = ((bb_max[i] - o[:, i]) / d[:, i]).astype(f32)[:, None]
            swap = dim_lo > dim_hi
            dim_lo, dim_hi = np.where(swap, dim_hi, dim_lo), np.where(swap, dim_lo, dim_hi)
            invalid = invalid | (dim_hi < lo) | (dim_lo > hi)
            lo = np.where(dim_lo > lo, dim_lo, lo)
            hi = np.where(dim_hi < hi, dim_hi, hi)
    lo = np.where(invalid, f32(0), lo)
    lo = np.where(lo < 0, f32(0), lo)
    return (o + (lo * d).astype(f32)).astype(f32), ~invalid.reshape(-1)


@pytest.mark.parametrize("P", [3, 4])
def test_launch_sequence_against_a_float32_replay_fed_the_recorded_sdf(dev, net3, net4, unit_box, P):
    """the fused launch sequence -- psdf_box_trace_begin, psdf_box_trace_step under the per-ray mask -- with `_sdf` replaced by
    an analytic field and recorded; the reference's loop replayed in float32 numpy, in its operation order, fed the very values
    the GPU used: end points and flags bit-exact"""
    from permuto_sdf_amd.box_trace import BoxTracer
    net, box = (net3 if P == 3 else net4), unit_box
    time_val = None if P == 3 else T_VAL

    def field(p):
        return p[:, :3].norm(dim=1, keepdim=True) - 0.3 + 0.01 * torch.sin(40 * p[:, 0:1])

    class Recording(BoxTracer):
        def _sdf(self, pts, dims, packed, skip=None, out=None, feat_buf=None):
            assert pts.shape[1] == P and (P == 3 or bool((pts[:, 3] == float(np.float32(T_VAL))).all()))
            s = field(pts).view(1, -1)
            if out is None:
                out = s.clone()
            elif skip is None:
                out.copy_(s)
            else:
                out.copy_(torch.where(skip.view(1, -1).bool(), out, s))
            self.recorded.append((out.clone(), None if skip is None else skip.clone().bool()))
            return None, out

    tracer = Recording(net.enc, net.mlp, box, net.win)
    tracer.recorded = []
    n_iter, mult, thr = 15, 0.9, 2e-4
    o, d = fan(R_RAYS, dev, seed=12)
    pts, sdf, _, conv = tracer.trace(o, d, n_iter, mult, thr, time_val=time_val, return_gradients=False)
    assert len(tracer.recorded) == n_iter + 1
    rec = [(s.cpu().numpy().reshape(-1), k.cpu().numpy().reshape(-1)) for s, k in tracer.recorded]
    f32 = np.float32
    on, dn = o.cpu().numpy(), d.cpu().numpy()
    entry, hit = _numpy_intersection(box, on, dn)
    ids = np.nonzero(hit)[0]
    ref_pts, dirs = entry[ids].copy(), dn[ids]
    ref_conv = np.zeros(len(ids), bool)
    tr, half = np.asarray(box.translation, f32), box.half.astype(f32)
    for it in range(n_iter):
        sel = ~ref_conv
        if not sel.any():
            break
        vals, skip = rec[it]
        assert not skip[ids[sel]].any()                    # the rays the CPU still traces are the ones the GPU evaluated
        s = vals[ids[sel]].astype(f32).reshape(-1, 1)
        pu = (ref_pts[sel] + ((dirs[sel] * s).astype(f32) * f32(mult)).astype(f32)).astype(f32)
        newly = (np.abs(s) < f32(thr)).reshape(-1)
        q = (pu - tr).astype(f32)
        within = ((q < half) & (q > -half)).sum(-1) == 3
        ref_pts[sel] = pu
        ref_conv[sel] = newly | ~within
    got, got_conv = pts.cpu().numpy(), conv.cpu().numpy().reshape(-1)
    assert 1000 < len(ids) < R_RAYS - 100
    assert np.array_equal(got[ids].view(np.uint32), ref_pts.view(np.uint32))          # bit-exact end points
    assert np.array_equal(got_conv[ids], ref_conv) and 0 < ref_conv.sum() <= len(ids)
    miss = np.setdiff1d(np.arange(R_RAYS), ids)
    assert np.array_equal(miss, np.nonzero(tracer.no_hit.cpu().numpy())[0])
    assert np.array_equal(got[miss], on[miss]) and got_conv[miss].all()                # untouched, reported converged
    assert bool((sdf.view(-1)[tracer.no_hit] == 0).all())


@pytest.mark.parametrize("P", [3, 4])
def test_normals_are_autograds_gradient_at_the_end_points(dev, net3, net4, unit_box, P):
    """reference: get_sdf_and_gradient on the end points with their time column, the first three columns (sdf_utils.py:199-204)"""
    from permuto_sdf_amd.box_trace import BoxTracer
    net = net3 if P == 3 else net4
    time_val = None if P == 3 else T_VAL
    tracer = BoxTracer(net.enc, net.mlp, unit_box, net.win)
    o, d = fan(R_RAYS, dev)
    pts, sdf, grads, conv = tracer.trace(o, d, 20, 0.9, 2e-4, time_val=time_val)
    hit = ~tracer.no_hit
    q = with_time(pts[hit], time_val).clone().requires_grad_(True)
    s = net.mlp(net.enc(q, net.win))
    (ga,) = torch.autograd.grad(s, q, torch.ones_like(s))
    assert ga.shape[1] == P and int(hit.sum()) > 1000
    err, bar = float((ga[:, :3] - grads[hit]).abs().max()), 1e-4 * max(1.0, float(ga.abs().max()))
    print("%d-D: max |normal - autograd| = %.3e, bar %.3e" % (P, err, bar))
    assert err < bar
    assert torch.equal(s.detach(), sdf[hit])


def test_traced_surface_is_the_moving_sphere(dev, net4, unit_box):
    """Covered here: the rays whose final |sdf| is below the convergence threshold.  At such an end point |net| < thresh, so
    |analytic| <= thresh + E with E = max |net - analytic| over the box at that time, measured here on 2^16 random points with
    the existing operators; and the mean x of those points follows the centre, c(0.9) - c(0.1) = 0.2 * 0.8, within 2 (thresh + E).
    A far camera on the axis of symmetry: the covered cap is seen nearly orthographically at both times."""
    from permuto_sdf_amd.box_trace import BoxTracer
    n_iter, mult, thr = 40, 0.9, 2e-3
    tracer = BoxTracer(net4.enc, net4.mlp, unit_box, net4.win)
    o, d = fan(R_RAYS, dev, camera=(0.0, 0.0, -8.0), spread=0.6, seed=7)
    mean_x, tol = {}, {}
    gen = torch.Generator(device=dev).manual_seed(11)
    for t in (0.1, 0.9):
        x = with_time(unit_box.rand_points_inside(2 ** 16, device=dev, generator=gen), t)
        E = float((forward_of(net4)(x) - analytic(x)).abs().max())
        pts, sdf, _, conv = tracer.trace(o, d, n_iter, mult, thr, time_val=t, return_gradients=False)
        covered = ~tracer.no_hit & (sdf.view(-1).abs() < thr)
        assert int(covered.sum()) > 200 and bool((sdf.view(-1)[covered] < 0.01).all())
        worst = float(analytic(with_time(pts[covered], t)).abs().max())
        mean_x[t], tol[t] = float(pts[covered, 0].double().mean()), thr + E
        print("t = %.1f: %d covered, E = %.3e, max |analytic sdf| at the end points %.3e (bar %.3e), mean x %.4f (centre %.4f)"
              % (t, int(covered.sum()), E, worst, thr + E, mean_x[t], centre(t)))
        assert worst <= thr + E
    moved = mean_x[0.9] - mean_x[0.1]
    print("mean x moved by %.4f, expected %.4f within %.4f" % (moved, 0.2 * 0.8, 2 * max(tol.values())))
    assert abs(moved - 0.2 * 0.8) <= 2 * max(tol.values())


def test_graph_replay_at_another_time_equals_the_eager_trace(dev, net4, unit_box):
    from permuto_sdf_amd.box_trace import BoxTracer
    t0, t1, kw = 0.25, 0.6, dict(nr_sphere_traces=20, sdf_multiplier=0.9, sdf_converged_tresh=2e-4)
    o, d = fan(R_RAYS, dev)
    tracer = BoxTracer(net4.enc, net4.mlp, unit_box, net4.win)
    first = [x.clone() for x in tracer.capture(o.clone(), d.clone(), time_val=t0, **kw)]
    out = tracer.replay(t1)
    replayed = [x.clone() for x in out] + [tracer.no_hit.clone()]
    eager_tracer = BoxTracer(net4.enc, net4.mlp, unit_box, net4.win)
    eager = list(eager_tracer.trace(o, d, time_val=t1, **kw)) + [eager_tracer.no_hit]
    for name, a, b in zip(("pts", "sdf", "grads", "conv", "no_hit"), replayed, eager):
        assert torch.equal(a, b), name
    assert not torch.equal(replayed[0], first[0])                       # the time did change the trace
    again = tracer.replay(t0)
    assert all(x is y for x, y in zip(again, out))                      # the same output tensors every time
    for name, a, b in zip(("pts", "sdf", "grads", "conv"), again, first):
        assert torch.equal(a, b), name
    eager0 = eager_tracer.trace(o, d, time_val=t0, **kw)
    assert all(torch.equal(a, b) for a, b in zip(first, eager0))
    # a 4-D field is captured at a time
    with pytest.raises(ValueError):
        tracer.capture(o, d, **kw)


def _frame(dev, H=41, W=53):
    from permuto_sdf_amd import render
    K = torch.tensor([[60.0, 0.0, W / 2], [0.0, 60.0, H / 2], [0.0, 0.0, 1.0]])
    tf = torch.eye(4)
    tf[:3, 3] = torch.tensor([0.1, -0.05, -1.6])
    return render.Frame(K.to(dev), tf.to(dev), H, W)


@pytest.mark.parametrize("P", [3, 4])
def test_frame_planes_against_the_restated_chain_and_the_player(dev, net3, net4, unit_box, P):
    from permuto_sdf_amd import render
    from permuto_sdf_amd.box_trace import BoxPlayer, BoxTracer, render_box_traced
    net, box = (net3 if P == 3 else net4), unit_box
    times = (None, None) if P == 3 else (0.3, 0.8)
    frame = _frame(dev)
    H, W = frame.height, frame.width
    kw = dict(nr_sphere_traces=40, sdf_multiplier=0.3, sdf_converged_tresh=2e-3, coverage_tresh=0.01)     # vis_4d_sdf.py:105-106
    whole = render_box_traced(net, box, frame, time_val=times[0], camera_normals=True, **kw)
    chunked = render_box_traced(net, box, frame, time_val=times[0], camera_normals=True, max_rays_per_chunk=512, **kw)
    assert render.FramePlan(H, W, 1, 512).nr_chunks == 5
    for name in ("normals", "normals_cam", "weights_sum", "depth"):
        a, b = getattr(whole, name), getattr(chunked, name)
        assert a.shape == ((1 if name in ("weights_sum", "depth") else 3), H, W) and torch.equal(a, b), name
    # vis_4d_sdf.py:105-118: trace, filter_unconverged_points, F.normalize, the image and its alpha; index-put into zero planes
    o, d = render.frame_rays(frame)
    tracer = BoxTracer(net.enc, net.mlp, box, net.win)
    ray_end, ray_end_sdf, ray_end_gradient, _ = tracer.trace(o, d, 40, 0.3, 2e-3, time_val=times[0], return_gradients=True)
    is_converged = (ray_end_sdf < 0.01).view(-1) & ~tracer.no_hit        # (rays that miss the box: the stated deviation)
    idx = torch.nonzero(is_converged).view(-1)
    n_cov = int(idx.numel())
    print("%d-D frame: %d of %d rays covered, %d miss the box" % (P, n_cov, H * W, int(tracer.no_hit.sum())))
    assert 100 < n_cov < H * W - 100 and int(tracer.no_hit.sum()) > 0
    weights = torch.zeros(H * W, device=dev)
    weights[idx] = 1.0
    q = ray_end[idx] - o[idx]
    depth = torch.zeros(H * W, device=dev)
    depth[idx] = (q[:, 0] * d[idx, 0] + q[:, 1] * d[idx, 1]) + q[:, 2] * d[idx, 2]
    assert torch.equal(whole.weights_sum.view(-1), weights) and torch.equal(whole.depth.view(-1), depth)
    # normals per entry against float64 of the chain's gradient at 4u (torch's own normalisation may differ in bits)
    g64 = ray_end_gradient[idx].double()
    want = g64 / g64.norm(dim=1, keepdim=True).clamp_min(float(np.float32(1e-12)))
    got = whole.normals.view(3, -1).t()
    err = float((got[idx].double() - want).abs().max())
    print("normals: worst error %.3f of the 4u bar" % (err / (4 * U)))
    assert err <= 4 * U
    rest = torch.ones(H * W, dtype=torch.bool, device=dev)
    rest[idx] = False
    assert bool((got[rest] == 0).all()) and bool((whole.normals_cam.view(3, -1).t()[rest] == 0).all())
    # camera-frame normals: normalize(R n) of the plane's own normal, the bar of tests/test_gpu_frame_trace.py
    R64, n64 = frame.rot_cam_world().double(), got[idx].double()
    c = n64 @ R64.t()
    cn = c.norm(dim=1, keepdim=True)
    bar = ((4 * U * (n64.abs() @ R64.abs().t())).norm(dim=1, keepdim=True) / cn.clamp_min(1e-300) + 4 * U).expand(-1, 3)
    assert bool(((whole.normals_cam.view(3, -1).t()[idx].double() - c / cn.clamp_min(1e-300)).abs() <= bar).all())
    # the player: one fill and one replay per frame
    player = BoxPlayer(net, box, frame, camera_normals=True, **kw)
    for t in times:
        eager = render_box_traced(net, box, frame, time_val=t, camera_normals=True, **kw)
        played = player.frame_at(t) if P == 4 else player.frame_at()
        for name in ("normals", "normals_cam", "weights_sum", "depth"):
            assert torch.equal(getattr(played, name), getattr(eager, name)), (name, t)
    if P == 4:
        assert not torch.equal(render_box_traced(net, box, frame, time_val=times[0], **kw).depth, played.depth)


def test_refusals(dev, net3, net4, unit_box):
    from permuto_sdf_amd._lib import PsdfError
    from permuto_sdf_amd.box_trace import BoxPlayer, BoxTracer, render_box_traced
    o, d = fan(64, dev)
    with pytest.raises(ValueError):
        BoxTracer(net4.enc, net4.mlp, unit_box, net4.win).trace(o, d)
    with pytest.raises(ValueError):
        BoxTracer(net3.enc, net3.mlp, unit_box, net3.win).trace(o, d, time_val=0.5)
    with pytest.raises(PsdfError):
        BoxTracer(net3.enc, net3.mlp, unit_box, net3.win).trace(o.cpu(), d.cpu())
    with pytest.raises(PsdfError):
        unit_box.ray_intersection(o.cpu(), d.cpu())
    frame = _frame(dev)
    with pytest.raises(ValueError):
        BoxPlayer(net3, unit_box, frame, max_rays_per_chunk=512)
    with pytest.raises(ValueError):
        render_box_traced(net4, unit_box, frame)
    with pytest.raises(ValueError):
        BoxPlayer(net4, unit_box, frame).frame_at()
    with pytest.raises(ValueError):
        BoxPlayer(net3, unit_box, frame).frame_at(0.5)
    # an empty batch of rays
    pts, sdf, grads, conv = BoxTracer(net3.enc, net3.mlp, unit_box, net3.win).trace(o[:0], d[:0])
    assert pts.shape == (0, 3) and sdf.shape == (0, 1) and grads.shape == (0, 3) and conv.shape == (0, 1)


def test_fitters_conveniences_trace_and_render_the_fit(dev, unit_box):
    """SdfFitter.tracer / .render: the fit's own box by default, a 4-D fit rendered at a time"""
    from permuto_sdf_amd import sdf_fit
    from permuto_sdf_amd.box_trace import render_box_traced
    g = torch.Generator().manual_seed(2)
    n = torch.nn.functional.normalize(torch.randn(4000, 3, generator=g), dim=1)
    t = torch.rand(4000, 1, generator=g)
    cloud = sdf_fit.OrientedCloud(torch.cat([n * 0.25, t], 1).to(dev), n.to(dev))
    fitter = sdf_fit.SdfFitter(cloud, n_surf=1000, n_off=1000)
    for _ in range(3):
        fitter.step()
    box = fitter.box()
    assert box.sizes_xyz == [1.0, 1.0, 1.0] and box.translation == [0.0, 0.0, 0.0]
    tracer = fitter.tracer()
    assert tracer.pos_dim == 4 and tracer.box.sizes_xyz == box.sizes_xyz
    frame = _frame(dev)
    a = fitter.render(frame, t=0.5, nr_sphere_traces=5)
    b = render_box_traced(fitter.net, unit_box, frame, it=fitter.iter, time_val=0.5, nr_sphere_traces=5)
    assert torch.equal(a.normals, b.normals) and torch.equal(a.weights_sum, b.weights_sum) and torch.equal(a.depth, b.depth)
    with pytest.raises(ValueError):
        fitter.render(frame)
