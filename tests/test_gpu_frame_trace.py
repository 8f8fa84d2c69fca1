"""Sphere-traced frames on the GPU (permuto_sdf_amd/render.py: render_traced; csrc/sampling.hip: trace_select_*;
csrc/frame_trace.hip).

  * select: the valid rays of a chunk -- not no_hit, end point in an occupied voxel, strictly inside the sphere -- and their
    compaction in ray order, bit for bit what torch's boolean mask gives, over wave and workgroup edges and forced patterns;
    `inside` is decided in float64, and no drawn point lies where fp32 could decide otherwise (asserted); the exact ties apart;
  * resolve: colour copied bit for bit, weight exactly 0 / 1, zeros at invalid rays, canaries everywhere else; normals, camera
    normals and depth per entry against float64 with derived bars;
  * whole frame: bit for bit the operator chain the tree already had (SphereTracer, check_occupancy,
    check_point_inside_primitive, boolean masks, the two networks, index_put), in one chunk and in eight;
  * a frame that looks away renders zeros without running a network; rendering leaves a training run as it was;
    render_views(mode="traced").

The bars, u = 2^-24:
  normals      n = g / max(|g|, eps): |g|^2 is three products and two sums of non-negative terms (at most 3u relative), the root
               halves that and rounds once (2.5u on |g|, counted as the 2u of a correctly rounded root plus room), the quotient
               rounds once more: 3.5u |n_c| <= 3.5u to first order.  Bar 4u per component.
  normals_cam  as tests/test_gpu_frame.py: normalize(R n) of the kernel's own fp32 normal; three products and two sums per entry
               (4u A_c, A_c = sum_j |R_cj| |n_j|), then the normalisation: |e|_2 / |c| + 4u.
  depth        ((px - ox) dx + (py - oy) dy) + (pz - oz) dz: every term carries the rounding of its difference (u), of its product
               (u) and of at most two sums (2u): 4u S to first order, S = sum_i |(p_i - o_i) d_i|.  Bar 5u S, the fifth u being room
               for the second-order terms: the constant is 5."""
import math

import pytest
import torch

from tests.float64_check import check, show

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
CANARY = -77.25
ICANARY = -7777
PAD = 64
RADIUS = 0.5
SIZES = [1, 63, 64, 65, 255, 256, 257, 1000, 5 * 256 + 17]
PATTERNS = ["random", "none", "all", "first", "last", "no_hit_on_valid"]


# ============================================================================================================== select
def _grid_and_sphere(dev):
    from permuto_sdf_amd.bridge import OccupancyGrid, Sphere
    grid = OccupancyGrid(32, 1.0, [0, 0, 0], device=dev)
    g = torch.Generator().manual_seed(5)
    grid.set_grid_occupancy((torch.rand(32 ** 3, generator=g) < 0.5).to(dev))
    return grid, Sphere(RADIUS, [0, 0, 0])


def _inside64(pts):
    """the sphere predicate in float64, after asserting that NO point lies where fp32 could decide otherwise: the fp32 norm is
    within 2.5u |p| of the exact one (see the normals' bar), so the two can differ only for | |p - c| - r | <= 4u r"""
    n = pts.detach().cpu().double().norm(dim=1)
    assert not bool(((n - RADIUS).abs() <= 4 * U * RADIUS).any()), "a drawn point lies in the band where fp32 may decide otherwise"
    return n < RADIUS


def _draw(R, seed):
    """points uniform in [-0.7, 0.7]^3 (some outside the grid, some outside the sphere), unit directions, no_hit on a quarter"""
    g = torch.Generator().manual_seed(seed)
    pts = (torch.rand(R, 3, generator=g) * 2 - 1) * 0.7
    d = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=1)
    no_hit = torch.rand(R, generator=g) < 0.25
    return pts, d, no_hit


def _case(dev, grid, R, pattern):
    """-> pts, dirs, no_hit on the device and the wanted mask, from operators the tree already had"""
    seed = 1000 * PATTERNS.index(pattern) + R
    if pattern in ("random", "none"):
        pts, d, no_hit = _draw(R, seed)
        if pattern == "none":
            no_hit[:] = True
    else:   # R points that are valid but for no_hit: the first R of a larger draw that the existing operators accept
        cand, d, _ = _draw(16 * R + 64, seed)
        ok = grid.check_occupancy(cand.to(dev)).view(-1).cpu() & _inside64(cand)
        assert int(ok.sum()) >= R
        pts, d = cand[ok][:R].contiguous(), d[:R].contiguous()
        no_hit = torch.zeros(R, dtype=torch.bool)
        if pattern == "first":
            no_hit[1:] = True
        elif pattern == "last":
            no_hit[:-1] = True
        elif pattern == "no_hit_on_valid":
            no_hit = torch.rand(R, generator=torch.Generator().manual_seed(seed + 1)) < 0.5
    pts, d, no_hit = pts.to(dev), d.to(dev), no_hit.to(dev)
    valid = ~no_hit & grid.check_occupancy(pts).view(-1) & _inside64(pts).to(dev)
    return pts, d, no_hit, valid


def _select(dev, grid, sphere, pts, d, no_hit):
    """the raw entry into canary-padded buffers -> slot [R], pos [R, 3], dirs [R, 3] (rows from M on still canary), M"""
    from permuto_sdf_amd import render
    R = pts.shape[0]
    nscratch = 2 * ((R + 255) // 256)
    scratch = torch.full((nscratch + 2 * PAD,), ICANARY, dtype=torch.int32, device=dev)
    slot = torch.full((R + 2 * PAD,), ICANARY, dtype=torch.int32, device=dev)
    pos = torch.full((R + 2 * PAD, 3), CANARY, device=dev)
    dirs = torch.full((R + 2 * PAD, 3), CANARY, device=dev)
    count = torch.full((1 + 2 * PAD,), ICANARY, dtype=torch.int32, device=dev)
    render.trace_frame_select_raw(grid, sphere, pts, d, no_hit, scratch[PAD:PAD + nscratch], slot[PAD:PAD + R], pos[PAD:PAD + R],
                                  dirs[PAD:PAD + R], count[PAD:PAD + 1])
    M = int(count[PAD])
    for buf, n in ((scratch, nscratch), (slot, R), (count, 1)):
        assert bool((buf[:PAD] == ICANARY).all()) and bool((buf[PAD + n:] == ICANARY).all())
    for buf in (pos, dirs):
        assert bool((buf[:PAD] == CANARY).all()) and bool((buf[PAD + M:] == CANARY).all())      # rows from M on are not written
    return slot[PAD:PAD + R], pos[PAD:PAD + R], dirs[PAD:PAD + R], M


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("R", SIZES)
def test_select_is_the_boolean_mask_of_the_existing_operators_bit_for_bit(dev, R, pattern):
    grid, sphere = _grid_and_sphere(dev)
    pts, d, no_hit, valid = _case(dev, grid, R, pattern)
    slot, pos, dirs, M = _select(dev, grid, sphere, pts, d, no_hit)
    want_M = int(valid.sum())
    if pattern == "random" and R >= 63:
        assert 0 < want_M < R
        inside = _inside64(pts).to(dev)
        assert bool((~inside).any()) and bool((pts.abs().max(dim=1).values > 0.5).any())      # outside the sphere, outside the grid
    elif pattern in ("none", "all", "first", "last"):
        assert want_M == {"none": 0, "all": R, "first": 1, "last": 1}[pattern]
    assert M == want_M
    want_slot = torch.where(valid, torch.cumsum(valid.int(), 0, dtype=torch.int32) - 1, torch.full_like(slot, -1))
    assert torch.equal(slot, want_slot)
    assert torch.equal(pos[:M], pts[valid]) and torch.equal(dirs[:M], d[valid])
    # the same predicate through the sphere's own fp32 operator
    assert torch.equal(valid, ~no_hit & grid.check_occupancy(pts).view(-1) & sphere.check_point_inside_primitive(pts).view(-1))
    # a second call: the same bits
    slot2, pos2, dirs2, M2 = _select(dev, grid, sphere, pts, d, no_hit)
    assert M2 == M and torch.equal(slot2, slot) and torch.equal(pos2, pos) and torch.equal(dirs2, dirs)


def test_select_decides_the_exact_ties_of_the_sphere_as_not_inside(dev):
    from permuto_sdf_amd.bridge import OccupancyGrid, Sphere
    # every voxel occupied, and a cube of edge 2: the offsets of length 0.5 lie well inside it, the sphere alone decides (in the
    # unit cube x = 0.5 - 2^-25 is outside: x + 0.5 rounds to 1)
    grid = OccupancyGrid(32, 2.0, [0, 0, 0], device=dev)
    c = [0.0, -0.0625, 0.25]                                       # exact in fp32, as are the sums and differences below
    sphere = Sphere(RADIUS, c)
    below = float(torch.nextafter(torch.tensor(0.5), torch.tensor(0.0)))
    off = torch.tensor([[0.5, 0.0, 0.0], [0.0, -0.5, 0.0], [0.3, 0.4, 0.0], [below, 0.0, 0.0]])
    pts = (off.double() + torch.tensor(c, dtype=torch.float64)).float()
    # (0.3, 0.4, 0) in fp32: the squares round to a sum whose root is exactly 0.5 -- the tie the issue names
    q = pts[2] - torch.tensor(c)
    assert float(torch.sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2])) == 0.5
    assert torch.equal(pts - torch.tensor(c), off)                 # every offset survives the round trip through p
    pts = pts.to(dev)
    d = torch.zeros(4, 3, device=dev)
    slot, pos, _, M = _select(dev, grid, sphere, pts, d, torch.zeros(4, dtype=torch.bool, device=dev))
    assert slot.tolist() == [-1, -1, -1, 0] and M == 1 and torch.equal(pos[0], pts[3])


def test_select_refuses_bad_arguments_and_skips_an_empty_chunk(dev):
    import ctypes
    from permuto_sdf_amd import _lib as L
    fn = L.lib().psdf_trace_frame_select
    p, t = ctypes.c_void_p(4096), (ctypes.c_float * 3)(0, 0, 0)     # (never read: every call returns before a launch)
    f = ctypes.c_float
    assert fn(0, 32, f(1), None, None, f(0.5), None, None, None, None, None, None, None, None, None, None) == 0
    assert fn(-1, 32, f(1), t, p, f(0.5), t, p, p, p, p, p, p, p, p, None) == -1
    for k in (3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14):
        args = [8, 32, f(1), t, p, f(0.5), t, p, p, p, p, p, p, p, p, None]
        args[k] = None
        assert fn(*args) == -1, k


# ============================================================================================================= resolve
def _rotation(dev):
    """a rotation that is no permutation: 50 degrees about (1, 2, 3) / sqrt(14), float64 rounded to float32"""
    a = torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64)
    a = a / a.norm()
    Kx = torch.tensor([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]], dtype=torch.float64)
    th = math.radians(50.0)
    R = torch.eye(3, dtype=torch.float64) + math.sin(th) * Kx + (1 - math.cos(th)) * (Kx @ Kx)
    return R.float().contiguous().to(dev)


def _rows(img, first, R):
    """[C, H, W] -> the [R, C] rows of the pixels [first, first + R), and the others"""
    flat = img.reshape(img.shape[0], -1)
    outside = torch.ones(flat.shape[1], dtype=torch.bool, device=img.device)
    outside[first:first + R] = False
    return flat[:, first:first + R].t().contiguous(), flat[:, outside]


@pytest.mark.parametrize("pattern", ["random", "no_hit_on_valid"])      # about one ray in sixteen valid, and every second one
@pytest.mark.parametrize("H,W,first,R", [(7, 13, 0, 91), (40, 48, 77, 333)])
def test_resolve_copies_colour_and_meets_the_float64_bars_of_normals_and_depth(dev, H, W, first, R, pattern):
    from permuto_sdf_amd import _lib as L
    from permuto_sdf_amd import render
    grid, sphere = _grid_and_sphere(dev)
    pts, d, no_hit, valid = _case(dev, grid, R, pattern)
    slot, pos, _, M = _select(dev, grid, sphere, pts, d, no_hit)
    slot, pos = slot.contiguous(), pos[:M].contiguous()
    assert 2 <= M < R
    g = torch.Generator().manual_seed(R)
    o = ((torch.rand(R, 3, generator=g) * 2 - 1) * 1.5).to(dev)
    grad = ((torch.rand(M, 3, generator=g) * 2 - 1) * 2).to(dev)
    grad[0] = 0.0                                                   # a zero gradient: normal 0 through the eps
    grad[1] = torch.tensor([1e-20, 0.0, 0.0])                       # |g|^2 underflows: g / eps
    rgb = torch.rand(M, 3, generator=g).to(dev)
    rot = _rotation(dev)

    def planes():
        return [torch.full((c, H, W), CANARY, device=dev) for c in (3, 3, 3, 1, 1)]

    img, nimg, cimg, wimg, dimg = planes()
    render.trace_frame_resolve_raw(slot, M, o, d, pos, grad, rgb, H, W, first, img, nimg, wimg, dimg, cimg, rot)
    got = {}
    for name, plane in (("rgb", img), ("normals", nimg), ("normals_cam", cimg), ("weights_sum", wimg), ("depth", dimg)):
        got[name], outside = _rows(plane, first, R)
        assert bool((outside == CANARY).all()), name
        assert bool((got[name][~valid] == 0).all()), name          # exactly 0 at the invalid rays of the chunk
    assert torch.equal(got["rgb"][valid], rgb)
    assert torch.equal(got["weights_sum"].view(-1), valid.float())
    # a second call: the same bits; without camera normals the other planes are the same bits and that plane is untouched
    again = planes()
    render.trace_frame_resolve_raw(slot, M, o, d, pos, grad, rgb, H, W, first, again[0], again[1], again[3], again[4], again[2], rot)
    assert all(torch.equal(a, b) for a, b in zip(again, (img, nimg, cimg, wimg, dimg)))
    plain = planes()
    render.trace_frame_resolve_raw(slot, M, o, d, pos, grad, rgb, H, W, first, plain[0], plain[1], plain[3], plain[4])
    assert all(torch.equal(plain[i], (img, nimg, cimg, wimg, dimg)[i]) for i in (0, 1, 3, 4)) and bool((plain[2] == CANARY).all())
    # float64, per entry
    live = valid.cpu()
    out = []
    g64 = torch.zeros(R, 3, dtype=torch.float64)
    g64[live] = grad.cpu().double()
    eps = float(torch.tensor(1e-12, dtype=torch.float32))
    want_n = g64 / g64.norm(dim=1, keepdim=True).clamp_min(eps)
    check(out, "normals", got["normals"], want_n, torch.full((R, 3), 4 * U, dtype=torch.float64), keep=live)
    hit_rows = torch.nonzero(live).view(-1)
    assert bool((got["normals"][hit_rows[0]] == 0).all()) and bool((got["normals_cam"][hit_rows[0]] == 0).all())
    assert abs(float(got["normals"][hit_rows[1], 0]) - 1e-20 / eps) <= 4 * U
    n64, R64 = got["normals"].cpu().double(), rot.cpu().double()
    cam = n64 @ R64.t()
    cn = cam.norm(dim=1, keepdim=True)
    e = 4 * U * (n64.abs() @ R64.abs().t())
    want_c = torch.where(live[:, None], cam / cn.clamp_min(1e-300), torch.zeros_like(cam))
    bar_c = (e.norm(dim=1, keepdim=True) / cn.clamp_min(1e-300) + 4 * U).expand(-1, 3)
    check(out, "normals_cam", got["normals_cam"], want_c, bar_c, keep=live)
    p64 = torch.zeros(R, 3, dtype=torch.float64)
    p64[live] = pos.cpu().double()
    terms = (p64 - o.cpu().double()) * d.cpu().double()
    want_d = torch.where(live, terms.sum(1), torch.zeros(R, dtype=torch.float64)).view(-1, 1)
    check(out, "depth", got["depth"], want_d, (5 * U * terms.abs().sum(1)).view(-1, 1), keep=live)
    show("resolve %d x %d, pixels [%d, %d), %s, %d valid" % (H, W, first, first + R, pattern, M), out)
    # no valid ray: the dense arrays may be missing
    img0, nimg0, _, wimg0, dimg0 = planes()
    render.trace_frame_resolve_raw(torch.full_like(slot, -1), 0, o, d, None, None, None, H, W, first, img0, nimg0, wimg0, dimg0)
    for plane in (img0, nimg0, wimg0, dimg0):
        inside, outside = _rows(plane, first, R)
        assert bool((inside == 0).all()) and bool((outside == CANARY).all())
    # the refusals
    fn = L.lib().psdf_trace_frame_resolve

    def call(H_=H, W_=W, first_=first):
        return fn(L.c_i(R), L.c_i(M), L.ptr(slot), L.ptr(o), L.ptr(d), L.ptr(pos), L.ptr(grad), L.ptr(rgb), None, L.c_i(H_), L.c_i(W_),
                  L.c_l(first_), L.ptr(img0), L.ptr(nimg0), None, L.ptr(wimg0), L.ptr(dimg0), L.stream())

    assert call(first_=H * W - R + 1) == -1 and call(H_=0) == -1


# ========================================================================================================= whole frame
H, W = 40, 48
IT = 9999999
TRACE = (15, 0.9, 2e-4)


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


def _yardstick(tr, frame, max_rays):
    """the operator chain the tree already had, on the same rays in the same chunks -> rgb, gradient, weights_sum, depth planes"""
    from permuto_sdf_amd import render
    from permuto_sdf_amd.sphere_trace import SphereTracer
    dev = frame.K.device
    plan = render.FramePlan(frame.height, frame.width, 1, max_rays)
    rnd = render.FrameRenderer(tr)
    net = tr.sdf
    tracer = SphereTracer(net.encoding, net.mlp_sdf, tr.grid, tr.sphere, net.window(IT).float())
    HW = frame.height * frame.width
    rows = {k: torch.zeros(HW, c, device=dev) for k, c in (("rgb", 3), ("gradient", 3), ("normals", 3), ("weights_sum", 1), ("depth", 1))}
    with torch.no_grad():
        for first, count in plan.chunks():
            o, d = render.frame_rays(frame, first, count)
            pts = tracer.trace(o, d, *TRACE, return_gradients=False)[0]
            valid = (~tracer.no_hit) & tr.grid.check_occupancy(pts).view(-1) & tr.sphere.check_point_inside_primitive(pts).view(-1)
            if not bool(valid.any()):
                continue
            p, dd, oo = pts[valid], d[valid], o[valid]
            _, grad, feat = rnd._sdf_and_gradient(p, IT)
            rgb = tr.rgb(p, dd, grad, feat)
            q = p - oo
            depth = (q[:, 0] * dd[:, 0] + q[:, 1] * dd[:, 1]) + q[:, 2] * dd[:, 2]
            idx = (torch.nonzero(valid).view(-1) + first,)
            rows["rgb"].index_put_(idx, rgb.float())
            rows["gradient"].index_put_(idx, grad.float())
            rows["normals"].index_put_(idx, torch.nn.functional.normalize(grad.float(), dim=1))
            rows["weights_sum"].index_put_(idx, torch.ones(p.shape[0], 1, device=dev))
            rows["depth"].index_put_(idx, depth.view(-1, 1))
    return {k: v.t().reshape(-1, frame.height, frame.width).contiguous() for k, v in rows.items()}, plan


def test_whole_frame_is_the_operator_chain_bit_for_bit_in_two_chunkings(dev, trained):
    from permuto_sdf_amd import render
    from permuto_sdf_amd._lib import PsdfError
    tr, reel = trained
    frame = render.Frame.from_reel(reel, 1)
    rnd = render.FrameRenderer(tr)
    for max_rays, chunks in ((1 << 21, [(0, 1920)]), (256, [(256 * i, 256) for i in range(7)] + [(1792, 128)])):
        yard, plan = _yardstick(tr, frame, max_rays)
        assert plan.chunks() == chunks
        out = rnd.render_traced(frame, max_rays_per_chunk=max_rays)
        assert out.normals_cam is None
        for k in ("rgb", "normals", "weights_sum", "depth"):
            v = getattr(out, k)
            assert v.dtype == torch.float32 and v.is_cuda and v.shape == ((3 if k in ("rgb", "normals") else 1), H, W), k
            assert bool(torch.isfinite(v).all()), k
        for k in ("rgb", "weights_sum", "depth"):
            assert torch.equal(getattr(out, k), yard[k]), (len(chunks), k, float((getattr(out, k) - yard[k]).abs().max()))
        # the frame is not trivial
        ws = out.weights_sum
        hit = ws.view(-1) == 1
        print("%d chunk(s): %.1f%% of the pixels hit" % (len(chunks), 100 * float(hit.float().mean())))
        assert int(hit.sum()) > 0 and int((ws == 0).sum()) > 0 and bool(((ws == 0) | (ws == 1)).all())
        assert torch.equal(out.depth > 0, ws == 1)
        # normals: torch's F.normalize has the same formula; its bits may differ from normalize_eps (the order of the norm's
        # sum is torch's own), so the normals are held to the bar of the resolve test against float64 of the chain's gradient
        g64 = yard["gradient"].reshape(3, -1).t().cpu().double()
        eps = float(torch.tensor(1e-12, dtype=torch.float32))
        want = g64 / g64.norm(dim=1, keepdim=True).clamp_min(eps)
        lines = []
        check(lines, "normals", out.normals.reshape(3, -1).t().contiguous(), want, torch.full_like(want, 4 * U), keep=hit.cpu())
        show("whole frame in %d chunk(s)" % len(chunks), lines)
        print("normals that differ in bits from F.normalize: %d of %d" % (int((out.normals != yard["normals"]).sum()), out.normals.numel()))
        assert bool((out.normals.reshape(3, -1)[:, ~hit] == 0).all())
        # hit pixels near the image centre: the depth lies between the bounding sphere's entry and exit of that ray
        o, d = render.frame_rays(frame)
        _, t0, _, t1, _ = tr.sphere.ray_intersection(o, d)
        centre = torch.zeros(H, W, dtype=torch.bool, device=dev)
        centre[H // 2 - 4:H // 2 + 4, W // 2 - 4:W // 2 + 4] = True
        sel = centre.view(-1) & hit
        assert int(sel.sum()) > 0
        dep = out.depth.view(-1)[sel]
        assert bool((dep >= t0.view(-1)[sel] - 1e-5).all()) and bool((dep <= t1.view(-1)[sel] + 1e-5).all())
    # camera normals: the same other planes, and the world normals rotated by the rotation of tf_cam_world
    plain = rnd.render_traced(frame)
    cam = rnd.render_traced(frame, camera_normals=True)
    for k in ("rgb", "normals", "weights_sum", "depth"):
        assert torch.equal(getattr(cam, k), getattr(plain, k)), k
    hit = (cam.weights_sum.view(-1) == 1).cpu()
    n64, R64 = cam.normals.double().reshape(3, -1).t().cpu(), frame.tf_world_cam[:3, :3].t().double().cpu()
    c = n64 @ R64.t()
    cn = c.norm(dim=1, keepdim=True)
    e = 4 * U * (n64.abs() @ R64.abs().t())
    want = torch.where(hit[:, None], c / cn.clamp_min(1e-300), torch.zeros_like(c))
    bar = (e.norm(dim=1, keepdim=True) / cn.clamp_min(1e-300) + 4 * U).expand(-1, 3)
    lines = []
    check(lines, "normals_cam", cam.normals_cam.reshape(3, -1).t().contiguous(), want, bar, keep=hit)
    show("whole frame", lines)
    assert bool((cam.normals_cam.reshape(3, -1)[:, ~hit.to(dev)] == 0).all())
    # a frame on another device than the models is refused before any launch
    with pytest.raises(PsdfError):
        rnd.render_traced(render.Frame(frame.K.cpu(), frame.tf_world_cam.cpu(), H, W))


def test_a_frame_that_looks_away_renders_zeros_without_running_a_network(dev, trained, monkeypatch):
    from permuto_sdf_amd import render
    tr, reel = trained
    tf = reel.tf_world_cam_reel[1].clone()
    tf[:3, 0] *= -1                   # half a turn about the camera's y axis: x and z flip
    tf[:3, 2] *= -1
    frame = render.Frame(reel.K_reel[1], tf, H, W)
    rnd = render.FrameRenderer(tr)

    def never(*a, **k):
        raise AssertionError("a network ran for a chunk without a valid ray")

    monkeypatch.setattr(tr, "rgb", never)
    monkeypatch.setattr(rnd, "_sdf_and_gradient", never)
    for max_rays in (1 << 21, 256):
        out = rnd.render_traced(frame, camera_normals=True, max_rays_per_chunk=max_rays)
        for k in ("rgb", "normals", "normals_cam", "weights_sum", "depth"):
            assert bool((getattr(out, k) == 0).all()), k


def test_traced_rendering_leaves_a_training_run_as_it_was(dev, trained):
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
    out = render.FrameRenderer(tr).render_traced(render.Frame.from_reel(reel, 0), max_rays_per_chunk=256, camera_normals=True)
    assert bool(torch.isfinite(out.rgb).all()) and int((out.weights_sum == 1).sum()) > 0
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


def test_render_views_stacks_the_traced_colours_on_request(dev, trained):
    from permuto_sdf_amd import render
    tr, reel = trained
    rnd = render.FrameRenderer(tr)
    frames = [render.Frame.from_reel(reel, i) for i in (0, 3)]
    views = rnd.render_views(frames, mode="traced")
    assert views.shape == (2, 3, H, W) and views.dtype == torch.float32 and views.is_cuda
    assert torch.equal(views, torch.stack([rnd.render_traced(f).rgb for f in frames]))
    assert torch.equal(rnd.render_views(frames, mode="traced", max_rays_per_chunk=256),
                       torch.stack([rnd.render_traced(f, max_rays_per_chunk=256).rgb for f in frames]))
    default = torch.stack([rnd.render(f).rgb for f in frames])
    assert torch.equal(rnd.render_views(frames), default) and torch.equal(rnd.render_views(frames, mode="volumetric"), default)
    assert not torch.equal(views, default)
    with pytest.raises(ValueError):
        rnd.render_views(frames, mode="sphere")
    with pytest.raises(ValueError):
        rnd.render_views([], mode="traced")
