"""The NeRF frame renderer on the GPU (permuto_sdf_amd/nerf_view.py, csrc/frame_composite.hip: frame_render_nerf_kernel).

  1. kernel against the kernel the tree has: radiance, weight sum and transmittance bit-for-bit psdf_nerf_render_forward's for
     the containers of tests/nerf_render_float64.py (rays of 0, 1, 63, 64, 65, 128, 129 and 256 samples, empty and overflowed
     rays, the equal-count mode), the depth bit-for-bit that kernel's first channel with the colours replaced by z, written at
     a pixel offset with canaries around; without a depth plane the other planes hold the same bits;
  2. kernel against float64, every entry within the bar of nerf_render_float64.render; the depth against the same evaluator
     with the colours replaced by z (z enters as exact fp32 coefficients, as a colour does: the derivation holds unchanged);
  3. a container without samples renders zeros and ones from NULL sample pointers;
  4. whole frame, with a background and under with_mask: bit-for-bit the chain frame_rays -> NerfTrainer.sample ->
     _branch_forward -> nerf_render_raw -> nerf_composite_forward_raw on the same chunks, scattered by torch; two chunkings
     agree entry by entry to within twice what that chain itself moves between them;
  5. an empty grid: foreground planes and depth zero, rgb == rgb_bg;
  6. rendering leaves a run as it was; 7. a checkpoint renders what its trainer renders, views go straight into the scores,
     and 60 steps on a constant-colour reel raise the PSNR of view 0.

The 60 x 80 frame of a SyntheticReel has the camera at distance 1.5 with focal length 1.2 W: the image centre hits the
radius-0.5 sphere (half angle 19.5 degrees), the corners (27.5 degrees off the axis) miss it."""
import math
import types

import pytest
import torch

from tests import nerf_render_float64 as n64
from tests.float64_check import check, show

pytestmark = pytest.mark.gpu

CANARY = -77.25
FIRST = 37                  # pixel offset of the kernel cases, as in tests/test_gpu_frame.py
FH, FW = 13, 17             # their frame: 221 pixels, more than 37 + 11
H, W = 60, 80
POOL_5, POOL_19 = 64 * 1024, 64 * 256       # four chunks of 1 024 rays and one of 704; 18 of 256 and one of 192


# ============================================================================================================ the kernel
def _z(c, seed=0):
    """[N, 1]: seeded, positive, increasing along each ray (from 0.4, in steps of 0.01 .. 0.06)"""
    g = torch.Generator().manual_seed(6000 + seed)
    N = c["N"]
    step = torch.rand(N, generator=g) * 0.05 + 0.01
    z = torch.zeros(N)
    for s, e in c["start_end"].tolist():
        e = min(e, N)
        if e > s:
            z[s:e] = 0.4 + torch.cumsum(step[s:e], 0)
    return z.view(-1, 1)


def _make_rs(c, dev, dt=None, z=None, N=None):
    from permuto_sdf import RaySamplesPacked
    N = c["N"] if N is None else N
    rs = RaySamplesPacked(c["R"], N, device=dev)
    rs.ray_start_end_idx = c["start_end"].to(dev)
    if c["equal"]:
        rs.rays_have_equal_nr_of_samples, rs.fixed_nr_of_samples_per_ray = True, c["fixed"]
    if dt is not None:
        rs.samples_dt = dt.to(dev).view(-1, 1).contiguous()
    if z is not None:
        rs.samples_z = z.to(dev).view(-1, 1).contiguous()
    rs.cur_nr_samples.fill_(min(N, c["total"]))
    return rs


def _planes(dev, c):
    return torch.full((c, FH, FW), CANARY, device=dev)


def _inside(img, R):
    """[C, H, W] -> the [R, C] rows of the pixels [FIRST, FIRST + R), and the others"""
    flat = img.reshape(img.shape[0], -1)
    outside = torch.ones(flat.shape[1], dtype=torch.bool, device=img.device)
    outside[FIRST:FIRST + R] = False
    return flat[:, FIRST:FIRST + R].t().contiguous(), flat[:, outside]


@pytest.fixture(scope="module")
def kernel_cases(dev):
    """(container, family) -> the inputs, what the existing kernel gives and what the new one writes; computed once"""
    from permuto_sdf_amd import nerf_view
    from permuto_sdf_amd.nerf_train import nerf_render_raw
    cases = {}
    for cname in ("borders", "equal65"):
        c = n64.container(cname)
        R, N = c["R"], c["N"]
        assert FIRST + R < FH * FW
        z = _z(c)
        for s, e in c["start_end"].tolist():        # positive and increasing along each ray
            zz = z[s:min(e, N), 0]
            assert bool((zz > 0).all()) and bool((zz[1:] > zz[:-1]).all())
        for fam in ("float64", "saturated"):
            raw, dt, rgb = n64.family(c, fam)
            rs = _make_rs(c, dev, dt, z)
            raw_d, rgb_d = raw.to(dev), rgb.to(dev)
            pred, ws, bg = nerf_render_raw(rs, raw_d, rgb_d)
            zpred = nerf_render_raw(rs, raw_d, z.expand(N, 3).contiguous().to(dev), want_weights_sum=False, want_bg=False)[0]
            img, wimg, dimg = _planes(dev, 3), _planes(dev, 1), _planes(dev, 1)
            T = torch.full((R + 8,), CANARY, device=dev)
            nerf_view.frame_render_nerf_raw(rs, raw_d, rgb_d, FH, FW, FIRST, img, wimg, T, dimg)
            cases[cname, fam] = types.SimpleNamespace(c=c, rs=rs, raw=raw, dt=dt, rgb=rgb, z=z, raw_d=raw_d, rgb_d=rgb_d, pred=pred,
                                                      ws=ws, bg=bg, zpred=zpred, img=img, wimg=wimg, dimg=dimg, T=T)
    torch.cuda.synchronize()
    return cases


@pytest.mark.parametrize("fam", ["float64", "saturated"])
@pytest.mark.parametrize("cname", ["borders", "equal65"])
def test_kernel_is_the_existing_render_bit_for_bit_in_planes(dev, kernel_cases, cname, fam):
    from permuto_sdf_amd import nerf_view
    k = kernel_cases[cname, fam]
    c, R = k.c, k.c["R"]
    got = {}
    for name, plane in (("rgb", k.img), ("weights_sum", k.wimg), ("depth", k.dimg)):
        got[name], outside = _inside(plane, R)
        assert bool((outside == CANARY).all()), name
    assert bool((k.T[R:] == CANARY).all())
    assert torch.equal(got["rgb"], k.pred)
    assert torch.equal(got["weights_sum"], k.ws)
    assert torch.equal(k.T[:R].view(-1, 1), k.bg)
    assert torch.equal(got["depth"], k.zpred[:, :1])
    assert float(got["depth"].max()) > 0.1 and float(got["rgb"].max()) > 0.1
    # without a depth plane the other planes hold the same bits (z is then not read: the container has none)
    rs2 = _make_rs(c, dev, k.dt)
    img2, wimg2, T2 = _planes(dev, 3), _planes(dev, 1), torch.empty(R, device=dev)
    nerf_view.frame_render_nerf_raw(rs2, k.raw_d, k.rgb_d, FH, FW, FIRST, img2, wimg2, T2)
    assert torch.equal(img2, k.img) and torch.equal(wimg2, k.wimg) and torch.equal(T2, k.T[:R])
    # empty and overflowed rays: 0, 0, 0 and 1
    skipped = ~n64.rays_of(c).valid
    if cname == "borders":
        assert int(skipped.sum()) == 4
    sk = skipped.to(dev)
    for name in ("rgb", "weights_sum", "depth"):
        assert bool((got[name][sk] == 0).all()), name
    assert bool((k.T[:R][sk] == 1).all())


@pytest.mark.parametrize("cname", ["borders", "equal65"])
def test_kernel_lies_within_its_float64_bars(dev, kernel_cases, cname):
    k = kernel_cases[cname, "float64"]
    c, R, N = k.c, k.c["R"], k.c["N"]
    rays = n64.rays_of(c)
    ref = n64.render(rays, k.raw, k.dt, k.rgb)
    assert ref["min_om"] > 1e-4                 # the regime the bars are derived for
    ref_z = n64.render(rays, k.raw, k.dt, k.z.expand(N, 3).contiguous())
    out = []
    check(out, "pred", _inside(k.img, R)[0], *ref["pred"])
    check(out, "weights_sum", _inside(k.wimg, R)[0], *ref["weights_sum"])
    check(out, "bg", k.T[:R], *ref["bg"])
    check(out, "depth", _inside(k.dimg, R)[0], ref_z["pred"][0][:, 0], ref_z["pred"][1][:, 0])
    show("nerf frame render %s" % cname, out)


def test_a_container_without_samples_renders_the_empty_values_from_null_pointers(dev):
    from permuto_sdf_amd import _lib as L
    from permuto_sdf_amd import nerf_view
    c = n64.container("borders")
    R = c["R"]
    se = c["start_end"].to(dev)

    def verify(img, wimg, dimg, T):
        for plane in (img, wimg, dimg):
            inside, outside = _inside(plane, R)
            assert bool((inside == 0).all()) and bool((outside == CANARY).all())
        assert bool((T[:R] == 1).all()) and bool((T[R:] == CANARY).all())

    for equal, fixed in ((0, 0), (1, 64), (1, 0)):
        img, wimg, dimg = _planes(dev, 3), _planes(dev, 1), _planes(dev, 1)
        T = torch.full((R + 8,), CANARY, device=dev)
        L.call("psdf_nerf_frame_render", L.c_i(R), L.ptr(se), L.c_i(equal), L.c_i(fixed), L.c_i(0), None, None, None, None, L.c_i(FH),
               L.c_i(FW), L.c_l(FIRST), L.ptr(img), L.ptr(wimg), L.ptr(dimg), L.ptr(T), L.stream())
        verify(img, wimg, dimg, T)
    # and through the wrapper
    img, wimg, dimg = _planes(dev, 3), _planes(dev, 1), _planes(dev, 1)
    T = torch.full((R + 8,), CANARY, device=dev)
    nerf_view.frame_render_nerf_raw(_make_rs(c, dev, N=0), None, None, FH, FW, FIRST, img, wimg, T, dimg)
    verify(img, wimg, dimg, T)


# =========================================================================================================== whole frame
def _hp(nr_rays):
    from permuto_sdf_amd.nerf_train import HyperParams
    hp = HyperParams()
    hp.nr_rays = nr_rays
    return hp


def _reel(dev, constant=False):
    from permuto_sdf_amd.train_step import SyntheticReel
    reel = SyntheticReel(dev, nr_images=4, height=H, width=W)
    if constant:
        reel.rgb_reel[:] = torch.tensor([0.8, 0.3, 0.1], device=dev).view(1, 3, 1, 1)
    return reel


@pytest.fixture(scope="module")
def trained(dev):
    """a seeded trainer after 10 steps: the grid was refreshed at iterations 0 and 8"""
    from permuto_sdf_amd.nerf_train import NerfTrainer
    reel = _reel(dev)
    tr = NerfTrainer(dev, hp=_hp(256), seed=11)
    for _ in range(10):
        tr.step(reel)
    torch.cuda.synchronize()
    return tr, reel


def _yardstick(t, frame, pool, it):
    """the operator chain the tree already had, on the same rays in the same chunks, scattered by torch -> rgb, rgb_bg,
    weights_sum, depth as planes, and the foreground samples of every ray"""
    from permuto_sdf_amd import render
    from permuto_sdf_amd.nerf_train import NerfTrainer, nerf_render_raw
    from permuto_sdf_amd.neus import nerf_composite_forward_raw
    hp, dev = t.hp, frame.K.device
    plan = render.FramePlan(frame.height, frame.width, hp.max_nr_samples_per_ray, pool)
    keep_pool = t.grid.max_nr_samples
    t.grid.max_nr_samples = pool
    rows = {k: [] for k in ("rgb", "rgb_bg", "weights_sum", "depth", "counts")}
    with torch.no_grad():
        for first, count in plan.chunks():
            o, d = render.frame_rays(frame, first, count)
            _, fg, bg = NerfTrainer.sample(t, o, d, False)
            if fg.samples_pos.shape[0] == 0:
                pred, dep = torch.zeros(count, 3, device=dev), torch.zeros(count, 1, device=dev)
                ws, bgT = torch.zeros(count, 1, device=dev), torch.ones(count, 1, device=dev)
            else:
                B = NerfTrainer._branch_forward(t.net, fg.samples_pos, fg.samples_dirs, it)
                pred, ws, bgT = nerf_render_raw(fg, B.raw_den, B.rgb)
                dep = nerf_render_raw(fg, B.raw_den, fg.samples_z.expand(-1, 3).contiguous(), want_weights_sum=False,
                                      want_bg=False)[0][:, :1]
            if bg is not None:
                B = NerfTrainer._branch_forward(t.net_bg, bg.samples_pos_4d, bg.samples_dirs, it)
                pred_bg, pred = nerf_composite_forward_raw(bg, B.raw_den, B.rgb, pred, bgT)
                rows["rgb_bg"].append(bgT * pred_bg)             # one fp32 product: one rounding
            se = fg.ray_start_end_idx
            rows["counts"].append((se[:, 1] - se[:, 0]).view(-1, 1).float())
            rows["rgb"].append(pred)
            rows["weights_sum"].append(ws)
            rows["depth"].append(dep)
    t.grid.max_nr_samples = keep_pool
    return {k: torch.cat(v, 0).t().reshape(-1, frame.height, frame.width).contiguous() if v else None for k, v in rows.items()}


PLANES = ("rgb", "rgb_bg", "weights_sum", "depth")


@pytest.mark.parametrize("with_mask", [False, True])
def test_whole_frame_is_the_operator_chain_bit_for_bit_in_two_chunkings(dev, trained, with_mask):
    from permuto_sdf_amd import nerf_view, render
    tr, reel = trained
    assert tr.iter == 10
    frame = render.Frame.from_reel(reel, 1)
    assert (frame.height, frame.width) == (H, W)
    t = tr
    if with_mask:          # the same nets without the background one (the sampling then makes no background samples)
        t = types.SimpleNamespace(net=tr.net, net_bg=None, grid=tr.grid, sphere=tr.sphere, hp=tr.hp, with_mask=True, iter=tr.iter)
    rnd = nerf_view.NerfFrameRenderer(t) if with_mask else tr.renderer()
    assert isinstance(rnd, nerf_view.NerfFrameRenderer)
    got, yard = {}, {}
    for pool, chunks, last in ((POOL_5, 5, 704), (POOL_19, 19, 192)):
        plan = render.FramePlan(H, W, tr.hp.max_nr_samples_per_ray, pool)
        assert (plan.nr_chunks, plan.last_chunk) == (chunks, last)
        out = rnd.render(frame, pool_samples=pool, depth=True)
        got[chunks] = {k: getattr(out, k) for k in PLANES}
        yard[chunks] = _yardstick(t, frame, pool, tr.iter)
        assert (out.rgb_bg is None) == with_mask and (yard[chunks]["rgb_bg"] is None) == with_mask
        for k in PLANES:
            g, y = got[chunks][k], yard[chunks][k]
            if g is None:
                continue
            assert g.dtype == torch.float32 and g.is_cuda and g.shape == ((3 if k.startswith("rgb") else 1), H, W), k
            assert bool(torch.isfinite(g).all()), k
            assert torch.equal(g, y), (chunks, k, float((g - y).abs().max()))
    # the frame holds rays with foreground samples and rays without: the centre hits the sphere, the corners miss it
    counts = yard[5]["counts"][0]
    print("rays with foreground samples: %d of %d; weight sum up to %.3f" % (int((counts > 0).sum()), H * W,
                                                                            float(got[5]["weights_sum"].max())))
    assert float(counts[H // 2, W // 2]) > 0 and all(float(counts[y, x]) == 0 for y in (0, H - 1) for x in (0, W - 1))
    assert float(got[5]["weights_sum"].max()) > 0 and float(got[5]["depth"].max()) > 0
    # two chunkings need not agree to the bit (the MLP dispatch picks kernel forms by batch size): the operator chain sets the
    # bar, entry by entry
    for k in PLANES:
        if got[5][k] is None:
            continue
        d_code, d_yard = (got[5][k] - got[19][k]).abs(), (yard[5][k] - yard[19][k]).abs()
        print("%s: five chunks against nineteen: the renderer moves by %.3e, the operator chain by %.3e"
              % (k, float(d_code.max()), float(d_yard.max())))
        assert bool((d_code <= 2 * d_yard).all()), k
    # no depth plane unless asked for, and the other planes are the same bits; `it` None is the trainer's iteration
    plain = rnd.render(frame, pool_samples=POOL_5)
    assert plain.depth is None and torch.equal(plain.rgb, got[5]["rgb"]) and torch.equal(plain.weights_sum, got[5]["weights_sum"])
    assert torch.equal(rnd.render(frame, it=tr.iter, pool_samples=POOL_5).rgb, plain.rgb)
    if not with_mask:      # another iteration selects another window of the background net (open after 10 000 iterations)
        assert not torch.equal(rnd.render(frame, it=20000, pool_samples=POOL_5).rgb, plain.rgb)
        # a frame on another device than the models is refused before any launch
        from permuto_sdf_amd._lib import PsdfError
        with pytest.raises(PsdfError):
            rnd.render(render.Frame(frame.K.cpu(), frame.tf_world_cam.cpu(), H, W))


def test_an_empty_grid_renders_the_background_alone(dev):
    from permuto_sdf_amd import render
    from permuto_sdf_amd.nerf_train import NerfTrainer
    tr = NerfTrainer(dev, hp=_hp(256), seed=3)
    tr.grid.set_grid_occupancy(torch.zeros_like(tr.grid.get_grid_occupancy()))
    out = tr.renderer().render(render.Frame.from_reel(_reel(dev), 0), pool_samples=POOL_5, depth=True)
    assert bool((out.weights_sum == 0).all()) and bool((out.depth == 0).all())
    assert torch.equal(out.rgb, out.rgb_bg) and float(out.rgb.abs().max()) > 0 and bool(torch.isfinite(out.rgb).all())


def test_rendering_leaves_a_run_as_it_was(dev):
    """Two trainers of one seed take 3 steps; one renders a frame; both take one more step on the same batch: the same loss,
    bit for bit.  (The lattice scatter adds with float atomics, in an order that differs from launch to launch: after the three
    steps the second trainer takes the first one's parameters and grid, as tests/test_gpu_nerf_train.py::_pair does.  The loss
    of a step is computed before its update, so nothing else of the optimiser enters it.)"""
    from permuto_sdf_amd import render
    from permuto_sdf_amd.nerf_train import NerfTrainer
    reel = _reel(dev)
    a, b = (NerfTrainer(dev, hp=_hp(256), seed=5) for _ in range(2))
    for _ in range(3):
        batch = a.draw(reel)
        a.step(batch=batch)
        b.step(batch=batch)
    for n_a, n_b in zip(a.nets, b.nets):
        n_b.load_state_dict(n_a.state_dict())
    b.grid.set_grid_values(a.grid.get_grid_values().clone())
    b.grid.set_grid_occupancy(a.grid.get_grid_occupancy().clone())

    def snapshot():
        torch.cuda.synchronize()
        return dict(params=[p.detach().clone() for p in a.params],
                    grads=[None if p.grad is None else p.grad.detach().clone() for p in a.params],
                    grad_ids=[None if p.grad is None else id(p.grad) for p in a.params],
                    moments=[v.clone() for p in a.params for k, v in sorted(a.opt.state.get(p, {}).items()) if torch.is_tensor(v)],
                    touched=[(tr.touched.clone(), tr.grad.clone()) for tr in a.touched],
                    grid=(a.grid.get_grid_values().clone(), a.grid.get_grid_occupancy().clone()),
                    scalars=(a.iter, a.grid.max_nr_samples, [n.training for n in a.nets]), rng=torch.cuda.get_rng_state(dev))

    before = snapshot()
    assert any(g is not None for g in before["grads"]) and len(before["moments"]) >= 2 * len(a.params)
    out = a.renderer().render(render.Frame.from_reel(reel, 0), pool_samples=POOL_19, depth=True)
    assert bool(torch.isfinite(out.rgb).all()) and float(out.weights_sum.max()) > 0
    after = snapshot()
    for k in ("params", "moments"):
        assert len(before[k]) == len(after[k]) and all(torch.equal(x, y) for x, y in zip(before[k], after[k])), k
    assert before["grad_ids"] == after["grad_ids"]
    assert all((x is None and y is None) or torch.equal(x, y) for x, y in zip(before["grads"], after["grads"]))
    assert all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(before["touched"], after["touched"]))
    assert torch.equal(before["grid"][0], after["grid"][0]) and torch.equal(before["grid"][1], after["grid"][1])
    assert before["scalars"] == after["scalars"] and before["scalars"][0] == 3
    assert torch.equal(before["rng"], after["rng"])
    # and the run goes on as the one that did not render
    batch = a.draw(reel)
    la, lb = a.step(batch=batch), b.step(batch=batch)
    assert math.isfinite(float(la)) and torch.equal(la, lb), (float(la), float(lb))


def test_a_checkpoint_renders_what_its_trainer_renders_and_views_go_into_the_scores(dev, trained, tmp_path):
    from permuto_sdf_amd import image_eval, nerf_view, render
    tr, reel = trained
    frame = render.Frame.from_reel(reel, 2)
    tr.save_checkpoint(str(tmp_path))
    ck = nerf_view.NerfFrameRenderer.from_checkpoint(str(tmp_path), dev)
    # the files do not hold the iteration: given the trainer's, the checkpoint renders the trainer's bits; given none, it opens
    # every lattice level
    a = tr.renderer().render(frame, it=tr.iter, depth=True)
    b = ck.render(frame, it=tr.iter, depth=True)
    for k in PLANES:
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert torch.equal(ck.render(frame).rgb, tr.renderer().render(frame, it=nerf_view.IT_WINDOW_OPEN).rgb)
    masked = nerf_view.NerfFrameRenderer.from_checkpoint(str(tmp_path), dev, with_mask=True).render(frame, it=tr.iter)
    assert masked.rgb_bg is None and torch.equal(masked.weights_sum, a.weights_sum)
    # views of two frames, straight into the scores
    rnd = tr.renderer()
    views = rnd.render_views([render.Frame.from_reel(reel, i) for i in (0, 3)])
    assert views.shape == (2, 3, H, W) and views.dtype == torch.float32 and views.is_cuda
    assert float(views.min()) >= 0.0 and float(views.max()) <= 1.0 and not torch.equal(views[0], views[1])
    psnr, ssim = image_eval.evaluate_views(views, views)
    assert psnr.shape == (2,) and ssim.shape == (2,)
    assert float((psnr - 80.0).abs().max()) <= 1e-9 and float((ssim - 1.0).abs().max()) <= 1e-9
    with pytest.raises(ValueError):
        rnd.render_views([])


def test_training_on_a_constant_colour_raises_the_psnr_of_a_view(dev):
    """60 steps at 256 rays on a constant-colour reel (test_gpu_nerf_train.py::test_trainer_learns_a_constant_colour shows that
    the loss falls): the PSNR of view 0 is higher than the untrained trainer's, strictly and without a margin.
    On an MI355X: 10.36 dB untrained, 27.52 dB after the 60 steps."""
    from permuto_sdf_amd import image_eval, render
    from permuto_sdf_amd.nerf_train import NerfTrainer
    reel = _reel(dev, constant=True)
    frame = render.Frame.from_reel(reel, 0)
    tr = NerfTrainer(dev, hp=_hp(256))
    gt = reel.rgb_reel[0:1]
    before = float(image_eval.evaluate_views(tr.renderer().render_views([frame]), gt)[0][0])
    for _ in range(60):
        tr.step(reel)
    after = float(image_eval.evaluate_views(tr.renderer().render_views([frame]), gt)[0][0])
    print("PSNR of view 0: untrained %.2f dB, after 60 steps %.2f dB" % (before, after))
    assert math.isfinite(before) and math.isfinite(after) and after > before
