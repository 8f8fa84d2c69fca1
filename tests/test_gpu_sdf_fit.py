"""SDF fitting from oriented points on the device (permuto_sdf_amd/sdf_fit.py, csrc/sdf_fit.hip).

(a) the batch kernel against index_select and the affine map in torch, bit for bit, an index of M and of -1 clamped;
(b) one hand-written step against the same step as an autograd graph, on the same batch after one identical preceding step, for
    P in {3, 4} at 300 + 3000 rows: loss to 1e-5 relative, every dense gradient within 2e-4 of its largest entry, the lattice
    buffer within 2e-4 relative L2 and 1e-3 of its largest entry -- the tolerances of
    test_gpu_train_step.py::test_manual_backward_equals_autograd without its curvature term, for its reason: the lattice scatter
    adds with float atomics, in an order that differs from launch to launch;
(c) a fit of an analytic torus (major radius 0.3, minor 0.12, 20 000 points with outward normals, box [-0.5, 0.5]^3): finite
    losses, the mean of the last ten below 0.6 of the mean of the first five (the ratio of
    test_manual_trainer_learns_constant_colour), and a mean |sdf| on 5000 held-out surface points of at most twice the autograd
    fitter's at the same step count, seed and learning rate (the trajectories separate chaotically once atomic order differs:
    equality is not expected; FIT_LR below says why the rate is 1e-4 here);
(d) a 4-D fit of a sphere whose radius grows from 0.2 at time 0 to 0.3 at time 1: the same loss condition, non-empty meshes of
    both time slices at 64^3 with mean vertex radii ordered as the slices are;
(e) the fitted 3-D net through MeshExtractor.from_sdf_net, and a checkpoint round trip that reproduces sdf_only bit for bit."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

STEPS = 300
C2F = 150             # nr_iters_for_c2f, shortened: the lattice window is fully open half-way through the fit
# The learning rate of the torus fit (c).  At the reference's 1e-3 AdamW moves the last bias -- the field's offset -- by about the
# rate per step, in the direction of the sign of the surface term's gradient: measured over the last 20 of 300 steps, the held-out
# mean |sdf| of EITHER fitter then spans 0.0002 - 0.002 (profiles/sdf_fit_parity.json, LABNOTES.md), so the value after one
# particular step is a sample of that jitter, not a property of the step's code.  At 1e-4 the same spread is 0.00048 - 0.00055 for
# both fitters (a factor 1.15, against the 2 the comparison allows) and the loss still falls to 0.14 of its start.  The 4-D fit
# (d) has no such comparison and runs at the reference's rate.
FIT_LR = 1e-4
R_MAJOR, R_MINOR = 0.3, 0.12


def _sf():
    from permuto_sdf_amd import sdf_fit
    return sdf_fit


def torus(count, seed, dev):
    """points and outward unit normals of the torus around the z axis"""
    gen = torch.Generator().manual_seed(seed)
    u, v = (torch.rand(count, generator=gen, dtype=torch.float64) * 2 * math.pi for _ in range(2))
    ring = R_MAJOR + R_MINOR * torch.cos(v)
    p = torch.stack([ring * torch.cos(u), ring * torch.sin(u), R_MINOR * torch.sin(v)], 1)
    n = torch.stack([torch.cos(v) * torch.cos(u), torch.cos(v) * torch.sin(u), torch.sin(v)], 1)
    return p.float().to(dev), n.float().to(dev)


def sphere(count, radius, seed, dev):
    gen = torch.Generator().manual_seed(seed)
    n = torch.nn.functional.normalize(torch.randn(count, 3, generator=gen, dtype=torch.float64), dim=1)
    return (radius * n).float().to(dev), n.float().to(dev)


# ------------------------------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("P", [3, 4])
@pytest.mark.parametrize("n_surf, n_off", [(0, 5), (5, 0), (63, 65), (257, 1000)])
def test_batch_kernel_is_index_select_and_the_affine_map_bit_for_bit(dev, P, n_surf, n_off):
    sf = _sf()
    gen = torch.Generator().manual_seed(11 + P)
    M = 37
    cloud = sf.OrientedCloud(torch.randn(M, P, generator=gen), torch.randn(M, 3, generator=gen)).to(dev)
    idx = torch.randint(M, (n_surf,), generator=gen).to(dev)
    u = torch.rand(n_off, P, generator=gen).to(dev)
    lo, hi = [-0.5, -0.25, 0.125, 0.0][:P], [0.5, 0.75, 0.375, 1.0][:P]
    points, normals = sf.sdf_fit_batch_raw(cloud, idx, u, lo, hi)
    want_p, want_n = sf.sdf_fit_batch_torch(cloud, idx, u, lo, hi)
    assert points.shape == (n_surf + n_off, P) and normals.shape == (n_surf, 3)
    assert torch.equal(points, want_p) and torch.equal(normals, want_n)
    if P == 4 and n_off:      # lo = 0, hi = 1 in the time column: u itself
        assert torch.equal(points[n_surf:, 3], u[:, 3])
    if n_surf >= 5:           # indices outside the cloud read its first / last row, nothing else
        bad = idx.clone()
        bad[0], bad[1], bad[2], bad[3] = M, -1, 2 ** 62, -2 ** 62
        points, normals = sf.sdf_fit_batch_raw(cloud, bad, u, lo, hi)
        ok = bad.clamp(0, M - 1)
        want_p, want_n = sf.sdf_fit_batch_torch(cloud, ok, u, lo, hi)
        assert ok[:4].tolist() == [M - 1, 0, M - 1, 0]
        assert torch.equal(points, want_p) and torch.equal(normals, want_n)


# ------------------------------------------------------------------------------------------------------------------- (b)
def _cloud(P, dev):
    sf = _sf()
    if P == 3:
        return sf.OrientedCloud(*torus(20000, 1, dev))
    return sf.OrientedCloud.stack_in_time([sf.OrientedCloud(*sphere(10000, 0.2, 2, dev)), sf.OrientedCloud(*sphere(10000, 0.3, 3, dev))])


@pytest.mark.parametrize("P", [3, 4])
def test_hand_written_step_equals_the_autograd_step(dev, P):
    sf = _sf()
    cloud = _cloud(P, dev)
    kw = dict(n_surf=300, n_off=3000, nr_iters_for_c2f=C2F, seed=5)
    hand, auto = sf.SdfFitter(cloud, hand_written=True, **kw), sf.SdfFitter(cloud, hand_written=False, **kw)
    for a, b in zip(hand.net.parameters(), auto.net.parameters()):
        assert torch.equal(a, b)
    # one identical preceding step: the same batch through the same (hand-written) code, then the same parameters
    first = hand.draw()
    auto.hand_written = True
    hand.step(first)
    auto.step(first)
    auto.hand_written = False
    auto.net.load_state_dict(hand.net.state_dict())
    batch = hand.draw()
    hand.capture_grads, auto.capture_grads = {}, {}
    hand.step(batch)
    auto.step(batch)
    h, a = hand.capture_grads, auto.capture_grads
    lh, la = float(h["loss"]), float(a["loss"])
    print("P %d: loss hand-written %.9g autograd %.9g" % (P, lh, la))
    assert math.isfinite(lh) and abs(lh - la) <= 1e-5 * abs(la)
    assert len(h["dense"]) == len(a["dense"]) == 8
    for i, (gh, ga) in enumerate(zip(h["dense"], a["dense"])):
        scale = float(ga.abs().max())
        assert scale > 0
        d = float((gh - ga).abs().max())
        print("  dense %d %s: max |diff| / max |grad| %.2e" % (i, tuple(ga.shape), d / scale))
        assert d <= 2e-4 * scale, (i, d, scale)
    gh, ga = h["lattice"].double(), a["lattice"].double()
    assert float(ga.abs().max()) > 0
    rel_l2 = float((gh - ga).norm() / ga.norm())
    rel_max = float((gh - ga).abs().max() / ga.abs().max())
    print("  lattice: relative L2 %.2e, max |diff| / max |grad| %.2e" % (rel_l2, rel_max))
    assert rel_l2 <= 2e-4 and rel_max <= 1e-3
    # the step left nothing behind: buffers cleared for the next one
    assert not bool(hand.grad_buffer.flat.any()) and not bool(hand.touched.grad.any())


# ------------------------------------------------------------------------------------------------------------- (c), (e)
def _fit(fitter, steps):
    losses = [fitter.step() for _ in range(steps)]
    return torch.cat(losses).cpu().double()        # the one read-back, after the last step


@pytest.fixture(scope="module")
def torus_fits(dev):
    sf = _sf()
    cloud = sf.OrientedCloud(*torus(20000, 1, dev))
    held_out, _ = torus(5000, 99, dev)
    out = {}
    for name, hw in (("hand_written", True), ("autograd", False)):
        f = sf.SdfFitter(cloud, (-0.5, -0.5, -0.5), (0.5, 0.5, 0.5), nr_iters_for_c2f=C2F, hand_written=hw, seed=3, lr=FIT_LR)
        out[name] = (f, _fit(f, STEPS), float(f.surface_error(held_out)))
    return out


def _learns(losses):
    assert bool(torch.isfinite(losses).all())
    first, last = float(losses[:5].mean()), float(losses[-10:].mean())
    print("loss: first five %.6f, last ten %.6f (ratio %.3f)" % (first, last, last / first))
    assert last < 0.6 * first, (first, last)


def test_torus_fit_learns_and_matches_the_autograd_fitter(torus_fits):
    (f, losses, err), (_, losses_a, err_a) = torus_fits["hand_written"], torus_fits["autograd"]
    assert f.iter == STEPS and f.last_terms.shape == (4,)
    _learns(losses)
    _learns(losses_a)
    print("mean |sdf| on 5000 held-out surface points after %d steps: hand-written %.5f, autograd %.5f" % (STEPS, err, err_a))
    assert math.isfinite(err) and err <= 2.0 * err_a


def test_fitted_net_is_extracted_and_checkpointed(torus_fits, dev, tmp_path):
    from permuto_sdf_amd.mesh import MeshExtractor
    sf = _sf()
    f = torus_fits["hand_written"][0]
    mesh = MeshExtractor.from_sdf_net(f.net, f.iter).extract(64, -0.5, 0.5)
    assert mesh.V.shape[0] > 0 and mesh.F.shape[0] > 0
    ring = (mesh.V[:, :2].norm(dim=1) - R_MAJOR)
    dist = (torch.sqrt(ring * ring + mesh.V[:, 2] ** 2) - R_MINOR).abs()
    print("%d vertices, %d faces; mean distance of a vertex to the torus %.4f" % (mesh.V.shape[0], mesh.F.shape[0], float(dist.mean())))
    cloud2 = sf.OrientedCloud.from_extracted(mesh)
    assert len(cloud2) == mesh.V.shape[0] and cloud2.pos_dim == 3
    pts = (torch.rand(4099, 3, device=dev) - 0.5)
    want = f.net.sdf_only(pts, f.iter)
    f.save_checkpoint(str(tmp_path / "models"))
    other = sf.SdfFitter(f.cloud, nr_iters_for_c2f=C2F, seed=77)
    assert not torch.equal(other.net.sdf_only(pts, f.iter), want)
    other.load_checkpoint(str(tmp_path / "models"))
    assert torch.equal(other.net.sdf_only(pts, f.iter), want)


# ------------------------------------------------------------------------------------------------------------------- (d)
def test_4d_fit_of_a_growing_sphere(dev):
    from permuto_sdf_amd.mesh import MeshExtractor
    sf = _sf()
    cloud = _cloud(4, dev)
    assert cloud.pos_dim == 4 and set(cloud.points[:, 3].tolist()) == {0.0, 1.0}
    f = sf.SdfFitter(cloud, (-0.5, -0.5, -0.5), (0.5, 0.5, 0.5), pos_dim=4, nr_iters_for_c2f=C2F, seed=4)
    assert f.n_off == 3000 and f.box_lo[3] == 0.0 and f.box_hi[3] == 1.0
    _learns(_fit(f, STEPS))
    radii = []
    for t in (0.0, 1.0):
        mesh = MeshExtractor(f.net.time_slice(t, f.iter), device=dev).extract(64, -0.5, 0.5)
        assert mesh.V.shape[0] > 0 and mesh.F.shape[0] > 0
        radii.append(float(mesh.V.norm(dim=1).mean()))
    print("mean vertex radius of the slices at t = 0, 1: %.4f, %.4f (fitted to 0.2, 0.3)" % tuple(radii))
    assert radii[0] < radii[1]
