"""GPU: the hand-written training step of a `--with_mask` run (train_manual.ManualTrainer(with_mask=True): the render with the
per-ray weight sum and the colour + mask loss tail of csrc/neus_render.hip) against the autograd trainer on the same batch.

The reel carries a mask: a disc in `mask_reel`, `has_mask` set, so the batch's gt_mask holds zeros and ones and the ground-truth
colours are masked as the reference's loader masks them.  The bars of the gradient comparison are those of
tests/test_gpu_train_step.py::test_manual_backward_equals_autograd, mode by mode: they were measured for the unmasked step (run-to-
run noise of the float atomics, the ill-conditioned curvature term) and nothing of that changes under a mask."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

NEW = ("psdf_neus_render_forward", "psdf_neus_render_backward", "psdf_neus_mask_loss")


def _masked_reel(dev, nr_images=4, height=60, width=80, colour=None):
    from permuto_sdf_amd.train_step import SyntheticReel
    reel = SyntheticReel(dev, nr_images=nr_images, height=height, width=width)
    yy, xx = torch.meshgrid(torch.arange(height, device=dev), torch.arange(width, device=dev), indexing="ij")
    disc = (((yy - height / 2) ** 2 + (xx - width / 2) ** 2) <= (height / 3) ** 2).float()
    reel.mask_reel[:] = disc.view(1, 1, height, width)
    reel.has_mask = True
    if colour is not None:
        reel.rgb_reel[:] = torch.tensor(colour, device=dev).view(1, 3, 1, 1)
    return reel


def _record_calls(monkeypatch):
    from permuto_sdf_amd import _lib as L
    names, orig = [], L.call

    def call(name, *args):
        names.append(name)
        return orig(name, *args)
    monkeypatch.setattr(L, "call", call)
    return names


def _hp(reference_schedule=False, late=False, nr_rays=256):
    from permuto_sdf_amd.train_step import HyperParams
    hp = HyperParams()
    hp.nr_rays, hp.target_nr_of_samples = nr_rays, nr_rays * 96
    if reference_schedule:
        hp.nr_iter_sphere_fit, hp.lr_warmup_iters = 0, 4       # straight into the main phase, colour calibration on
    if late:   # the late phase: no curvature term, Lipschitz term on, weight decay on the colour lattice
        hp.iter_start_reduce_curv, hp.iter_finish_reduce_curv = -1, 0
    return hp


def _trainer_pair(dev, monkeypatch, reference_schedule, late=False, empty_grid=False):
    """tests/test_gpu_train_step.py::_trainer_pair with with_mask=True and a masked reel: the autograd trainer and the hand-written
    one, same seed, same first iteration (the samplers' process-global generators are rewound in between) -> per trainer (trainer,
    captured gradients, the batch's gt_mask, how often Trainer._main_phase ran, the library calls of the step)"""
    from permuto_sdf_amd.bridge import OccupancyGrid, RaySampler, VolumeRendering
    from permuto_sdf_amd.train_manual import ManualTrainer
    from permuto_sdf_amd.train_step import Trainer
    reel = _masked_reel(dev)
    owners = (OccupancyGrid, RaySampler, VolumeRendering)
    saved = [copy.deepcopy(c._rng) for c in owners]
    autograd_phase = []
    orig_phase = Trainer._main_phase

    def phase(self, *a, **k):
        autograd_phase.append(type(self).__name__)
        return orig_phase(self, *a, **k)
    monkeypatch.setattr(Trainer, "_main_phase", phase)
    calls = _record_calls(monkeypatch)
    out = []
    for cls in (Trainer, ManualTrainer):
        for c, r in zip(owners, saved):
            c._rng = copy.deepcopy(r)
        tr = cls(dev, _hp(reference_schedule, late), reference_schedule=reference_schedule, nr_images=4, with_mask=True)
        if empty_grid:
            tr.grid.set_grid_occupancy(torch.zeros_like(tr.grid.get_grid_occupancy()))
        masks = []
        draw = tr._draw_rays          # (an instance attribute: ManualTrainer then draws its rays itself, without the prefetch)
        tr._draw_rays = lambda r, draw=draw, masks=masks: (lambda rays: (masks.append(rays[5]), rays)[1])(draw(r))
        tr.capture_grads = {}
        del autograd_phase[:], calls[:]
        tr.step(reel)
        out.append((tr, tr.capture_grads, masks[0], list(autograd_phase), list(calls)))
    return out


def _bg_dense(tr):
    """indices, in the captured dense gradients, of the background network's parameters"""
    buffered = {id(m.encoding.lattice_values) for m in (tr.sdf, tr.rgb, tr.bg)}
    dense = [p for p in tr.params if id(p) not in buffered]
    bg = {id(p) for p in tr.bg.parameters()}
    idx = [i for i, p in enumerate(dense) if id(p) in bg]
    assert idx
    return idx


def test_masked_runs_take_the_hand_written_step(dev, monkeypatch):
    """fails on a tree whose hand-written step refuses with_mask: the step is the autograd graph there"""
    (a, _, gm_a, phase_a, calls_a), (m, _, gm_m, phase_m, calls_m) = _trainer_pair(dev, monkeypatch, False)
    assert m._hand_written_step_applies() and m.with_mask
    assert phase_a == ["Trainer"] and phase_m == []                # Trainer._main_phase is never entered by the hand-written step
    for name in NEW:
        assert name in calls_m and name not in calls_a, name
    # no background work, no composite kernels, no stand-alone colour loss
    for name in ("psdf_nerf_composite_forward", "psdf_nerf_composite_backward", "psdf_neus_composite_forward",
                 "psdf_neus_composite_backward", "psdf_l1_loss", "psdf_samples_bg"):
        assert name not in calls_m, name
    assert calls_m.count("psdf_neus_render_forward") == 1 and calls_m.count("psdf_neus_mask_loss") == 1
    assert torch.equal(gm_a, gm_m) and bool((gm_m == 0).any()) and bool((gm_m == 1).any())     # zeros and ones in the batch's mask


@pytest.mark.parametrize("mode", ["steady", "reference_schedule", "late"])
def test_masked_manual_backward_equals_autograd(dev, monkeypatch, mode):
    (a, ga, gm_a, _, _), (m, gm, gm_m, phase_m, _) = _trainer_pair(dev, monkeypatch, mode == "reference_schedule", late=(mode == "late"))
    assert phase_m == [] and torch.equal(gm_a, gm_m) and bool((gm_m == 0).any()) and bool((gm_m == 1).any())
    assert a.last == m.last and a.last["nr_fg_samples"] > 0, (a.last, m.last)
    print("loss autograd %.7f hand-written %.7f" % (float(ga["loss"]), float(gm["loss"])))
    assert abs(float(ga["loss"]) - float(gm["loss"])) <= 1e-5 * max(1.0, abs(float(ga["loss"])))
    bg = _bg_dense(m)
    for i, (x, y) in enumerate(zip(ga["dense"], gm["dense"])):
        scale = float(x.abs().max())
        err = float((x - y).abs().max())
        if i in bg:        # no background model under a mask: exactly zero in both trainers
            assert scale == 0.0 and float(y.abs().max()) == 0.0, ("background gradient %d" % i, scale)
            continue
        tol = 2e-4 if mode == "late" else 2e-3        # test_manual_backward_equals_autograd's, mode by mode
        print("dense %d %s: error %.3g of scale %.3g" % (i, tuple(x.shape), err, scale))
        assert err <= tol * scale + 1e-9, ("dense gradient %d" % i, tuple(x.shape), err, scale)
    for i, (x, y) in enumerate(zip(ga["lattices"], gm["lattices"])):
        scale = float(x.abs().max())
        if i == 2:
            assert scale == 0.0 and float(y.abs().max()) == 0.0
            continue
        err = float((x - y).abs().max())
        rel = float((x - y).norm() / x.norm())
        tol_rel, tol_max = (2e-4, 1e-3) if (mode == "late" or i > 0) else (4e-3, 2e-2)
        print("lattice %d: max error %.3g of scale %.3g, relative L2 %.3g" % (i, err, scale, rel))
        assert scale > 0 and err <= tol_max * scale and rel <= tol_rel, ("lattice %d" % i, err, scale, rel)


def test_masked_step_without_foreground_samples(dev, monkeypatch):
    """an empty occupancy grid: the render is 0, 0 and the tail still runs -- both trainers agree, the loss holds the mask term,
    the colour and background lattices get nothing, the SDF lattice the off-surface term alone"""
    import math
    (a, ga, gm_a, _, _), (m, gm, gm_m, phase_m, calls_m) = _trainer_pair(dev, monkeypatch, False, empty_grid=True)
    assert phase_m == [] and a.last == m.last and m.last["nr_fg_samples"] == 0
    assert "psdf_neus_mask_loss" in calls_m and "psdf_neus_render_forward" not in calls_m and "psdf_neus_render_backward" not in calls_m
    la, lm = float(ga["loss"]), float(gm["loss"])
    assert math.isfinite(lm) and abs(la - lm) <= 1e-5 * max(1.0, abs(la))
    # weights_sum = 0 clips to 1e-3: BCE = -log(1e-3) on the rays inside the disc, -log(1 - 1e-3) outside, times mask_weight
    inside = float(gm_m.mean())
    mask_term = m.hp.mask_weight * (inside * -math.log(1e-3) + (1 - inside) * -math.log(1 - 1e-3))
    assert inside > 0 and lm > 0.99 * mask_term
    for (x, y) in zip(ga["dense"], gm["dense"]):
        assert float((x - y).abs().max()) <= 2e-3 * float(x.abs().max()) + 1e-9
    for g in (ga, gm):
        lat = g["lattices"]
        assert float(lat[1].abs().max()) == 0.0 and float(lat[2].abs().max()) == 0.0 and float(lat[0].abs().max()) > 0
    x, y = ga["lattices"][0], gm["lattices"][0]
    assert float((x - y).norm() / x.norm()) <= 2e-4


def test_masked_manual_trainer_learns_colour_and_mask(dev):
    """60 steps on a constant-colour reel whose mask is the disc: the loss falls by the criterion of
    test_manual_trainer_learns_constant_colour, and the rendered weight sums follow the mask"""
    from permuto_sdf_amd import neus
    from permuto_sdf_amd.train_manual import ManualTrainer
    tr = ManualTrainer(dev, _hp(), with_mask=True)
    reel = _masked_reel(dev, colour=[0.8, 0.3, 0.1])
    seen = []
    tail = neus.neus_mask_loss_raw
    import permuto_sdf_amd.train_manual as tm

    def tail_spy(pred, gt, hit, ws, gt_mask, *a, **k):
        seen.append((ws.detach().view(-1), gt_mask.detach().view(-1)))
        return tail(pred, gt, hit, ws, gt_mask, *a, **k)
    tm.neus_mask_loss_raw = tail_spy
    try:
        losses = [float(tr.step(reel)) for _ in range(60)]
    finally:
        tm.neus_mask_loss_raw = tail
    assert all(l == l and abs(l) < 1e3 for l in losses), losses
    assert sum(losses[-10:]) / 10 < 0.6 * sum(losses[:5]) / 5, (losses[:5], losses[-10:])
    ws = torch.cat([w for w, _ in seen[-5:]])
    gm = torch.cat([g for _, g in seen[-5:]])
    out_mean, in_mean = float(ws[gm == 0].mean()), float(ws[gm == 1].mean())
    print("mean weights_sum outside the mask %.4f, inside %.4f" % (out_mean, in_mean))
    assert out_mean < in_mean
    t = tr.sdf.encoding.touched_rows
    assert float(t.grad.abs().max()) == 0.0 and int(t.touched.sum()) == 0


def test_unmasked_step_keeps_its_library_calls(dev, monkeypatch):
    """one step of ManualTrainer(with_mask=False): none of the new entries, and the composite kernels and the colour loss it has
    always called"""
    from permuto_sdf_amd.train_manual import ManualTrainer
    from permuto_sdf_amd.train_step import SyntheticReel
    tr = ManualTrainer(dev, _hp())
    reel = SyntheticReel(dev, nr_images=4, height=60, width=80)
    calls = _record_calls(monkeypatch)
    tr.step(reel)
    assert tr.last["nr_fg_samples"] > 0
    for name in NEW:
        assert name not in calls, name
    for name in ("psdf_neus_composite_forward", "psdf_neus_composite_backward", "psdf_nerf_composite_forward",
                 "psdf_nerf_composite_backward", "psdf_l1_loss"):
        assert calls.count(name) == 1, (name, calls.count(name))
