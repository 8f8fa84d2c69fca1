"""NeRF training on the device (permuto_sdf_amd/nerf_train.py: NerfTrainer over csrc/nerf_render.hip).

(a) one hand-written step against the same step as an autograd graph over the operators the tree had before, on the same batch
    after identical preceding iterations, with the background net and under with_mask: loss to 1e-5 relative, every dense
    gradient within 2e-4 of its largest entry, the lattice buffers within 2e-4 relative L2 and 1e-3 of their largest entry -- the
    bars test_gpu_train_step.py::test_manual_backward_equals_autograd holds in its `late` mode, for its reason: the lattice
    scatter adds with float atomics, in an order that differs from launch to launch;
(b) 60 steps on a constant-colour SyntheticReel at 256 rays: finite losses, the mean of the last ten below 0.6 of the mean of the
    first five (the criterion of test_manual_trainer_learns_constant_colour);
(c) an empty grid -- no foreground samples -- still steps, and the two forms agree;
(d) the grid is refreshed on iterations 0, 8, ... and on no other, and the refresh changes the occupancy;
(e) a checkpoint in the reference's files reproduces the next step's loss; (f) colour calibration raises."""
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu


def _nt():
    from permuto_sdf_amd import nerf_train
    return nerf_train


def _reel(dev, constant=False, **kw):
    from permuto_sdf_amd.train_step import SyntheticReel
    reel = SyntheticReel(dev, **{**dict(nr_images=4, height=60, width=80), **kw})
    if constant:
        reel.rgb_reel[:] = torch.tensor([0.8, 0.3, 0.1], device=dev).view(1, 3, 1, 1)
    return reel


def _hp(nr_rays):
    hp = _nt().HyperParams()
    hp.nr_rays = nr_rays
    return hp


def _masked(reel):
    """a mask that is 1 left of the image's middle and 0 right of it"""
    reel.has_mask = True
    reel.mask_reel[..., reel.mask_reel.shape[-1] // 2:] = 0.0
    return reel


def _compare(h, a, nr_lattices, nr_dense):
    lh, la = float(h["loss"]), float(a["loss"])
    print("loss hand-written %.9g autograd %.9g" % (lh, la))
    assert math.isfinite(lh) and abs(lh - la) <= 1e-5 * abs(la)
    assert len(h["dense"]) == len(a["dense"]) == nr_dense
    for i, (gh, ga) in enumerate(zip(h["dense"], a["dense"])):
        scale = float(ga.abs().max())
        d = float((gh - ga).abs().max())
        print("  dense %d %s: max |diff| / max |grad| %.2e" % (i, tuple(ga.shape), d / scale if scale else 0.0))
        assert d <= 2e-4 * scale, (i, d, scale)
    assert len(h["lattices"]) == len(a["lattices"]) == nr_lattices
    for i, (gh, ga) in enumerate(zip(h["lattices"], a["lattices"])):
        gh, ga = gh.double(), ga.double()
        if float(ga.abs().max()) == 0.0:
            assert float(gh.abs().max()) == 0.0
            continue
        rel_l2 = float((gh - ga).norm() / ga.norm())
        rel_max = float((gh - ga).abs().max() / ga.abs().max())
        print("  lattice %d: relative L2 %.2e, max |diff| / max |grad| %.2e" % (i, rel_l2, rel_max))
        assert rel_l2 <= 2e-4 and rel_max <= 1e-3


def _pair(dev, with_mask, reel, empty_grid=False, preceding=2):
    """a hand-written and an autograd trainer with the same parameters and grid after `preceding` identical iterations
    (both run them through the hand-written code on the same batches), then ONE step of each form on the same batch"""
    nt = _nt()
    hand = nt.NerfTrainer(dev, with_mask=with_mask, hand_written=True, hp=_hp(256), seed=5)
    auto = nt.NerfTrainer(dev, with_mask=with_mask, hand_written=True, hp=_hp(256), seed=5)
    for x, y in zip(hand.params, auto.params):
        assert torch.equal(x, y)
    if empty_grid:
        for t in (hand, auto):
            t.grid.set_grid_occupancy(torch.zeros_like(t.grid.get_grid_occupancy()))
            t.hp.grid_refresh_every = 10 ** 9          # (iteration 0 would refresh it)
            t.iter = 1
    for _ in range(preceding):
        b = hand.draw(reel)
        hand.step(batch=b)
        auto.step(batch=b)
        for n_h, n_a in zip(hand.nets, auto.nets):      # float atomics: the same parameters again, bit for bit
            n_a.load_state_dict(n_h.state_dict())
        auto.grid.set_grid_values(hand.grid.get_grid_values().clone())
        auto.grid.set_grid_occupancy(hand.grid.get_grid_occupancy().clone())
    auto.hand_written = False
    b = hand.draw(reel)
    hand.capture_grads, auto.capture_grads = {}, {}
    hand.step(batch=b)
    auto.step(batch=b)
    return hand, auto, b


# ------------------------------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("with_mask", [False, True])
def test_hand_written_step_equals_the_autograd_step(dev, with_mask):
    reel = _reel(dev)
    if with_mask:
        _masked(reel)
    hand, auto, b = _pair(dev, with_mask, reel)
    assert b.n_fg > 0 and hand.last == auto.last and (b.bg is None) == with_mask
    _compare(hand.capture_grads, auto.capture_grads, nr_lattices=1 if with_mask else 2, nr_dense=14 if with_mask else 28)
    assert hand.last_terms.shape == (2,) and (float(hand.last_terms[1]) > 0) == with_mask
    assert abs(float(hand.last_terms[0]) - float(auto.last_terms[0])) <= 1e-5 * float(auto.last_terms[0])
    # the step left nothing behind: the lattice buffers are cleared for the next one
    for tr in hand.touched:
        assert not bool(tr.grad.any()) and int(tr.touched.sum()) == 0


# ------------------------------------------------------------------------------------------------------------------- (b)
@pytest.mark.parametrize("with_mask", [False, True])
def test_trainer_learns_a_constant_colour(dev, with_mask):
    # under with_mask nothing is rendered outside the bounding sphere, and a ray that misses it keeps -log(1e-3) of the mask term
    # for good: the cameras stand at 0.8, where the sphere (radius 0.5, 38.7 degrees) covers the whole 60 x 80 image (its corner is
    # 27.5 degrees off the axis), and the mask is 1 everywhere -- a target the foreground alone can reach
    reel = _reel(dev, constant=True, **(dict(dist=0.8) if with_mask else {}))
    tr = _nt().NerfTrainer(dev, with_mask=with_mask, hp=_hp(256))
    if with_mask:
        reel.has_mask = True
        assert bool((reel.mask_reel == 1).all()) and bool(tr.draw(reel).hit.all())
    losses = torch.cat([tr.step(reel) for _ in range(60)]).cpu().double()
    assert bool(torch.isfinite(losses).all())
    first, last = float(losses[:5].mean()), float(losses[-10:].mean())
    print("with_mask %d: loss first five %.5f, last ten %.5f (ratio %.3f); %d foreground samples in the last step"
          % (with_mask, first, last, last / first, tr.last["nr_fg_samples"]))
    assert last < 0.6 * first, (first, last)
    assert tr.iter == 60


# ------------------------------------------------------------------------------------------------------------------- (c)
@pytest.mark.parametrize("with_mask", [False, True])
def test_step_without_foreground_samples(dev, with_mask):
    reel = _reel(dev, nr_images=2, height=40, width=60)
    if with_mask:
        _masked(reel)
    hand, auto, b = _pair(dev, with_mask, reel, empty_grid=True, preceding=1)
    assert b.n_fg == 0 and hand.last["nr_fg_samples"] == 0
    h, a = hand.capture_grads, auto.capture_grads
    _compare(h, a, nr_lattices=1 if with_mask else 2, nr_dense=14 if with_mask else 28)
    assert float(h["lattices"][0].abs().max()) == 0.0                   # nothing rendered in the foreground
    assert all(float(g.abs().max()) == 0.0 for g in h["dense"][:14])
    if not with_mask:
        assert float(h["lattices"][1].abs().max()) > 0                  # the background carries the whole image


# ------------------------------------------------------------------------------------------------------------------- (d)
def test_grid_refresh_every_eighth_iteration(dev):
    tr = _nt().NerfTrainer(dev, with_mask=True, hp=_hp(64))
    reel = _masked(_reel(dev, nr_images=2, height=40, width=60))
    # from an empty grid, so that what a refresh does is seen: it marks the voxels it sampled (the density of a fresh net is
    # softplus(~0) = 0.7, far above the threshold 1e-3)
    tr.grid.set_grid_values(torch.zeros_like(tr.grid.get_grid_values()))
    tr.grid.set_grid_occupancy(torch.zeros_like(tr.grid.get_grid_occupancy()))
    changed = []
    for it in range(17):
        values, occ = tr.grid.get_grid_values().clone(), tr.grid.get_grid_occupancy().clone()
        tr.step(reel)
        changed.append((not torch.equal(values, tr.grid.get_grid_values()), not torch.equal(occ, tr.grid.get_grid_occupancy())))
    assert [i for i, (v, _) in enumerate(changed) if v] == [0, 8, 16], changed
    assert [i for i, (_, o) in enumerate(changed) if o] == [0, 8, 16], changed
    share = float(tr.grid.get_grid_occupancy().float().mean())
    print("occupied after three refreshes of 65 536 random voxels of 64^3: %.3f" % share)
    assert 0.3 < share < 0.7              # 65 536 draws of 262 144 voxels, three times: 1 - exp(-3 / 4) = 0.53 drawn at least once


# ------------------------------------------------------------------------------------------------------------------- (e)
@pytest.mark.parametrize("with_mask", [False, True])
def test_checkpoint_round_trip_reproduces_the_next_loss(dev, tmp_path, with_mask):
    nt = _nt()
    reel = _masked(_reel(dev)) if with_mask else _reel(dev)
    tr = nt.NerfTrainer(dev, with_mask=with_mask, hp=_hp(128), seed=3)
    for _ in range(3):
        tr.step(reel)
    folder = str(tmp_path / "models")
    tr.save_checkpoint(folder)
    want = sorted(["nerf_hash_model.pt", "grid_values.pt", "grid_occupancy.pt"] + ([] if with_mask else ["nerf_hash_model_bg.pt"]))
    assert sorted(os.listdir(folder)) == want
    sd = torch.load(os.path.join(folder, "nerf_hash_model.pt"))
    assert "mlp_feat_and_density.6.weight" in sd and "mlp_rgb.4.bias" in sd and "encoding.lattice_values" in sd     # the reference's keys
    other = nt.NerfTrainer(dev, with_mask=with_mask, hp=_hp(128), seed=77)
    assert not torch.equal(other.net.mlp_rgb.layers[0].weight, tr.net.mlp_rgb.layers[0].weight)
    other.load_checkpoint(folder)
    for x, y in zip(other.params, tr.params):
        assert torch.equal(x, y)
    assert torch.equal(other.grid.get_grid_occupancy(), tr.grid.get_grid_occupancy())
    # the next step's loss is computed before its optimiser update: the same batch through the loaded nets gives the same loss
    # (to the last bits that the lattice gather leaves alone: the forward has no atomics)
    other.iter = tr.iter
    b = tr.draw(reel)
    assert float(other.step(batch=b)) == float(tr.step(batch=b))


# ------------------------------------------------------------------------------------------------------------------- (f)
def test_colour_calibration_raises(dev):
    with pytest.raises(NotImplementedError):
        _nt().NerfTrainer(dev, colorcal=object())
