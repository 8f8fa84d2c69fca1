"""The NeRF trainer's per-image colour calibration on the device (csrc/colorcal.hip, permuto_sdf_amd/nerf_train.py).

Containers of tests/colorcal_float64.py: rays of 0, 1, 15, 16, 17, 31, 32, 33, 64, 3 and 0 samples (every border of a 16-lane row, M
no multiple of 64), one ray of one sample, 5 x 32 in the equal-count form, a pool with slots no ray owns.  4 images, image 0 fixed,
no ray of image 3, one ray each with img_idx = -1 and = 4; tables of order 0.3, raw colours in +-6.

(a) the forward, every entry inside its float64 bar; (b) with zero tables the bits of sigmoid_rows_raw, with nonzero tables still
on the rays of the fixed image and of the images outside the tables; (c) g_raw_fm, g_ray and the folded [I, 3] pair inside their
bars with one branch and with two, the fixed and the undrawn image's rows exactly 0, unowned slots 0; (d) two calls, equal bits;
(e) the autograd Function against the operator chain over train_step.Colorcal; (f) a hand-written against an autograd
NerfTrainer(nr_images=4), to the bars of tests/test_gpu_nerf_train.py; (g) the fixed image's rows stay exactly 0 through 30 steps,
another image's move; (h) the checkpoint writes colorcal_model.pt and reproduces the next loss; (i) nr_images=None issues none of
the new library calls, nr_images=4 issues them in the plain sigmoid's place."""
import math
import os

import pytest
import torch

from tests import colorcal_float64 as ev
from tests.float64_check import check, show

pytestmark = pytest.mark.gpu
NEW = ("psdf_colorcal_sigmoid_forward", "psdf_colorcal_sigmoid_backward", "psdf_colorcal_fold")


def _nt():
    from permuto_sdf_amd import nerf_train
    return nerf_train


def make_rs(c, dev):
    from permuto_sdf_amd.bridge import RaySamplesPacked
    rs = RaySamplesPacked(c["R"], c["M"], device=dev)
    rs.ray_start_end_idx = c["start_end"].to(dev)
    if c["equal"]:
        rs.rays_have_equal_nr_of_samples, rs.fixed_nr_of_samples_per_ray = True, c["fixed"]
    rs.cur_nr_samples.fill_(int(c["counts"].sum()))
    return rs


def _module(dev, wd, bias):
    from permuto_sdf_amd.train_step import Colorcal
    cc = Colorcal(ev.NR_IMAGES, ev.IDX_FIXED).to(dev)
    with torch.no_grad():
        cc.weight_delta.copy_(wd)
        cc.bias.copy_(bias)
    return cc


def _case(cname, dev, seed=0, zero_tables=False):
    c = ev.container(cname)
    raw_fm, g_rgb, wd, bias = ev.family(c, seed, zero_tables)
    return c, make_rs(c, dev), raw_fm, g_rgb, wd, bias, _module(dev, wd, bias), c["img_idx"].to(dev)


def _identity_samples(c):
    img = c["img_idx"].long()[c["ray_of"].clamp_min(0)]
    return (c["ray_of"] >= 0) & ((img == ev.IDX_FIXED) | (img < 0) | (img >= ev.NR_IMAGES))


# ------------------------------------------------------------------------------------------------------------ (a), (b)
@pytest.mark.parametrize("cname", ev.CONTAINERS)
def test_forward_against_float64_and_the_identity_bits(dev, cname):
    nt = _nt()
    from permuto_sdf_amd.neus import sigmoid_rows_raw
    c, rs, raw_fm, _, wd, bias, cc, img = _case(cname, dev)
    owned = c["ray_of"] >= 0
    rgb = nt.colorcal_sigmoid_raw(rs, raw_fm.to(dev), img, cc)
    out = []
    val, bar = ev.forward(c, raw_fm, c["img_idx"], wd, bias)
    check(out, "rgb", torch.where(owned[:, None].to(dev), rgb, torch.zeros_like(rgb)), val, bar)
    show(cname, out)
    plain = sigmoid_rows_raw(raw_fm.to(dev))
    keep = _identity_samples(c).to(dev)
    assert torch.equal(rgb[keep].view(torch.int32), plain[keep].view(torch.int32))
    if cname == "rows":
        assert int(keep.sum()) == 1 + 17 + 32 + 33              # the fixed image's two rays, img_idx -1 and img_idx I
    if cname == "gap":
        assert not bool(rgb[~owned.to(dev)].any())              # what no ray owns is not written: the zeros of the allocation
    # zero tables: the plain sigmoid's bits on every owned sample
    c, rs, raw_fm, _, wd, bias, cc, img = _case(cname, dev, zero_tables=True)
    rgb0 = nt.colorcal_sigmoid_raw(rs, raw_fm.to(dev), img, cc)
    o = owned.to(dev)
    assert torch.equal(rgb0[o].view(torch.int32), sigmoid_rows_raw(raw_fm.to(dev))[o].view(torch.int32))


# ------------------------------------------------------------------------------------------------------------ (c), (d)
@pytest.mark.parametrize("cname", ev.CONTAINERS)
def test_backward_and_fold_against_float64_and_twice_the_same_bits(dev, cname):
    nt = _nt()
    c, rs, raw_fm, g_rgb, wd, bias, cc, img = _case(cname, dev, seed=2)
    raw_d, g_d = raw_fm.to(dev), g_rgb.to(dev)
    rgb = nt.colorcal_sigmoid_raw(rs, raw_d, img, cc)
    owned = (c["ray_of"] >= 0).to(dev)
    rgb = torch.where(owned[:, None], rgb, torch.zeros_like(rgb))
    g_raw_fm, g_ray = nt.colorcal_sigmoid_backward_raw(rs, g_d, rgb, raw_d, img, cc)
    back = ev.backward(c, g_rgb, rgb, raw_fm, c["img_idx"], wd, bias)           # handed the kernel's own fp32 rgb
    out = []
    check(out, "g_raw_fm", g_raw_fm, *back["g_raw_fm"])
    check(out, "g_ray", g_ray, *back["g_ray"])
    assert not bool(g_raw_fm[:, ~owned].any())                                  # slots no ray owns
    idle = (c["counts"] == 0) | (c["img_idx"] == ev.IDX_FIXED) | (c["img_idx"] < 0) | (c["img_idx"] >= ev.NR_IMAGES)
    assert not bool(g_ray[idle.to(dev)].any())                                  # exactly 0: empty rays, rays that keep the identity
    # the fold, one branch
    g_wd, g_b = nt.colorcal_fold_raw(img, cc, g_ray)
    one = ev.fold(c["img_idx"], [back["g_ray"]])
    check(out, "g_weight_delta", g_wd, *one["g_weight_delta"])
    check(out, "g_bias", g_b, *one["g_bias"])
    # two branches: a second upstream gradient on the same container stands in for the background's
    g2 = torch.randn(c["M"], 3, generator=torch.Generator().manual_seed(99))
    _, g_ray2 = nt.colorcal_sigmoid_backward_raw(rs, g2.to(dev), rgb, raw_d, img, cc)
    back2 = ev.backward(c, g2, rgb, raw_fm, c["img_idx"], wd, bias)
    g_wd2, g_b2 = nt.colorcal_fold_raw(img, cc, g_ray, g_ray2)
    two = ev.fold(c["img_idx"], [back["g_ray"], back2["g_ray"]])
    check(out, "g_weight_delta (two)", g_wd2, *two["g_weight_delta"])
    check(out, "g_bias (two)", g_b2, *two["g_bias"])
    show(cname, out)
    for t in (g_wd, g_b, g_wd2, g_b2):
        assert not bool(t[ev.IDX_FIXED].any()) and not bool(t[3].any())         # the fixed image, the image no ray drew
    # (d) the same inputs again: the same bits in every output
    again = nt.colorcal_sigmoid_backward_raw(rs, g_d, rgb, raw_d, img, cc)
    again_fold = nt.colorcal_fold_raw(img, cc, again[1], g_ray2)
    rgb_again = nt.colorcal_sigmoid_raw(rs, raw_d, img, cc)
    for x, y in ((g_raw_fm, again[0]), (g_ray, again[1]), (g_wd2, again_fold[0]), (g_b2, again_fold[1]),
                 (rgb[owned], rgb_again[owned])):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------- (e)
@pytest.mark.parametrize("cname", ["rows", "equal32"])
def test_autograd_function_gives_the_operator_chains_gradients(dev, cname):
    nt = _nt()
    c, rs, raw_fm, g_rgb, wd, bias, cc, img = _case(cname, dev, seed=3)
    inside = img.clone()
    inside[(inside < 0) | (inside >= ev.NR_IMAGES)] = ev.IDX_FIXED               # the module cannot index outside its tables
    raw_a = raw_fm.to(dev).requires_grad_(True)
    rgb = nt.colorcal_sigmoid(rs, raw_a, img, cc)
    (rgb * g_rgb.to(dev)).sum().backward()
    got = raw_a.grad.clone(), cc.weight_delta.grad.clone(), cc.bias.grad.clone()
    cc.weight_delta.grad = cc.bias.grad = None
    raw_b = raw_fm.to(dev).t().contiguous().requires_grad_(True)
    chain = torch.sigmoid(cc.calib_RGB_samples_packed(raw_b, inside, rs.ray_start_end_idx))
    (chain * g_rgb.to(dev)).sum().backward()
    want = raw_b.grad.t(), cc.weight_delta.grad, cc.bias.grad
    # both are held against ONE float64 evaluation of the whole chain (forward and backward together): the bars of (c), carrying
    # the forward's bar into the backward, since each backward starts from its own fp32 rgb
    fwd = ev.forward(c, raw_fm, c["img_idx"], wd, bias)
    back = ev.backward(c, g_rgb, fwd[0], raw_fm, c["img_idx"], wd, bias, rgb_bar=fwd[1])
    folded = ev.fold(c["img_idx"], [back["g_ray"]])
    out = []
    for tag, r, (g_raw, g_wd, g_b) in (("", rgb, got), (" (chain)", chain, want)):
        check(out, "rgb" + tag, r, *fwd)
        check(out, "g_raw_fm" + tag, g_raw, *back["g_raw_fm"])
        check(out, "g_weight_delta" + tag, g_wd, *folded["g_weight_delta"])
        check(out, "g_bias" + tag, g_b, *folded["g_bias"])
        assert not bool(g_wd[ev.IDX_FIXED].any()) and not bool(g_wd[3].any()) and not bool(g_b[ev.IDX_FIXED].any())
    show(cname, out)


# ------------------------------------------------------------------------------------------------------------------- (f)
def _reel(dev, **kw):
    from permuto_sdf_amd.train_step import SyntheticReel
    return SyntheticReel(dev, **{**dict(nr_images=4, height=60, width=80), **kw})


def _hp(nr_rays):
    hp = _nt().HyperParams()
    hp.nr_rays = nr_rays
    return hp


def _set_tables(trainers, seed=11):
    g = torch.Generator().manual_seed(seed)
    wd, bias = torch.randn(4, 3, generator=g) * 0.3, torch.randn(4, 3, generator=g) * 0.3
    for t in trainers:
        with torch.no_grad():
            t.colorcal.weight_delta.copy_(wd)
            t.colorcal.bias.copy_(bias)


def _pair(dev, with_mask, reel, preceding=2):
    """tests/test_gpu_nerf_train.py::_pair with nr_images=4: a hand-written and an autograd trainer with the same parameters and
    grid after `preceding` identical iterations, nonzero calibration tables, then ONE step of each form on the same batch"""
    nt = _nt()
    hand = nt.NerfTrainer(dev, with_mask=with_mask, hand_written=True, hp=_hp(256), seed=5, nr_images=4)
    auto = nt.NerfTrainer(dev, with_mask=with_mask, hand_written=True, hp=_hp(256), seed=5, nr_images=4)
    for x, y in zip(hand.params, auto.params):
        assert torch.equal(x, y)
    for _ in range(preceding):
        b = hand.draw(reel)
        hand.step(batch=b)
        auto.step(batch=b)
        for n_h, n_a in zip(hand.nets + [hand.colorcal], auto.nets + [auto.colorcal]):      # float atomics: the same parameters again
            n_a.load_state_dict(n_h.state_dict())
        auto.grid.set_grid_values(hand.grid.get_grid_values().clone())
        auto.grid.set_grid_occupancy(hand.grid.get_grid_occupancy().clone())
    _set_tables((hand, auto))
    auto.hand_written = False
    b = hand.draw(reel)
    hand.capture_grads, auto.capture_grads = {}, {}
    hand.step(batch=b)
    auto.step(batch=b)
    return hand, auto, b


@pytest.mark.parametrize("with_mask", [False, True])
def test_hand_written_calibrated_step_equals_the_autograd_step(dev, with_mask):
    reel = _reel(dev)
    if with_mask:
        reel.has_mask = True
        reel.mask_reel[..., reel.mask_reel.shape[-1] // 2:] = 0.0
    hand, auto, b = _pair(dev, with_mask, reel)
    assert b.n_fg > 0 and (b.bg is None) == with_mask and b.img_idx.shape == (256,)
    h, a = hand.capture_grads, auto.capture_grads
    lh, la = float(h["loss"]), float(a["loss"])
    print("loss hand-written %.9g autograd %.9g" % (lh, la))
    assert math.isfinite(lh) and abs(lh - la) <= 1e-5 * abs(la)
    assert len(h["dense"]) == len(a["dense"]) == (16 if with_mask else 30)
    for i, (gh, ga) in enumerate(zip(h["dense"], a["dense"])):
        scale, d = float(ga.abs().max()), float((gh - ga).abs().max())
        print("  dense %d %s: max |diff| / max |grad| %.2e" % (i, tuple(ga.shape), d / scale if scale else 0.0))
        assert d <= 2e-4 * scale, (i, d, scale)
    # the calibration's two gradients are the last two dense entries; the fixed image's rows are exactly 0 in both forms
    for g in h["dense"][-2:] + a["dense"][-2:]:
        assert g.shape == (4, 3) and not bool(g[0].any()) and bool(g[1:].any())
    assert hand.dense[-2] is hand.colorcal.weight_delta and hand.dense[-1] is hand.colorcal.bias


# ------------------------------------------------------------------------------------------------------------------- (g)
def test_fixed_image_stays_at_the_identity_while_a_darkened_image_is_calibrated(dev):
    reel = _reel(dev)
    reel.rgb_reel[:] = torch.tensor([0.8, 0.5, 0.3], device=dev).view(1, 3, 1, 1)
    reel.rgb_reel[2] *= 0.5                                  # image 2: the same scene at half the exposure
    tr = _nt().NerfTrainer(dev, hp=_hp(256), nr_images=4, idx_with_fixed_calib=0)
    for _ in range(30):
        loss = tr.step(reel)
    assert math.isfinite(float(loss))
    cc = tr.colorcal
    assert not bool(cc.weight_delta[0].any()) and not bool(cc.bias[0].any())
    assert bool(cc.weight_delta[2].any()) and bool(cc.bias[2].any())
    print("after 30 steps: bias %s" % cc.bias.detach().cpu().numpy().round(4).tolist())


# ------------------------------------------------------------------------------------------------------------------- (h)
def test_checkpoint_round_trip_with_calibration(dev, tmp_path):
    nt = _nt()
    reel = _reel(dev)
    tr = nt.NerfTrainer(dev, hp=_hp(128), seed=3, nr_images=4)
    for _ in range(3):
        tr.step(reel)
    assert bool(tr.colorcal.bias[1:].any())
    folder = str(tmp_path / "models")
    tr.save_checkpoint(folder)
    assert sorted(os.listdir(folder)) == sorted(["nerf_hash_model.pt", "nerf_hash_model_bg.pt", "grid_values.pt", "grid_occupancy.pt",
                                                 "colorcal_model.pt"])
    sd = torch.load(os.path.join(folder, "colorcal_model.pt"))
    assert sorted(sd) == ["bias", "weight_delta"] and tuple(sd["bias"].shape) == (4, 3)
    other = nt.NerfTrainer(dev, hp=_hp(128), seed=77, nr_images=4)
    other.load_checkpoint(folder)
    for x, y in zip(other.params, tr.params):
        assert torch.equal(x, y)
    other.iter = tr.iter
    b = tr.draw(reel)
    assert float(other.step(batch=b)) == float(tr.step(batch=b))
    # a checkpoint of a run without calibration loads into a calibrated trainer, whose tables stay at zero
    plain = nt.NerfTrainer(dev, hp=_hp(128), seed=3)
    plain.step(reel)
    folder2 = str(tmp_path / "plain")
    plain.save_checkpoint(folder2)
    assert "colorcal_model.pt" not in os.listdir(folder2)
    fresh = nt.NerfTrainer(dev, hp=_hp(128), seed=78, nr_images=4)
    fresh.load_checkpoint(folder2)
    assert torch.equal(fresh.net.mlp_rgb.layers[0].weight, plain.net.mlp_rgb.layers[0].weight)
    assert not bool(fresh.colorcal.weight_delta.any()) and not bool(fresh.colorcal.bias.any())


# ------------------------------------------------------------------------------------------------------------------- (i)
def _calls_of_one_step(monkeypatch, dev, reel, **kw):
    from permuto_sdf_amd import _lib as L
    tr = _nt().NerfTrainer(dev, hp=_hp(64), seed=1, **kw)
    tr.step(reel)                                            # iteration 0 refreshes the grid; record iteration 1
    names, real = [], L.call

    def recording(name, *args):
        names.append(name)
        return real(name, *args)
    monkeypatch.setattr(L, "call", recording)
    tr.step(reel)
    monkeypatch.setattr(L, "call", real)
    return names


def test_default_keyword_issues_none_of_the_new_calls(dev, monkeypatch):
    reel = _reel(dev)
    plain = _calls_of_one_step(monkeypatch, dev, reel)
    assert plain.count("psdf_sigmoid_rows") == 2 and plain.count("psdf_sigmoid_rows_backward") == 2
    assert not [n for n in plain if n in NEW]
    assert plain == _calls_of_one_step(monkeypatch, dev, reel, nr_images=None)
    cal = _calls_of_one_step(monkeypatch, dev, reel, nr_images=4)
    assert cal.count(NEW[0]) == 2 and cal.count(NEW[1]) == 2 and cal.count(NEW[2]) == 1
    assert "psdf_sigmoid_rows" not in cal and "psdf_sigmoid_rows_backward" not in cal
    # the calibrated step IS the plain step with the sigmoids exchanged, one fold and the optimiser's two more tensors
    swap = {"psdf_sigmoid_rows": NEW[0], "psdf_sigmoid_rows_backward": NEW[1]}
    core = [n for n in cal if n != NEW[2] and not n.startswith("psdf_adamw")]
    assert core == [swap.get(n, n) for n in plain if not n.startswith("psdf_adamw")]
