"""GPU: the image scores of permuto_sdf_amd/image_eval.py (csrc/image_eval.hip) against the float64 yardstick
tests/image_eval_reference.py, on every map entry and every score.

Bars.  Both sides are float64 and differ in summation order alone.
  * SSIM: a moment errs by at most about (24 + f^2) 2^-53 sum(w |t|) with sum(w |t|) <= 1 (two 11-tap passes and the f x f mean);
    the two ratios amplify that by at most 8 / c1 + 12 / c2 = 9.3e4: about 5e-10 with both sides counted.  Asserted: 1e-9 on
    every map entry and on every score.
  * PSNR: the mean squared error is a sum of non-negative terms, so its relative error is at most (partials + tree depth) 2^-53;
    through 10 / ln 10 that is below 1e-11 dB.  Asserted: 1e-9 dB.
With -s every case prints its worst error over the bar (LABNOTES.md holds a copy)."""
import numpy as np
import pytest
import torch

from tests import image_eval_reference as ref

pytestmark = pytest.mark.gpu

BAR = 1e-9


@pytest.fixture(scope="module")
def ie(dev):
    from permuto_sdf_amd import image_eval
    return image_eval


@pytest.fixture(scope="module")
def tile(ie):
    p = ie.SsimPlan(1, 1, 64, 64)
    return p.tile_h, p.tile_w


def device_image(a, dev, nhwc=False):
    """the array on the device, as it is (NCHW) or as an NHWC buffer behind a permuted view"""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    if nhwc:
        t = t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        assert not t.is_contiguous() or t.shape[1] == 1
    return t


def check(ie, dev, label, x, y, mask=None, data_range=1.0, nhwc=(False, False), **kw):
    """one case: psnr, ssim and the map against the yardstick; the second run gives the same bits"""
    tx, ty = device_image(x, dev, nhwc[0]), device_image(y, dev, nhwc[1])
    tm = None if mask is None else torch.from_numpy(mask).to(dev)
    ptr = tx.data_ptr()
    score, smap = ie.ssim(tx, ty, tm, data_range=data_range, reduction="none", return_map=True, **kw)
    db = ie.psnr(tx, ty, tm, data_range=data_range, reduction="none")
    score2, smap2 = ie.ssim(tx, ty, tm, data_range=data_range, reduction="none", return_map=True, **kw)
    db2 = ie.psnr(tx, ty, tm, data_range=data_range, reduction="none")
    assert score.dtype == smap.dtype == db.dtype == torch.float64 and score.is_cuda and db.is_cuda
    assert tx.data_ptr() == ptr
    assert torch.equal(score, score2) and torch.equal(smap, smap2) and torch.equal(db, db2), label + ": two runs differ"
    assert torch.equal(ie.ssim(tx, ty, tm, data_range=data_range, reduction="none", **kw), score)      # without the map
    want_score, want_map = ref.ssim(x, y, mask, data_range, **kw)
    want_db = ref.psnr(x, y, mask, data_range)
    assert smap.shape == want_map.shape and score.shape == want_score.shape and db.shape == want_db.shape
    e_map = float(np.abs(smap.cpu().numpy() - want_map).max())
    e_score = float(np.abs(score.cpu().numpy() - want_score).max())
    e_db = float(np.abs(db.cpu().numpy() - want_db).max())
    print("%-44s map %s: error / bar: map %.2e score %.2e psnr %.2e" % (label, tuple(want_map.shape[-2:]), e_map / BAR, e_score / BAR,
                                                                       e_db / BAR))
    assert e_map <= BAR and e_score <= BAR and e_db <= BAR, (label, e_map, e_score, e_db)
    assert np.isfinite(want_map).all()
    # the reductions
    assert abs(float(ie.ssim(tx, ty, tm, data_range=data_range, **kw)) - want_score.mean()) <= BAR
    assert abs(float(ie.psnr(tx, ty, tm, data_range=data_range)) - want_db.mean()) <= BAR


def test_one_map_entry_and_the_next_size(ie, dev):
    x, y = ref.scene(1, 1, 11, 11, seed=2)
    check(ie, dev, "11 x 11", x, y)
    x, y = ref.scene(3, 3, 12, 11, seed=3)
    check(ie, dev, "12 x 11, N 3, C 3, uint8 0/255 mask", x, y, ref.block_mask(3, 12, 11))


@pytest.mark.parametrize("which", ["th - 1", "th", "th + 1", "3 th + 1"])
def test_map_extents_around_the_tile(ie, dev, tile, which):
    """map extents of th - 1, th, th + 1 and 3 th + 1 rows, and the same for tw columns: a last tile that is one short, full,
    one entry wide, and more than one workgroup in both directions; the input forms rotate over the sizes"""
    th, tw = tile
    mh, mw = {"th - 1": (th - 1, tw - 1), "th": (th, tw), "th + 1": (th + 1, tw + 1), "3 th + 1": (3 * th + 1, 3 * tw + 1)}[which]
    H, W = mh + 10, mw + 10
    p = ie.SsimPlan(1, 1, H, W)
    assert (p.map_h, p.map_w, p.factor) == (mh, mw, 1) and (p.tiles_y, p.tiles_x) == (-(-mh // th), -(-mw // tw))
    if which == "th - 1":        # both uint8, both NHWC, graded float mask, N 1, C 3
        x, y = ref.scene(1, 3, H, W, seed=4)
        check(ie, dev, "th - 1: uint8, NHWC, graded mask", x, y, ref.graded_mask(1, H, W, 5), nhwc=(True, True))
    elif which == "th":          # float32 against uint8, NCHW, no mask, N 3, C 1
        x, y = ref.scene(3, 1, H, W, seed=6)
        check(ie, dev, "th: float32 / uint8", (x / np.float32(255)).astype(np.float32), y)
    elif which == "th + 1":      # unnormalised floats with data_range = 255, one of them NHWC, 0/255 mask, N 1, C 3
        x, y = ref.scene(1, 3, H, W, seed=7)
        check(ie, dev, "th + 1: data_range 255, NHWC / NCHW", x.astype(np.float32), y.astype(np.float32), ref.block_mask(1, H, W),
              data_range=255.0, nhwc=(True, False))
    else:                        # uint8 against float32, NHWC against NCHW, graded mask, N 3, C 3
        x, y = ref.scene(3, 3, H, W, seed=8)
        check(ie, dev, "3 th + 1: uint8 NHWC / float32 NCHW", x, (y / np.float32(255)).astype(np.float32),
              ref.graded_mask(3, H, W, 9), nhwc=(True, False))


def test_pooling_by_two_drops_a_remainder_column(ie, dev):
    x, y = ref.scene(1, 3, 384, 390, seed=1)
    assert ie.SsimPlan(1, 3, 384, 390).factor == 2 and ie.SsimPlan(1, 3, 384, 390).pooled_w == 195
    check(ie, dev, "384 x 390: f = 2, float32 NHWC / uint8", (x / np.float32(255)).astype(np.float32), y, ref.block_mask(1, 384, 390),
          nhwc=(True, False))
    # the other parameters reach the kernel: every wrong variant of the host test is a different, correct answer here
    for kw in (dict(kernel_sigma=1.0), dict(k2=0.3), dict(downsample=False), dict(kernel_size=9), dict(k1=0.05)):
        check(ie, dev, "384 x 390 C 1, %s" % kw, x[:, :1], y[:, :1], **kw)


def test_pooling_by_three_drops_rows_and_columns(ie, dev):
    x, y = ref.scene(1, 3, 641, 650, seed=1)
    p = ie.SsimPlan(1, 3, 641, 650)
    assert (p.factor, p.pooled_h, p.pooled_w) == (3, 213, 216)
    check(ie, dev, "641 x 650: f = 3, uint8, graded mask", x, y, ref.graded_mask(1, 641, 650, 2))


def test_hand_cases(ie, dev):
    c1 = 0.01 ** 2
    a, b = 0.25, 0.75
    x = torch.full((2, 3, 40, 50), a, dtype=torch.float32, device=dev)
    y = torch.full((2, 3, 40, 50), b, dtype=torch.float32, device=dev)
    score, smap = ie.ssim(x, y, reduction="none", return_map=True)
    want = (2 * a * b + c1) / (a * a + b * b + c1)
    assert float((smap - want).abs().max()) <= 1e-12 and float((score - want).abs().max()) <= 1e-12
    u, _ = ref.scene(2, 3, 40, 50, seed=3)
    t = torch.from_numpy(u).to(dev)
    score, smap = ie.ssim(t, t, reduction="none", return_map=True)
    assert float((smap - 1.0).abs().max()) <= 1e-12 and float((score - 1.0).abs().max()) <= 1e-12
    assert float((ie.psnr(t, t, reduction="none") - 80.0).abs().max()) <= 1e-12
    zero, one = torch.zeros(1, 3, 12, 12, device=dev), torch.ones(1, 3, 12, 12, device=dev)
    assert abs(float(ie.psnr(zero, one)) - (-10 * np.log10(1 + 1e-8))) <= 1e-14
    # a 3-D image is one view; a mask of zeros hides every difference; a bool mask is a 0 / 1 mask; a (1, 1, H, W) mask expands
    assert float(ie.psnr(zero[0], one[0], torch.zeros(1, 12, 12, device=dev))) == float(ie.psnr(zero, zero))
    x8, y8 = (torch.from_numpy(v).to(dev) for v in ref.scene(2, 3, 40, 50, seed=4))
    m = torch.from_numpy(ref.block_mask(1, 40, 50)).to(dev)
    assert torch.equal(ie.ssim(x8, y8, m, reduction="none"), ie.ssim(x8, y8, (m > 0).expand(2, 1, 40, 50), reduction="none"))
    assert torch.equal(ie.psnr(x8, y8, m, reduction="none"), ie.psnr(x8, y8, (m > 0).float(), reduction="none"))


def test_to_u8_is_numpys_rint_with_ties_to_even(ie, dev):
    r = np.random.default_rng(0)
    ties = ((np.arange(-2, 258, dtype=np.float64) + 0.5) / 255).astype(np.float32)
    v = np.concatenate([ties, r.uniform(-0.2, 1.2, 5000).astype(np.float32), np.arange(256, dtype=np.float32) / np.float32(255),
                        np.float32([0.0, 1.0, -0.0, 2.0, -3.0])])
    prod = v * np.float32(255)
    assert (np.abs(prod - np.floor(prod) - 0.5) == 0).sum() >= 100          # exact ties are in the set
    got = ie.to_u8(torch.from_numpy(v).to(dev))
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), ref.to_u8(v))
    assert np.array_equal(got.cpu().numpy(), np.clip(np.rint(prod), 0, 255).astype(np.uint8))
    u = torch.arange(256, dtype=torch.uint8, device=dev)
    assert ie.to_u8(u) is u
    v64 = torch.from_numpy(v.astype(np.float64)).to(dev)
    assert np.array_equal(ie.to_u8(v64).cpu().numpy(), ref.to_u8(v.astype(np.float64)))


def test_empty_batch_and_error_paths(ie, dev):
    e = torch.zeros(0, 3, 32, 32, device=dev)
    assert ie.psnr(e, e, reduction="none").shape == (0,) and ie.psnr(e, e, reduction="none").dtype == torch.float64
    score, smap = ie.ssim(e, e.to(torch.uint8), reduction="none", return_map=True)
    assert score.shape == (0,) and smap.shape[0] == 0 and score.is_cuda
    p, s = ie.evaluate_views(e, e)
    assert p.shape == s.shape == (0,)
    x = torch.rand(2, 3, 32, 40, device=dev)
    for bad in (lambda: ie.psnr(x, x[:, :, :, :39]), lambda: ie.ssim(x, x[:1]), lambda: ie.ssim(x, x.cpu()),
                lambda: ie.ssim(x[:, :, :10], x[:, :, :10]), lambda: ie.ssim(x, x, kernel_size=10),
                lambda: ie.ssim(x, x, kernel_size=ie.max_kernel_size() + 2), lambda: ie.ssim(x, x, kernel_sigma=0.0),
                lambda: ie.psnr(x, x, torch.ones(2, 1, 32, 39, device=dev)), lambda: ie.psnr(x, x, torch.ones(3, 1, 32, 40, device=dev)),
                lambda: ie.psnr(x, x, data_range=0.0), lambda: ie.psnr(x, x, reduction="sum"), lambda: ie.ssim(x.double(), x.double()),
                lambda: ie.psnr(x[0, 0], x[0, 0]), lambda: ie.psnr(x * 2, x, check_range=True),
                lambda: ie.ssim(x - 1, x, check_range=True), lambda: ie.psnr(x * 255, x, data_range=100.0, check_range=True)):
        with pytest.raises(ValueError):
            bad()
    # in range: accepted
    assert float(ie.psnr(x, x, check_range=True)) == float(ie.psnr(x, x))
    assert float(ie.psnr(x * 255, x * 255, data_range=255.0, check_range=True)) == float(ie.psnr(x, x))


def test_views_of_two_scenes_score_like_the_reference(ie, dev):
    """evaluate_views on three float views of two scenes (8-bit conversion first, then both scores) and the SceneScores table
    against the yardstick on the converted images"""
    r = np.random.default_rng(12)
    x8, y8 = ref.scene(3, 3, 48, 56, seed=10)
    pred = np.clip(x8 / np.float32(255) + r.uniform(-0.4, 0.4, x8.shape).astype(np.float32) / np.float32(255), -0.1, 1.1).astype(np.float32)
    gt = (y8 / np.float32(255)).astype(np.float32)
    mask = ref.graded_mask(3, 48, 56, 11)
    p, s = ie.evaluate_views(torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev), torch.from_numpy(mask).to(dev))
    pu, gu = ref.to_u8(pred), ref.to_u8(gt)
    assert np.array_equal(gu, y8)
    want_p, want_s = ref.psnr(pu, gu, mask), ref.ssim(pu, gu, mask)[0]
    assert p.shape == s.shape == (3,) and p.dtype == s.dtype == torch.float64
    assert np.abs(p.cpu().numpy() - want_p).max() <= BAR and np.abs(s.cpu().numpy() - want_s).max() <= BAR
    scores = ie.SceneScores("ours")
    scores.update("dtu_scan24", p[:2], s[:2])
    scores.update("dtu_scan37", p[2], s[2])
    assert abs(scores.scene_mean("dtu_scan24")[0] - want_p[:2].mean()) <= BAR and abs(scores.scene_mean("dtu_scan37")[1] - want_s[2]) <= BAR
    mean = scores.mean()
    assert abs(mean[0] - (want_p[:2].mean() + want_p[2]) / 2) <= BAR and abs(mean[1] - (want_s[:2].mean() + want_s[2]) / 2) <= BAR
    assert "%2.2f & %2.2f & " % (want_p[:2].mean(), want_p[2]) in scores.table()
