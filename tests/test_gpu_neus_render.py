"""The kernels of csrc/neus_render.hip against psdf_neus_composite_forward / _backward (bits) and against the float64 evaluator
tests/neus_render_float64.py (ENTRY BY ENTRY), on every path.

(a) forward on one container with rays of 0, 1, 63, 64, 65, 128, 129 and 256 samples and both kinds of invalid ray (empty,
    overflowed), and on equal-count containers of 1, 65 and 129 samples (the other RayIndex mode): pred and bg are the composite
    forward's bits, every weight sum lies within its float64 bar, each output is nullable on its own.
(b) backward with max_per_ray declared as 64, 128 and 256 (K = 1, 2, 4).  Without g_weights_sum: the composite backward's bits,
    g_bg on and off, reference_compat on and off (g_inv_s, whose one-atomic-per-wave sum has no fixed order in either kernel, within
    its bar).  With g_weights_sum, for every upstream subset that holds it: every entry of g_sdf, g_gradients, g_rgb, g_inv_s
    within its float64 bar.  A ray longer than declared comes back as NaN and every other ray keeps its bits.
(c) the loss tail on the cases of tests/host/neus_mask_loss_check.cpp: R in {1, 255, 256, 257, limit, limit + 1}, weight sums on,
    beside and between the clip bounds against both mask values, hit null / all zero / mixed; the accumulator is added to; two
    calls give the same bits.
Every comparison prints (-s) the worst error / bar; no constant of a bar is tuned to what the kernels give (the derivations: the
helper's docstring; tests/test_neus_render_host.py checks them on the CPU)."""
import pytest
import torch

from tests import neus_render_float64 as ev64
from tests.float64_check import check, show

pytestmark = pytest.mark.gpu

CASES = [("borders", 64), ("borders", 128), ("borders", 256), ("equal1", 64), ("equal65", 128), ("equal129", 256)]
_SHARED = {}


def make_rs(c, dev, dirs, dt):
    from permuto_sdf_amd.bridge import RaySamplesPacked
    rs = RaySamplesPacked(c["R"], c["N"], device=dev)
    rs.ray_start_end_idx = c["start_end"].to(dev)
    if c["equal"]:
        rs.rays_have_equal_nr_of_samples, rs.fixed_nr_of_samples_per_ray = True, c["fixed"]
    rs.samples_dirs = dirs.to(dev).contiguous()
    rs.samples_dt = dt.to(dev).view(-1, 1).contiguous()
    rs.cur_nr_samples.fill_(min(c["N"], c["total"]))
    return rs


def _setup(cname, dev):
    """container, rays, host family, device tensors, and the evaluator's forward: computed once per container, never changed"""
    key = (cname, str(dev))
    if key not in _SHARED:
        c = ev64.container(cname)
        rays = ev64.rays_of(c)
        fam = ev64.family(c, "float64")
        sdf, dirs, grad, dt, rgb, inv_s = fam
        rs = make_rs(c, dev, dirs, dt)
        dv = dict(sdf=sdf.to(dev), grad=grad.to(dev), rgb=rgb.to(dev), inv=inv_s.to(dev))
        fwd = ev64.render(rays, *fam)
        assert fwd["min_om"] > 1e-4 and not bool(fwd["kink"].any())
        _SHARED[key] = (c, rays, fam, rs, dv, fwd)
    return _SHARED[key]


def _ups(c, subset, dev, seed=0):
    return [t.to(dev) if on else None for t, on in zip(ev64.upstream(c, seed), subset)]


def _long(c, rays, mpr):
    """samples of the processed rays that are longer than declared"""
    ray_long = rays.valid & (rays.cnt > mpr)
    m = torch.zeros(c["N"], dtype=torch.bool)
    m[rays.idx[rays.mask & ray_long[:, None]]] = True
    return m


def _same_bits(a, b):
    """torch.equal with NaN == NaN (the poisoned rays of both kernels)"""
    return a.shape == b.shape and bool((torch.isnan(a) == torch.isnan(b)).all()) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


# ==================================================================================================================== (a)
@pytest.mark.parametrize("cname", ["borders", "equal1", "equal65", "equal129"])
def test_forward_bits_of_the_composite_and_weight_sum_every_entry(dev, cname):
    from permuto_sdf_amd.neus import neus_composite_forward_raw, neus_render_forward_raw
    c, rays, fam, rs, dv, fwd = _setup(cname, dev)
    args = (rs, dv["sdf"], dv["grad"], dv["rgb"], dv["inv"], ev64.RATIO)
    pred, ws, bg = neus_render_forward_raw(*args, want_bg=True)
    pred_c, bg_c, _ = neus_composite_forward_raw(*args)
    assert torch.equal(pred, pred_c) and torch.equal(bg, bg_c)
    out = []
    check(out, "weights_sum", ws, *fwd["weights_sum"])
    check(out, "pred", pred, *fwd["pred"])
    check(out, "bg", bg, *fwd["bg"])
    for want in ((True, False, False), (False, True, False), (False, False, True)):
        got = neus_render_forward_raw(*args, *want)
        for g, full, on in zip(got, (pred, ws, bg), want):
            assert (g is None) == (not on) and (g is None or torch.equal(g, full))
    skipped = ~rays.valid
    assert bool(skipped.any()) == (cname == "borders")              # the empty rays and the two whose range passes the pool
    assert not bool(pred.cpu()[skipped].any()) and not bool(ws.cpu()[skipped].any()) and bool((bg.cpu()[skipped] == 1).all())
    show("neus render forward %s" % cname, out)


# ==================================================================================================================== (b)
@pytest.mark.parametrize("cname,mpr", CASES)
def test_backward_without_weight_sum_has_the_bits_of_the_composite_backward(dev, cname, mpr):
    from permuto_sdf_amd.bridge import VolumeRendering as VR
    from permuto_sdf_amd.neus import neus_composite_backward_raw, neus_render_backward_raw, neus_render_plan
    c, rays, fam, rs, dv, fwd = _setup(cname, dev)
    assert neus_render_plan(1, mpr)[0] == {64: 1, 128: 2, 256: 4}[mpr]
    g_pred, _, g_bg = _ups(c, (True, True, True), dev)
    tail = (dv["sdf"], dv["grad"], dv["rgb"], dv["inv"], ev64.RATIO)
    long_ = _long(c, rays, mpr)
    out = []
    saved = VR.reference_compat
    try:
        for compat in (False, True):
            VR.reference_compat = compat
            for gb in (g_bg, None):
                new = neus_render_backward_raw(rs, mpr, g_pred, None, gb, *tail)
                old = neus_composite_backward_raw(rs, mpr, g_pred, gb, *tail)
                for name, a, b in zip(("g_sdf", "g_gradients", "g_rgb"), new, old):
                    assert _same_bits(a, b), (name, compat, gb is not None)
                assert bool(torch.isnan(new[0].cpu().view(-1)[long_]).all()) and not bool(torch.isnan(new[0].cpu().view(-1)[~long_]).any())
                # g_inv_s: one atomic per wave in both kernels, in whatever order the waves finish: under the float64 bar instead
                ev = ev64.render(rays, *fam, g_pred=g_pred.cpu(), g_bg=None if gb is None else gb.cpu(), compat=compat)
                if not bool(long_.any()):
                    check(out, "g_inv_s[compat %d, g_bg %d]" % (compat, gb is not None), new[3], *ev["g_inv_s"])
                    check(out, "g_inv_s of the composite", old[3], *ev["g_inv_s"])
                # and the optional outputs off
                only = neus_render_backward_raw(rs, mpr, g_pred, None, gb, *tail, need_grad=False, need_rgb=False, need_inv_s=False)
                assert only[1] is None and only[2] is None and only[3] is None and _same_bits(only[0], new[0])
    finally:
        VR.reference_compat = saved
    show("neus render backward, no g_weights_sum, %s max_per_ray %d" % (cname, mpr), out)


@pytest.mark.parametrize("cname,mpr", CASES)
def test_backward_with_weight_sum_every_entry(dev, cname, mpr):
    from permuto_sdf_amd.bridge import VolumeRendering as VR
    from permuto_sdf_amd.neus import neus_render_backward_raw
    c, rays, fam, rs, dv, fwd = _setup(cname, dev)
    N = c["N"]
    tail = (dv["sdf"], dv["grad"], dv["rgb"], dv["inv"], ev64.RATIO)
    long_ = _long(c, rays, mpr)
    keep = ~long_
    assert bool(long_.any()) == (c["max_per_ray"] > mpr)
    z = torch.zeros((), device=dev)
    out = []
    saved = VR.reference_compat
    try:
        for compat in (False, True):
            VR.reference_compat = compat
            for subset in [s for s in ev64.SUBSETS if s[1]]:
                ups = _ups(c, subset, dev)
                ev = ev64.render(rays, *fam, **{k: None if u is None else u.cpu() for k, u in zip(("g_pred", "g_ws", "g_bg"), ups)}, compat=compat)
                g_sdf, g_grad, g_rgb, g_inv = neus_render_backward_raw(rs, mpr, *ups, *tail, need_rgb=subset[0])
                tag = "[%s%s%s, compat %d]" % tuple(["pwb"[i] if on else "-" for i, on in enumerate(subset)] + [compat])
                # a ray longer than declared: NaN in every gradient of the ray, and nothing else changes
                ld = long_.to(dev)
                assert bool(torch.isnan(g_sdf.view(-1)[ld]).all()) and bool(torch.isnan(g_grad[ld]).all())
                check(out, "g_sdf" + tag, torch.where(ld, z, g_sdf.view(-1)), *ev["g_sdf"], keep)
                check(out, "g_gradients" + tag, torch.where(ld[:, None], z, g_grad), *ev["g_gradients"], keep)
                if subset[0]:
                    assert bool(torch.isnan(g_rgb[ld]).all())
                    check(out, "g_rgb" + tag, torch.where(ld[:, None], z, g_rgb), *ev["g_rgb"], keep)
                else:
                    assert g_rgb is None
                if not bool(long_.any()):
                    check(out, "g_inv_s" + tag, g_inv, *ev["g_inv_s"])
                if mpr < 256:    # the rays that fit keep the bits they have under any declared length
                    full = neus_render_backward_raw(rs, 256, *ups, *tail, need_rgb=subset[0])
                    assert torch.equal(g_sdf.view(-1)[~ld], full[0].view(-1)[~ld]) and torch.equal(g_grad[~ld], full[1][~ld])
                again = neus_render_backward_raw(rs, mpr, *ups, *tail, need_rgb=subset[0])
                assert _same_bits(again[0], g_sdf) and _same_bits(again[1], g_grad)
                assert not bool(g_sdf.cpu().view(-1)[~rays.touched(N)].any())      # slots no processed ray owns stay zero
    finally:
        VR.reference_compat = saved
    show("neus render backward with g_weights_sum, %s max_per_ray %d" % (cname, mpr), out)


def test_a_ray_longer_than_declared_is_poisoned_and_every_other_ray_is_exact(dev):
    """65 samples declared as 64 (and every longer ray of the container): NaN on their gradients, the bits of the run that declares
    256 everywhere else"""
    from permuto_sdf_amd.neus import neus_render_backward_raw
    c, rays, fam, rs, dv, fwd = _setup("borders", dev)
    ups = _ups(c, (True, True, False), dev)
    tail = (dv["sdf"], dv["grad"], dv["rgb"], dv["inv"], ev64.RATIO)
    short = neus_render_backward_raw(rs, 64, *ups, *tail, need_inv_s=False)
    full = neus_render_backward_raw(rs, 256, *ups, *tail, need_inv_s=False)
    long_ = _long(c, rays, 64).to(dev)
    assert int(long_.sum()) == 65 + 128 + 129 + 256
    for a, b in zip(short[:3], full[:3]):
        a, b = a.view(c["N"], -1), b.view(c["N"], -1)
        assert bool(torch.isnan(a[long_]).all()) and not bool(torch.isnan(b).any())
        assert torch.equal(a[~long_], b[~long_])


# ==================================================================================================================== (c)
@pytest.mark.parametrize("R", [1, 255, 256, 257, 8192, 8193])
def test_loss_tail_every_entry_accumulates_and_repeats_its_bits(dev, R):
    from permuto_sdf_amd.neus import neus_mask_loss_raw, neus_render_plan
    lim = neus_render_plan(1, 64)[3]
    assert lim == 8192 and (neus_render_plan(R, 64)[2] == 0) == (R <= lim)
    out = []
    for hit_mode in (None, "zero", "mixed"):
        pred, gt, hit, ws, gm = ev64.mask_loss_cases(R, hit_mode)
        ev = ev64.mask_loss(pred, gt, hit, ws, gm, mask_weight=0.1, base=0.25)
        d = lambda t: None if t is None else t.to(dev)
        acc = torch.full((1,), 0.25, device=dev)                    # a nonzero value beforehand: added to, not overwritten
        loss, g_pred, g_ws = neus_mask_loss_raw(d(pred), d(gt), d(hit), d(ws), d(gm), 0.1, loss=acc)
        assert loss is acc
        tag = "[R %d, hit %s]" % (R, hit_mode)
        check(out, "loss" + tag, loss, *ev["loss"])
        check(out, "g_pred" + tag, g_pred, *ev["g_pred"])
        check(out, "g_weights_sum" + tag, g_ws, *ev["g_ws"])
        # the rule at the two bounds: zero exactly where the clip stops the gradient, and only there
        inside = (ws >= torch.tensor(1e-3)) & (ws <= torch.tensor(1.0 - 1e-3))
        assert torch.equal(g_ws.cpu().view(-1) != 0, inside)
        if hit_mode == "zero":
            assert not bool(g_pred.any())
        acc2 = torch.full((1,), 0.25, device=dev)
        loss2, g_pred2, g_ws2 = neus_mask_loss_raw(d(pred), d(gt), d(hit), d(ws), d(gm), 0.1, loss=acc2)
        assert torch.equal(loss, loss2) and torch.equal(g_pred, g_pred2) and torch.equal(g_ws, g_ws2)
        fresh, none1, none2 = neus_mask_loss_raw(d(pred), d(gt), d(hit), d(ws), d(gm), 0.1, want_grad=False)
        assert none1 is None and none2 is None
        base0 = ev64.mask_loss(pred, gt, hit, ws, gm, mask_weight=0.1, base=0.0)
        check(out, "loss from zero" + tag, fresh, *base0["loss"])
    show("neus mask loss, %d rays" % R, out)
