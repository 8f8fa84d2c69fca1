"""The kernels of csrc/nerf_render.hip against the float64 evaluator tests/nerf_render_float64.py, ENTRY BY ENTRY, on every path.

(a) render forward and backward on one container with rays of 0, 1, 63, 64, 65, 128, 129 and 256 samples and both kinds of
    invalid ray, and on equal-count containers (the other RayIndex mode), with max_per_ray declared as 64, 128 and 256 (K = 1, 2,
    4), every subset of the three upstream gradients, each output on its own.  reference_compat 0 against float64; reference_compat
    1 against float64 with the channel quirk AND against the unfused operator chain nerf_alpha -> cumprod -> multiply -> integrate
    -> sum_over_each_ray (two fp32 evaluations of one formula: within the sum of their bars).  A ray longer than declared comes
    back as NaN and nothing else changes.  pred has the bits of psdf_nerf_composite_forward's pred_bg.
(b) a saturated family (raw density up to 30, dt = 1e10 on the last sample: alpha == 1, the backward's floor active) against the
    unfused chain, with the bars of the ray stage on the fp32 opacities that psdf_nerf_alpha_forward returns.
(c) the loss tail for R in {1, 63, 257}, with and without hit and mask term, weight sums on both sides of both clip bounds; two
    calls give the same bits; (d) the head join for M in {1, 63, 64, 65, 1000} against torch's gelu / gelu_backward in float64;
(e) the autograd Functions hand the kernels' results through.
Every comparison prints (-s) the worst error / bar; no constant of a bar is tuned to what the kernels give (the derivations: the
helper's docstring; tests/test_nerf_host.py checks them on the CPU)."""
import pytest
import torch

from tests import nerf_render_float64 as ev64
from tests.float64_check import check, show

pytestmark = pytest.mark.gpu

CASES = [("borders", 64), ("borders", 128), ("borders", 256), ("equal1", 64), ("equal65", 128), ("equal129", 256)]


def make_rs(c, dev, dt):
    from permuto_sdf_amd.bridge import RaySamplesPacked
    rs = RaySamplesPacked(c["R"], c["N"], device=dev)
    rs.ray_start_end_idx = c["start_end"].to(dev)
    if c["equal"]:
        rs.rays_have_equal_nr_of_samples, rs.fixed_nr_of_samples_per_ray = True, c["fixed"]
    rs.samples_dt = dt.to(dev).view(-1, 1).contiguous()
    rs.cur_nr_samples.fill_(min(c["N"], c["total"]))
    return rs


def _ups(c, subset, dev, seed=0):
    return [t.to(dev) if on else None for t, on in zip(ev64.upstream(c, seed), subset)]


def _long(c, rays, mpr):
    """samples of the processed rays that are longer than declared"""
    ray_long = rays.valid & (rays.cnt > mpr)
    m = torch.zeros(c["N"], dtype=torch.bool)
    m[rays.idx[rays.mask & ray_long[:, None]]] = True
    return m


def _chain(rs, raw, rgb, ups):
    """the operator chain the tree had before, through autograd -> (pred, ws, bg, g_raw, g_rgb)"""
    from permuto_sdf_amd.neus import nerf_alpha
    from permuto_sdf_amd.train_step import _Cumprod, _Integrate, _SumRay
    raw_g, rgb_g = raw.view(-1, 1).clone().requires_grad_(True), rgb.clone().requires_grad_(True)
    alpha, one_minus = nerf_alpha(raw_g, rs.samples_dt)
    T, bg = _Cumprod.apply(rs, one_minus)
    w = (alpha * T).view(-1, 1)
    ws, _ = _SumRay.apply(rs, w)
    pred = _Integrate.apply(rs, rgb_g, w)
    total = raw_g.sum() * 0
    for out, g in zip((pred, ws, bg), ups):
        if g is not None:
            total = total + (out.reshape(g.shape) * g).sum()
    g_raw, g_rgb = torch.autograd.grad(total, (raw_g, rgb_g), allow_unused=True)
    return pred.detach(), ws.detach(), bg.detach(), g_raw.view(-1), torch.zeros_like(rgb) if g_rgb is None else g_rgb


def _within(out, name, a, b, bar, keep):
    """two fp32 evaluations of one formula: |a - b| <= the sum of their bars"""
    a, b = a.detach().cpu().double().reshape(bar.shape), b.detach().cpu().double().reshape(bar.shape)
    k = keep if keep.dim() == bar.dim() else keep.view(-1, *([1] * (bar.dim() - 1))).expand_as(bar)
    rel = torch.where(k, (a - b).abs() / (2 * bar).clamp_min(1e-300), torch.zeros_like(bar))
    assert bool(torch.isfinite(torch.where(k, a, torch.zeros_like(a))).all()) and bool(torch.isfinite(torch.where(k, b, torch.zeros_like(b))).all()), name
    out.append("%s %.3f" % (name, float(rel.max())))
    assert float(rel.max()) <= 1.0, (name, float(rel.max()), int(rel.argmax()))


# ==================================================================================================================== (a)
@pytest.mark.parametrize("cname,mpr", CASES)
def test_render_forward_and_backward_every_entry(dev, cname, mpr):
    from permuto_sdf_amd import nerf_train as nt
    from permuto_sdf_amd.bridge import VolumeRendering as VR
    from permuto_sdf_amd.neus import nerf_composite_forward_raw
    c = ev64.container(cname)
    N, R = c["N"], c["R"]
    rays = ev64.rays_of(c)
    raw, dt, rgb = ev64.family(c, "float64")
    rs = make_rs(c, dev, dt)
    raw_d, rgb_d = raw.to(dev), rgb.to(dev)
    fwd = ev64.render(rays, raw, dt, rgb)
    assert fwd["min_om"] > 1e-4
    out = []
    # ---- forward: all three outputs, each on its own with the same bits, pred with the bits of the background kernel's
    pred, ws, bg = nt.nerf_render_raw(rs, raw_d, rgb_d)
    check(out, "pred", pred, *fwd["pred"])
    check(out, "weights_sum", ws, *fwd["weights_sum"])
    check(out, "bg", bg, *fwd["bg"])
    for want in ((True, False, False), (False, True, False), (False, False, True)):
        got = nt.nerf_render_raw(rs, raw_d, rgb_d, *want)
        for g, full, on in zip(got, (pred, ws, bg), want):
            assert (g is None) == (not on) and (g is None or torch.equal(g, full))
    pred_bg, _ = nerf_composite_forward_raw(rs, raw_d, rgb_d)
    assert torch.equal(pred, pred_bg)
    skipped = ~rays.valid
    assert not bool(pred.cpu()[skipped].any()) and not bool(ws.cpu()[skipped].any()) and bool((bg.cpu()[skipped] == 1).all())
    # ---- backward
    long_ = _long(c, rays, mpr)
    keep = ~long_
    assert bool(long_.any()) == (c["max_per_ray"] > mpr)
    saved = VR.reference_compat
    try:
        for compat in (False, True):
            VR.reference_compat = compat
            for subset in ev64.SUBSETS:
                ups = _ups(c, subset, dev)
                ev = ev64.render(rays, raw, dt, rgb, *[None if u is None else u.cpu() for u in ups], compat=compat)
                g_raw, g_rgb = nt.nerf_render_backward_raw(rs, mpr, *ups, raw_d, rgb_d)
                tag = "[%s%s%s, compat %d]" % tuple(["pwb"[i] if on else "-" for i, on in enumerate(subset)] + [compat])
                # a ray longer than declared: NaN in every gradient of the ray, and nothing else changes
                assert bool(torch.isnan(g_raw.cpu()[long_]).all()) and bool(torch.isnan(g_rgb.cpu()[long_]).all())
                z = torch.zeros((), device=dev)
                g_raw_k, g_rgb_k = torch.where(long_.to(dev), z, g_raw), torch.where(long_.to(dev)[:, None], z, g_rgb)
                check(out, "g_raw" + tag, g_raw_k, *ev["g_raw"], keep)
                check(out, "g_rgb" + tag, g_rgb_k, *ev["g_rgb"], keep)
                if mpr < 256:
                    full = nt.nerf_render_backward_raw(rs, 256, *ups, raw_d, rgb_d)
                    assert torch.equal(g_raw[keep.to(dev)], full[0][keep.to(dev)]) and torch.equal(g_rgb[keep.to(dev)], full[1][keep.to(dev)])
                again = nt.nerf_render_backward_raw(rs, mpr, *ups, raw_d, rgb_d)
                assert torch.equal(g_raw_k, torch.where(long_.to(dev), z, again[0])) and torch.equal(g_rgb_k, torch.where(long_.to(dev)[:, None], z, again[1]))
                assert not bool(g_raw.cpu()[~rays.touched(N)].any())            # slots no processed ray owns stay zero
                if compat:       # the unfused chain under the same switch
                    cp, cw, cb, c_raw, c_rgb = _chain(rs, raw_d, rgb_d, ups)
                    _within(out, "chain g_raw" + tag, g_raw_k, c_raw, ev["g_raw"][1], keep)
                    _within(out, "chain g_rgb" + tag, g_rgb_k, c_rgb, ev["g_rgb"][1], keep)
                    everything = torch.ones(R, dtype=torch.bool)
                    _within(out, "chain pred", pred, cp, fwd["pred"][1], everything)
                    _within(out, "chain weights_sum", ws, cw, fwd["weights_sum"][1], everything)
                    _within(out, "chain bg", bg, cb, fwd["bg"][1], everything)
    finally:
        VR.reference_compat = saved
    show("nerf render %s (max_per_ray %d, %d samples of over-long rays)" % (cname, mpr, int(long_.sum())), out)


# ==================================================================================================================== (b)
@pytest.mark.parametrize("cname,mpr", [("borders", 256), ("equal129", 256), ("equal65", 128)])
def test_saturated_render_against_the_unfused_chain(dev, cname, mpr):
    from permuto_sdf_amd import _lib as L
    from permuto_sdf_amd import nerf_train as nt
    from permuto_sdf_amd.bridge import VolumeRendering as VR
    c = ev64.container(cname)
    N, R = c["N"], c["R"]
    rays = ev64.rays_of(c)
    raw, dt, rgb = ev64.family(c, "saturated")
    rs = make_rs(c, dev, dt)
    raw_d, rgb_d = raw.to(dev), rgb.to(dev)
    a, om = torch.empty_like(raw_d), torch.empty_like(raw_d)
    L.call("psdf_nerf_alpha_forward", L.c_l(N), L.ptr(raw_d), L.ptr(dt.view(-1).contiguous().to(dev)), L.ptr(a), L.ptr(om), L.stream())
    sat = float((a.cpu()[rays.touched(N)] == 1).float().mean())
    assert sat >= 0.1 and float(om.cpu()[rays.touched(N)].min()) < 1e-6            # the floor of the backward is active
    out = []
    everything, samples = torch.ones(R, dtype=torch.bool), torch.ones(N, dtype=torch.bool)
    worst_rel = 0.0
    saved = VR.reference_compat
    try:
        for compat in (False, True):
            VR.reference_compat = compat
            for subset in ev64.SUBSETS:
                ups = _ups(c, subset, dev, seed=1)
                # the ray stage on the fp32 opacities: exact inputs, valid at any saturation
                ev = ev64.render(rays, raw, dt, rgb, *[None if u is None else u.cpu() for u in ups], compat=compat, alpha=a, om=om)
                pred, ws, bg = nt.nerf_render_raw(rs, raw_d, rgb_d)
                g_raw, g_rgb = nt.nerf_render_backward_raw(rs, mpr, *ups, raw_d, rgb_d)
                cp, cw, cb, c_raw, c_rgb = _chain(rs, raw_d, rgb_d, ups)
                tag = "[%s%s%s, compat %d]" % tuple(["pwb"[i] if on else "-" for i, on in enumerate(subset)] + [compat])
                _within(out, "g_raw" + tag, g_raw, c_raw, ev["g_raw"][1], samples)
                _within(out, "g_rgb" + tag, g_rgb, c_rgb, ev["g_rgb"][1], samples)
                check(out, "g_raw/f64" + tag, g_raw, *ev["g_raw"])
                check(out, "g_rgb/f64" + tag, g_rgb, *ev["g_rgb"])
                worst_rel = max(worst_rel, float((g_raw - c_raw).abs().max() / c_raw.abs().max().clamp_min(1e-30)))
            _within(out, "pred", pred, cp, ev["pred"][1], everything)
            _within(out, "weights_sum", ws, cw, ev["weights_sum"][1], everything)
            _within(out, "bg", bg, cb, ev["bg"][1], everything)
    finally:
        VR.reference_compat = saved
    # (most entries behind an opaque sample are zero or subnormal: their bars are the absolute terms; printed beside them, the
    #  largest difference of the two evaluations of g_raw over the largest entry)
    print("fused against the chain, g_raw: max |diff| / max |entry| %.2e" % worst_rel)
    show("saturated nerf render %s (alpha == 1 on %.0f%% of the samples)" % (cname, 100 * sat), out)


# ==================================================================================================================== (c)
@pytest.mark.parametrize("R", [1, 63, 257])
@pytest.mark.parametrize("with_hit", [True, False])
@pytest.mark.parametrize("with_mask", [True, False])
def test_loss_tail_every_entry(dev, R, with_hit, with_mask):
    from permuto_sdf_amd import nerf_train as nt
    pred, gt, hit, ws, gm = ev64.loss_cases(R)
    hit = hit if with_hit else None
    ws, gm = (ws, gm) if with_mask else (None, None)
    ev = ev64.loss(pred, gt, hit, ws, gm, base=0.25)
    d = lambda t: None if t is None else t.to(dev)
    acc = torch.full((1,), 0.25, device=dev)
    loss, terms, g_pred, g_ws = nt.nerf_loss_raw(d(pred), d(gt), d(hit), d(ws), d(gm), loss=acc)
    out = []
    check(out, "terms", terms, *ev["terms"])
    check(out, "loss", loss, ev["loss"][0].reshape(1), ev["loss"][1].reshape(1))
    check(out, "g_pred", g_pred, *ev["g_pred"])
    if with_mask:
        check(out, "g_weights_sum", g_ws, *ev["g_ws"])
        inside = (ws >= torch.tensor(1e-3)) & (ws <= torch.tensor(1.0 - 1e-3))
        assert bool((g_ws.cpu().view(-1)[~inside] == 0).all()) and bool((g_ws.cpu().view(-1)[inside] != 0).all())
    else:
        assert g_ws is None and float(terms[1]) == 0.0
    # the same bits on every call, with and without the gradients
    loss2, terms2, g_pred2, g_ws2 = nt.nerf_loss_raw(d(pred), d(gt), d(hit), d(ws), d(gm), loss=torch.full((1,), 0.25, device=dev))
    _, terms3, none_p, none_w = nt.nerf_loss_raw(d(pred), d(gt), d(hit), d(ws), d(gm), want_grad=False)
    assert torch.equal(terms, terms2) and torch.equal(terms, terms3) and torch.equal(loss, loss2) and torch.equal(g_pred, g_pred2)
    assert none_p is None and none_w is None and (g_ws is None or torch.equal(g_ws, g_ws2))
    show("nerf loss R %d hit %d mask %d" % (R, with_hit, with_mask), out)


def test_loss_tail_past_one_pass_of_its_grid(dev):
    """more rays than the capped grid covers in one pass (a thread walks two rays): the same sums"""
    from permuto_sdf_amd import nerf_train as nt
    R = nt.plan(1)[2] + 77
    pred, gt, hit, ws, gm = ev64.loss_cases(R)
    ev = ev64.loss(pred, gt, hit, ws, gm)
    loss, terms, g_pred, g_ws = nt.nerf_loss_raw(*[t.to(dev) for t in (pred, gt, hit, ws, gm)])
    out = []
    check(out, "terms", terms, *ev["terms"])
    check(out, "g_pred", g_pred, *ev["g_pred"])
    check(out, "g_weights_sum", g_ws, *ev["g_ws"])
    show("nerf loss R %d (%d workgroups)" % (R, nt.plan(R)[0]), out)


# ==================================================================================================================== (d)
@pytest.mark.parametrize("M", [1, 63, 64, 65, 1000])
def test_head_join_and_its_backward(dev, M):
    from permuto_sdf_amd import nerf_train as nt
    from permuto_sdf_amd.bridge import PermutoSDF
    g = torch.Generator().manual_seed(M)
    fd = torch.randn(65, M, generator=g) * 3
    fd.view(-1)[::17] = torch.tensor([0.0, -10.0, 10.0, -6.5, 6.5, 1e-20]).repeat(fd.numel() // 17 // 6 + 1)[:len(fd.view(-1)[::17])]
    dirs = torch.nn.functional.normalize(torch.randn(M, 3, generator=g), dim=1).to(dev)
    sh = PermutoSDF.spherical_harmonics(dirs, 4)
    x2 = nt.nerf_head_join_raw(fd.to(dev), sh)
    assert x2.shape == (80, M) and torch.equal(x2[64:], sh.t())
    (val, bar_val), (der, bar_der) = ev64.gelu_bars(fd[1:])
    out = []
    check(out, "gelu", x2[:64], val, bar_val)
    g_raw, dX2 = torch.randn(M, generator=g), torch.randn(80, M, generator=g)
    g_fd = nt.nerf_head_join_backward_raw(g_raw.to(dev), dX2.to(dev), fd.to(dev))
    assert g_fd.shape == (65, M) and torch.equal(g_fd[0].cpu(), g_raw)
    gd = dX2[:64].double()
    check(out, "g_fd", g_fd[1:], gd * der, gd.abs() * bar_der + ev64.U * (gd * der).abs() + ev64.TINY)
    # what the step did before: gelu + t() + cat, gelu_backward + cat in torch's fp32 -- the same up to both sides' bars
    old = torch.cat([torch.nn.functional.gelu(fd.to(dev)[1:65]), sh.t()], 0)
    assert torch.equal(old[64:], x2[64:])
    print("against torch's fp32 gelu on the device: max |diff| / |z| %.2e" % float(((old[:64] - x2[:64]).abs().cpu() / fd[1:].abs().clamp_min(1e-30)).max()))
    show("nerf head join M %d" % M, out)


# ==================================================================================================================== (e)
def test_autograd_functions_hand_the_kernels_through(dev):
    from permuto_sdf_amd import nerf_train as nt
    c = ev64.container("borders")
    raw, dt, rgb = ev64.family(c, "float64")
    rs = make_rs(c, dev, dt)
    g_pred, g_ws, g_bg = (t.to(dev) for t in ev64.upstream(c))
    for subset in ev64.SUBSETS:
        raw_g, rgb_g = raw.to(dev).view(-1, 1).requires_grad_(True), rgb.to(dev).requires_grad_(True)
        outs = nt.nerf_render(rs, 256, raw_g, rgb_g)
        assert [tuple(o.shape) for o in outs] == [(c["R"], 3), (c["R"], 1), (c["R"], 1)]
        total = sum((o * g).sum() for o, g, on in zip(outs, (g_pred, g_ws, g_bg), subset) if on)
        total.backward()
        want = nt.nerf_render_backward_raw(rs, 256, *[g if on else None for g, on in zip((g_pred, g_ws, g_bg), subset)], raw.to(dev), rgb.to(dev))
        assert raw_g.grad.shape == (c["N"], 1) and torch.equal(raw_g.grad.view(-1), want[0]) and torch.equal(rgb_g.grad, want[1])
    # the loss: value and gradients of the Function are the raw call's; the torch form agrees to fp32 rounding
    pred, gt, hit, ws, gm = (t.to(dev) for t in ev64.loss_cases(257))
    p, w = pred.clone().requires_grad_(True), ws.clone().view(-1, 1).requires_grad_(True)
    loss, terms = nt.nerf_loss(p, gt, hit, w, gm.view(-1, 1))
    (loss * 2.0).backward()
    l0, t0, gp, gw = nt.nerf_loss_raw(pred, gt, hit, ws, gm)
    assert float(loss.detach()) == float(l0) and torch.equal(terms, t0) and torch.equal(p.grad, 2.0 * gp) and torch.equal(w.grad, 2.0 * gw)
    p2, w2 = pred.clone().requires_grad_(True), ws.clone().requires_grad_(True)
    lt, tt = nt.nerf_loss_torch(p2, gt, hit, w2, gm)
    lt.backward()
    assert abs(float(lt) - float(l0)) <= 1e-5 * abs(float(l0))
    assert float((p2.grad - gp).abs().max()) <= 1e-5 * float(gp.abs().max())
    assert float((w2.grad.view(-1, 1) - gw).abs().max()) <= 1e-5 * float(gw.abs().max())
    rgb_only, t_only = nt.nerf_loss(pred, gt, None)
    assert float(t_only[1]) == 0.0 and float(rgb_only) == float(t_only[0])
