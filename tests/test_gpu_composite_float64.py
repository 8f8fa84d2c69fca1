"""The compositing kernels (csrc/neus.hip, csrc/volume_rendering.hip, csrc/composite_fused.hip, composite_device.h) against the
float64 evaluator of the same formulas (oracle/composite_float64.py), ENTRY BY ENTRY, on every kernel path.

The older compositing tests compare gradients in the max-norm of the whole tensor.  Transmittance decays geometrically along a
ray: 75-80 % of the entries of g_sdf / g_gradients / g_rgb / w lie below 1e-5 of the largest one at 128 samples per ray, and a
kernel that wrote zeros there -- or dropped the cross-chunk tail of the suffix sum -- passed.  Those entries feed the lattice
gradient, and Adam rescales every entry by its own magnitude.  Here every entry has a bar of its own:

    ray stage      |kernel - float64| <= ((m + r) sum|t| + sum r_T |t|) u + 2^-126 uf        (oracle/composite_float64.error_bar)
                   m terms (any summation order), r roundings per term from the kernel expressions (the R_* constants),
                   r_T = i + 1 multiplication nodes behind the transmittance of sample i (scan_mults), uf for underflowed intermediates
    opacity stage  first-order running error analysis of section() and of the backward expressions, absolute where the formula is
                   ill-conditioned, with the measured accuracy of the device expf / log1pf (derivation: the evaluator's docstring)
    fused          bar(g_alpha D) = bar(g_alpha) |D| + |g_alpha| E(D) + bar(g_alpha) E(D)

No constant of a bar is tuned to what the kernels give.  Input families and containers: oracle/composite_cases.py (the CPU test
tests/test_oracle_composite_float64.py verifies the exclusion caps and the "bites" shares on the same inputs, no kernel involved).
Exclusions are conditions: an entry whose true_cos lies within its rounding error of a relu kink (cap: 0.1 % of a case) -- nothing
else.  Every comparison prints (-s) the worst error / bar, the share of non-zero reference entries whose bar is below 1e-3 of the
entry ("bites") and the share whose bar reaches the entry itself ("saturated": fp32 gives an exact 0 or a flushed value where
float64 keeps 1e-30; such entries pass through the absolute terms only and are NOT checked to fp32 accuracy).

At inv_s 64 the surface-crossing family does not saturate (sigmoid arguments end at -22; alpha == 1.0f needs -28): the 20 % /
subnormal-T assertions apply from inv_s 300 on and the shares at 64 are printed.
A ray of volume_render_nerf with some incoming T within its own bar of the 1e-4 early-out is left out (cap: 1 % of the rays of a
case; the seeds meet it on the CPU with the float64 evaluator alone)."""
import pytest
import torch

from oracle import composite_cases as cc
from oracle import composite_float64 as c64
from tests.float64_check import check, show

pytestmark = pytest.mark.gpu

RATIO = 0.6


def make_rs(c, dev, dirs=None, dt=None):
    from permuto_sdf import RaySamplesPacked
    rs = RaySamplesPacked(c["R"], c["N"], device=dev)
    rs.ray_start_end_idx = c["start_end"].to(dev)
    if c["equal"]:
        rs.rays_have_equal_nr_of_samples, rs.fixed_nr_of_samples_per_ray = True, c["fixed"]
    if dirs is not None:
        rs.samples_dirs = dirs.to(dev)
    if dt is not None:
        rs.samples_dt = dt.to(dev).view(-1, 1).contiguous()
    rs.cur_nr_samples.fill_(min(c["N"], c["total"]))
    return rs


def checkq(out, name, got, q, r, rays=None, N=None):
    if rays is not None:
        q = rays.scatter_q(q, N)
    return check(out, name, got, q.val, c64.error_bar(q, r))


# ============================================================================================ the opacity kernels alone
NEUS_CASES = [("noise", 300.0), ("cross", 64.0), ("cross", 300.0), ("cross", 1000.0), ("cross", 1e6), ("grazing", 300.0)]


@pytest.mark.parametrize("family,inv_s", NEUS_CASES)
def test_neus_alpha_forward_backward_every_entry(dev, family, inv_s):
    from permuto_sdf_amd.neus import neus_alpha_backward_raw, neus_alpha_forward_raw
    c = cc.container("ragged")
    N = c["N"]
    sdf, dirs, grad, dt = cc.neus_family(c, family)
    inv = torch.tensor([inv_s])
    op = c64.neus_opacity(sdf, dirs, grad, dt, inv, RATIO)
    keep = ~op["kink"]
    assert int(op["kink"].sum()) <= 1e-3 * N
    d = lambda t: t.to(dev)
    a, om = neus_alpha_forward_raw(d(sdf), d(dirs), d(grad), d(dt), d(inv), RATIO)
    out = []
    check(out, "alpha", a, op["alpha"], op["E_alpha"], keep)
    check(out, "1 - alpha + 1e-7", om, op["om"], op["E_om"], keep)
    sat = float((a == 1).float().mean())
    # asserted from inv_s 300 on: at 64 the sigmoid arguments of this family end at -22 and alpha == 1.0f needs the second sigmoid
    # below half an ulp of 1e-5, an argument below -28 (0.0 % there; the share is printed for every case)
    if family == "cross" and inv_s >= 300:
        assert sat >= 0.2
    g = torch.Generator().manual_seed(5)
    for upstream in ("dense", "needle"):
        ga = torch.randn(N, 1, generator=g)
        if upstream == "needle":
            ga[torch.randperm(N, generator=g)[5:]] = 0.0
        assert not bool(op["kink"][ga.view(-1) != 0].any()) or upstream == "dense"
        g_sdf, g_grad, g_inv = neus_alpha_backward_raw(d(ga), d(sdf), d(dirs), d(grad), d(dt), d(inv), RATIO)
        g64 = ga.double().view(-1)
        uf = c64.TINY * op["uf"] * (1 + g64.abs())
        check(out, "g_sdf[%s]" % upstream, g_sdf, g64 * op["D_sdf"], g64.abs() * op["E_sdf"] + uf, keep)
        check(out, "g_gradients[%s]" % upstream, g_grad, g64[:, None] * op["D_grad"], g64.abs()[:, None] * op["E_grad"] + uf[:, None], keep)
        # d / d inv_s: a signed sum over the samples in no fixed order (wave sums + one atomic per wave): m additions.  At full size
        # the bar is wide (m = N terms); the needle upstream keeps m at 5
        t = (g64 * op["D_inv"])[keep]
        m = int((t != 0).sum())
        bar = (g64.abs() * op["E_inv"] + uf)[keep].sum() + m * c64.U * c64.SLACK * t.abs().sum()
        nk = int(op["kink"][g64 != 0].sum())                        # a kink entry may take the other relu arm in fp32: the sum
        if nk == 0:                                                 # over the samples is then under no bar, and that is printed
            check(out, "g_inv_s[%s, m = %d]" % (upstream, m), g_inv, t.sum().reshape(1), bar.reshape(1))
        else:
            out.append("g_inv_s[%s] NOT CHECKED: %d kink entries carry a non-zero upstream" % (upstream, nk))
    show("neus alpha %s inv_s %g (alpha == 1 on %.1f%%, %d kink entries excluded)" % (family, inv_s, 100 * sat, int(op["kink"].sum())), out)


def test_nerf_alpha_forward_backward_every_entry(dev):
    from permuto_sdf_amd import _lib as L
    c = cc.container("ragged")
    N = c["N"]
    raw, dt = cc.nerf_family(c)
    op = c64.nerf_opacity(raw, dt)
    raw_d, dt_d = raw.to(dev), dt.view(-1).contiguous().to(dev)
    a, om = torch.empty_like(raw_d), torch.empty_like(raw_d)
    L.call("psdf_nerf_alpha_forward", L.c_l(N), L.ptr(raw_d), L.ptr(dt_d), L.ptr(a), L.ptr(om), L.stream())
    out = []
    check(out, "alpha", a, op["alpha"], op["E_alpha"])
    check(out, "1 - alpha + 1e-7", om, op["om"], op["E_om"])
    g = torch.Generator().manual_seed(6)
    ga, go = torch.randn(N, generator=g), torch.randn(N, generator=g)
    g_raw = torch.empty_like(raw_d)
    L.call("psdf_nerf_alpha_backward", L.c_l(N), L.ptr(raw_d), L.ptr(dt_d), L.ptr(ga.to(dev)), L.ptr(go.to(dev)), L.ptr(g_raw), L.stream())
    g64 = ga.double() - go.double()                                 # one_minus = 1 - alpha + 1e-7; the difference is rounded once
    bar = g64.abs() * (op["E_D"] + c64.U * op["D"].abs()) + c64.TINY * op["uf"] * (1 + g64.abs())
    check(out, "g_raw", g_raw, g64 * op["D"], bar)
    show("nerf alpha, dt = 1e10 on the last sample of %d rays" % int((dt == 1e10).sum()), out)


@pytest.mark.parametrize("family,inv_s", [("cross", 1000.0), ("grazing", 300.0), ("noise", 300.0)])
def test_fused_kernels_form_the_opacity_bits_of_the_opacity_kernels(dev, family, inv_s):
    """The ray stage of the evaluator starts from the fp32 alpha that psdf_neus_alpha_forward / psdf_nerf_alpha_forward return.
    That is valid for the fused kernels only if they form the same bits: re-index the samples as N rays of ONE sample each
    (T = 1): the fused NeuS weights are alpha, and with rgb = 1 the fused NeRF pred_bg is alpha, bit for bit."""
    from permuto_sdf_amd import _lib as L
    from permuto_sdf_amd.neus import neus_alpha_forward_raw, neus_composite_forward_raw, nerf_composite_forward_raw
    base = cc.container("ragged")
    N = base["N"]
    sdf, dirs, grad, dt = cc.neus_family(base, family)
    one = dict(name="ones", counts=torch.ones(N, dtype=torch.int64), start_end=torch.stack([torch.arange(N), torch.arange(N) + 1], 1).to(torch.int32),
               N=N, total=N, equal=False, fixed=0, max_per_ray=1, R=N)
    rs = make_rs(one, dev, dirs, dt)
    inv = torch.tensor([inv_s], device=dev)
    a, om = neus_alpha_forward_raw(sdf.to(dev), dirs.to(dev), grad.to(dev), dt.to(dev), inv, RATIO)
    pred, bg, w = neus_composite_forward_raw(rs, sdf.to(dev), grad.to(dev), torch.ones(N, 3, device=dev), inv, RATIO, want_weights=True)
    assert torch.equal(w, a) and torch.equal(pred, a.expand(N, 3)) and bool((bg == 1).all())
    raw, dtb = cc.nerf_family(base)
    rs.samples_dt = dtb.to(dev)
    an, omn = torch.empty(N, device=dev), torch.empty(N, device=dev)
    L.call("psdf_nerf_alpha_forward", L.c_l(N), L.ptr(raw.to(dev)), L.ptr(dtb.view(-1).contiguous().to(dev)), L.ptr(an), L.ptr(omn), L.stream())
    pb, _ = nerf_composite_forward_raw(rs, raw.to(dev), torch.ones(N, 3, device=dev))
    assert torch.equal(pb, an.view(N, 1).expand(N, 3))


# ================================================================================================ the operator chain
CHAIN = [("equal%d" % n, "cross", 1000.0, "dense") for n in cc.EQUAL_COUNTS] + [
    ("ragged", "cross", 300.0, "dense"), ("ragged", "cross", 300.0, "needle"), ("ragged", "noise", 300.0, "dense"),
    ("overflow", "cross", 1000.0, "dense"), ("overflow", "cross", 1e6, "needle")]


def _neus_setup(dev, cname, family, inv_s, up):
    from permuto_sdf_amd.neus import neus_alpha_forward_raw
    c = cc.container(cname)
    sdf, dirs, grad, dt = cc.neus_family(c, family)
    rgb, g_pred, g_bg = cc.upstream(c, up)
    rs = make_rs(c, dev, dirs, dt)
    inv = torch.tensor([inv_s], device=dev)
    dv = dict(sdf=sdf.to(dev), grad=grad.to(dev), rgb=rgb.to(dev), g_pred=g_pred.to(dev), g_bg=g_bg.to(dev), inv=inv)
    a, om = neus_alpha_forward_raw(dv["sdf"], rs.samples_dirs, dv["grad"], rs.samples_dt, inv, RATIO)
    rays = c64.Rays(c["start_end"], c["N"])
    return c, (sdf, dirs, grad, dt, rgb, g_pred, g_bg), rs, dv, a, om, rays


@pytest.mark.parametrize("cname,family,inv_s,up", CHAIN)
def test_operator_chain_every_entry(dev, cname, family, inv_s, up):
    """cumprod_alpha2transmittance and its backward, integrate_with_weights and its backward (compat on and off),
    cumsum_over_each_ray in both directions, sum_over_each_ray, compute_cdf: each against the evaluator on ITS OWN fp32 inputs,
    and the chain's end result g_alpha against the ray stage evaluated from (alpha, rgb, upstream) alone."""
    from permuto_sdf import VolumeRendering as VR
    c, (sdf, dirs, grad, dt, rgb, g_pred, g_bg), rs, dv, a, om, rays = _neus_setup(dev, cname, family, inv_s, up)
    N = c["N"]
    st = c64.RayStage(rays, a, om)
    out = []
    T, bg = VR.cumprod_alpha2transmittance(rs, om)
    qT, qbg = st.transmittance()
    _, bT = checkq(out, "T", T, qT, c64.R_T, rays, N)
    checkq(out, "bg", bg, qbg, c64.R_T)
    live = rays.touched(N)
    # from inv_s 300 on (see test_neus_alpha_forward_backward_every_entry) and for rays long enough to cross the surface: a ray of
    # 1 or 2 samples has no sample behind it
    if family == "cross" and inv_s >= 300 and c["max_per_ray"] >= 48:
        assert float((a.cpu().view(-1)[live] == 1).float().mean()) >= 0.2 and float(T.cpu().view(-1)[live].min()) < c64.TINY
    w = a * T
    _, bw = checkq(out, "w", w, st.weights(), c64.R_W, rays, N)
    pred = VR.integrate_with_weights(rs, dv["rgb"], w)
    checkq(out, "pred", pred, c64.op_integrate(rays, rgb, w), c64.R_OP_INTEGRATE)
    s_ray, s_smp = VR.sum_over_each_ray(rs, dv["rgb"])
    q_ray, q_smp = c64.op_sum(rays, rgb)
    checkq(out, "sum/ray", s_ray, q_ray, c64.R_OP_SUM)
    checkq(out, "sum/sample", s_smp, q_smp, c64.R_OP_SUM, rays, N)
    checkq(out, "cdf", VR.compute_cdf(rs, w), c64.op_cumsum(rays, w, False, True), c64.R_OP_SUM, rays, N)
    checkq(out, "cumsum", VR.cumsum_over_each_ray(rs, w, False), c64.op_cumsum(rays, w, False), c64.R_OP_SUM, rays, N)
    saved = VR.reference_compat
    try:
        for compat in (True, False):
            VR.reference_compat = compat
            g_rgb, g_w = VR.integrate_with_weights_backward(dv["g_pred"], rs, dv["rgb"], w, None)
            q_rgb, q_w = c64.op_integrate_backward(rays, g_pred, rgb, w, compat)
            checkq(out, "g_rgb", g_rgb, q_rgb, c64.R_OP_GRGB, rays, N)
            checkq(out, "g_w[compat %d]" % compat, g_w, q_w, c64.R_GW, rays, N)
            g_T = g_w * a
            v = g_T * T
            cs = VR.cumsum_over_each_ray(rs, v, True)
            checkq(out, "suffix sum", cs, c64.op_cumsum(rays, v, True), c64.R_OP_SUM, rays, N)
            g_om = VR.cumprod_alpha2transmittance_backward(g_T, dv["g_bg"], rs, om, T, bg, cs)
            checkq(out, "g_om (operator)", g_om, c64.op_cumprod_backward(rays, g_bg, om, bg, cs), c64.R_OP_CUMPROD_BWD, rays, N)
            g_alpha = g_w * T - g_om
            back = st.backward(rgb, g_pred, g_bg, compat)
            _, bga = checkq(out, "g_alpha (chain)[compat %d]" % compat, g_alpha, back["g_alpha"], c64.R_RAY_BWD, rays, N)
            checkq(out, "g_rgb (chain)", g_rgb, back["g_rgb"], c64.R_GRGB, rays, N)
    finally:
        VR.reference_compat = saved
    if family == "cross" and up == "dense" and c["max_per_ray"] >= 48:
        assert min(bT, bw, bga) >= 0.5, (bT, bw, bga)               # the bars of the ray stage bite (verified on the CPU first)
    show("operator chain %s %s inv_s %g %s" % (cname, family, inv_s, up), out)


# ================================================================================================== the fused kernels
FUSED = [("equal%d" % n, None, "cross", 1000.0, "dense") for n in cc.EQUAL_COUNTS] + [
    ("ragged", None, "noise", 300.0, "dense"), ("ragged", None, "cross", 64.0, "dense"), ("ragged", None, "cross", 300.0, "needle"),
    ("ragged", None, "cross", 1e6, "dense"), ("ragged", None, "grazing", 300.0, "dense"), ("overflow", None, "cross", 1000.0, "needle"),
    ("overflow", None, "cross", 300.0, "dense"),
    ("cap64", 64, "cross", 300.0, "dense"), ("cap64", 128, "cross", 300.0, "needle"), ("cap64", 256, "cross", 1000.0, "dense"),
    ("cap128", 128, "cross", 1000.0, "dense"), ("cap128", 256, "cross", 300.0, "needle"), ("cap256", 256, "cross", 300.0, "dense")]


def _fused_neus_bars(c, host, a, om, rays, inv_s, compat, with_bg):
    sdf, dirs, grad, dt, rgb, g_pred, g_bg = host
    N = c["N"]
    st = c64.RayStage(rays, a, om)
    back = st.backward(rgb, g_pred, g_bg if with_bg else None, compat)
    op = c64.neus_opacity(sdf, dirs, grad, dt, torch.tensor([inv_s]), RATIO)
    ga = rays.scatter_q(back["g_alpha"], N)
    bar_ga = c64.error_bar(ga, c64.R_RAY_BWD)
    return st, back, op, ga.val, bar_ga


@pytest.mark.parametrize("cname,max_per_ray,family,inv_s,up", FUSED)
def test_fused_neus_composite_every_entry(dev, cname, max_per_ray, family, inv_s, up):
    from permuto_sdf import VolumeRendering as VR
    from permuto_sdf_amd.neus import neus_composite_backward_raw, neus_composite_forward_raw
    c, host, rs, dv, a, om, rays = _neus_setup(dev, cname, family, inv_s, up)
    sdf, dirs, grad, dt, rgb, g_pred, g_bg = host
    N = c["N"]
    mpr = c["max_per_ray"] if max_per_ray is None else max_per_ray
    out = []
    # ---- forward: all optional outputs on, then off
    pred, bg, w = neus_composite_forward_raw(rs, dv["sdf"], dv["grad"], dv["rgb"], dv["inv"], RATIO, want_weights=True)
    st = c64.RayStage(rays, a, om)
    checkq(out, "pred", pred, st.radiance(rgb), c64.R_PRED)
    checkq(out, "bg", bg, st.transmittance()[1], c64.R_T)
    checkq(out, "w", w, st.weights(), c64.R_W, rays, N)
    pred2, bg2, none = neus_composite_forward_raw(rs, dv["sdf"], dv["grad"], dv["rgb"], dv["inv"], RATIO)
    assert none is None and torch.equal(pred, pred2) and torch.equal(bg, bg2)
    # ---- backward
    saved = VR.reference_compat
    try:
        for compat, with_bg in ((True, True), (False, True), (True, False)):
            VR.reference_compat = compat
            st, back, op, ga, bar_ga = _fused_neus_bars(c, host, a, om, rays, inv_s, compat, with_bg)
            keep = ~op["kink"]
            assert int(op["kink"].sum()) <= 1e-3 * N
            gbg = dv["g_bg"] if with_bg else None
            gs, gg, gr, gi = neus_composite_backward_raw(rs, mpr, dv["g_pred"], gbg, dv["sdf"], dv["grad"], dv["rgb"], dv["inv"], RATIO)
            tag = "[compat %d%s]" % (compat, "" if with_bg else ", no g_bg")
            check(out, "g_sdf" + tag, gs, ga * op["D_sdf"], c64.compose_bar(ga, bar_ga, op["D_sdf"], op["E_sdf"], op["uf"]), keep)
            check(out, "g_gradients" + tag, gg, ga[:, None] * op["D_grad"],
                  c64.compose_bar(ga[:, None], bar_ga[:, None], op["D_grad"], op["E_grad"], op["uf"][:, None]), keep)
            checkq(out, "g_rgb" + tag, gr, back["g_rgb"], c64.R_GRGB, rays, N)
            # d / d inv_s: m signed terms in no fixed order.  With the needle upstream m is the samples of a few rays; at full
            # size the bar is as wide as m u sum|t| and says little: printed as such
            t = ga * op["D_inv"]
            m = int((t != 0).sum())
            nk = int(op["kink"][t != 0].sum())
            if nk == 0:
                bar = c64.compose_bar(ga, bar_ga, op["D_inv"], op["E_inv"], op["uf"]).sum() + m * c64.U * c64.SLACK * t.abs().sum()
                check(out, "g_inv_s[m = %d]%s" % (m, tag), gi, t.sum().reshape(1), bar.reshape(1))
            else:
                out.append("g_inv_s%s NOT CHECKED: %d kink entries carry a non-zero g_alpha" % (tag, nk))
            # everything but g_inv_s has a fixed summation order: a second run gives the same bits; and the optional outputs off
            gs2, gg2, gr2, gi2 = neus_composite_backward_raw(rs, mpr, dv["g_pred"], gbg, dv["sdf"], dv["grad"], dv["rgb"], dv["inv"], RATIO)
            assert torch.equal(gs, gs2) and torch.equal(gg, gg2) and torch.equal(gr, gr2)
            gs3, n1, n2, n3 = neus_composite_backward_raw(rs, mpr, dv["g_pred"], gbg, dv["sdf"], dv["grad"], dv["rgb"], dv["inv"], RATIO,
                                                          need_grad=False, need_rgb=False, need_inv_s=False)
            assert n1 is None and n2 is None and n3 is None and torch.equal(gs, gs3)
    finally:
        VR.reference_compat = saved
    show("fused neus %s (max_per_ray %d) %s inv_s %g %s" % (cname, mpr, family, inv_s, up), out)


NERF = [("equal%d" % n, None, "dense") for n in cc.EQUAL_COUNTS] + [
    ("ragged", None, "dense"), ("ragged", None, "needle"), ("overflow", None, "dense"), ("cap64", 64, "dense"), ("cap64", 256, "needle"),
    ("cap128", 128, "dense"), ("cap128", 256, "dense"), ("cap256", 256, "needle")]


@pytest.mark.parametrize("cname,max_per_ray,up", NERF)
def test_fused_nerf_composite_every_entry(dev, cname, max_per_ray, up):
    """the background container (dt = 1e10 on each ray's last sample, raw densities -30 .. 25), with and without the foreground"""
    from permuto_sdf import VolumeRendering as VR
    from permuto_sdf_amd import _lib as L
    from permuto_sdf_amd.neus import nerf_composite_backward_raw, nerf_composite_forward_raw
    c = cc.container(cname)
    N, R = c["N"], c["R"]
    raw, dt = cc.nerf_family(c)
    rgb, g_pred, _ = cc.upstream(c, up)
    g = torch.Generator().manual_seed(8)
    fg_pred, fg_bg = torch.rand(R, 3, generator=g), torch.rand(R, 1, generator=g)
    rs = make_rs(c, dev, None, dt)
    rays = c64.Rays(c["start_end"], N)
    mpr = c["max_per_ray"] if max_per_ray is None else max_per_ray
    raw_d, rgb_d = raw.to(dev), rgb.to(dev)
    a, om = torch.empty_like(raw_d), torch.empty_like(raw_d)
    L.call("psdf_nerf_alpha_forward", L.c_l(N), L.ptr(raw_d), L.ptr(dt.view(-1).contiguous().to(dev)), L.ptr(a), L.ptr(om), L.stream())
    st = c64.RayStage(rays, a, om)
    op = c64.nerf_opacity(raw, dt)
    out = []
    q_pb = st.radiance(rgb)
    bar_pb = c64.error_bar(q_pb, c64.R_PRED)
    u, t = g_pred.double(), fg_bg.double()
    for with_fg in (True, False):
        pb, p = nerf_composite_forward_raw(rs, raw_d, rgb_d, *((fg_pred.to(dev), fg_bg.to(dev)) if with_fg else ()))
        check(out, "pred_bg", pb, q_pb.val, bar_pb)
        if with_fg:
            ref = fg_pred.double() + t * q_pb.val                    # pred = fg_pred + fg_bg * pred_bg: a product and a sum
            check(out, "pred", p, ref, t.abs() * bar_pb + c64.U * (t * q_pb.val).abs() + c64.U * ref.abs() + c64.TINY)
        else:
            assert p is None
        up64 = t * u if with_fg else u                               # dL / d pred_bg, rounded once in the kernel
        extra = 1 if with_fg else 0
        saved = VR.reference_compat
        try:
            for compat in (True, False):
                VR.reference_compat = compat
                back = st.backward(rgb, up64, None, compat)
                g_raw, g_rgb, g_fg = nerf_composite_backward_raw(rs, mpr, g_pred.to(dev), raw_d, rgb_d, fg_bg.to(dev) if with_fg else None)
                tag = "[%s, compat %d]" % ("fg" if with_fg else "alone", compat)
                ga = rays.scatter_q(back["g_alpha"], N)
                bar_ga = c64.error_bar(ga, c64.R_RAY_BWD + extra)
                check(out, "g_raw" + tag, g_raw, ga.val * op["D"], c64.compose_bar(ga.val, bar_ga, op["D"], op["E_D"], op["uf"]))
                checkq(out, "g_rgb" + tag, g_rgb, back["g_rgb"], c64.R_GRGB + extra, rays, N)
                if with_fg:                                          # <dL / d pred, pred_bg>: three products of a value with a bar
                    tt = u * q_pb.val
                    check(out, "g_fg_bg", g_fg, tt.sum(1, keepdim=True),
                          (u.abs() * bar_pb).sum(1, keepdim=True) + 4 * c64.U * c64.SLACK * tt.abs().sum(1, keepdim=True) + 3 * c64.TINY)
                else:
                    assert g_fg is None
                again = nerf_composite_backward_raw(rs, mpr, g_pred.to(dev), raw_d, rgb_d, fg_bg.to(dev) if with_fg else None)
                assert torch.equal(g_raw, again[0]) and torch.equal(g_rgb, again[1])
        finally:
            VR.reference_compat = saved
    show("fused nerf %s (max_per_ray %d) %s" % (cname, mpr, up), out)


# ================================================================================================== volume_render_nerf
@pytest.mark.parametrize("cname", ["equal1", "equal65", "equal129", "equal256", "ragged", "overflow"])
def test_volume_render_nerf_and_backward_every_entry(dev, cname):
    from permuto_sdf import VolumeRendering as VR
    c = cc.container(cname)
    N, R = c["N"], c["R"]
    rays = c64.Rays(c["start_end"], N)
    sigma, z, dt = cc.render_nerf_family(c)
    rgb, g_pred, g_bg = cc.upstream(c, "dense")
    rs = make_rs(c, dev, None, dt)
    rs.samples_z = z.to(dev)
    f = c64.render_nerf(rays, rgb, sigma, z, dt)
    ok = ~f["ambiguous"]
    assert int(f["ambiguous"].sum()) <= 0.01 * R
    ok_s = (rays.scatter(ok[:, None].expand(-1, rays.nmax).double(), N) > 0) | ~rays.touched(N)
    pred, depth, bg, w = VR.volume_render_nerf(rs, rgb.to(dev), sigma.to(dev), None, False)
    out = []
    check(out, "pred", pred, f["pred"][0], f["pred"][1], ok)
    check(out, "depth", depth.view(-1), f["depth"][0], f["depth"][1], ok)
    check(out, "bg", bg.view(-1), f["bg"][0], f["bg"][1], ok)
    check(out, "w", w.view(-1), rays.scatter(f["w"][0], N), rays.scatter(f["w"][1], N), ok_s)
    g_rgb, g_sigma = VR.volume_render_nerf_backward(g_pred.to(dev), g_bg.to(dev), None, pred, rs, rgb.to(dev), sigma.to(dev), None, False, bg)
    (vr, br), (vs, bs) = c64.render_nerf_backward(rays, f, g_pred, g_bg, pred, bg)
    check(out, "g_rgb", g_rgb, rays.scatter(vr, N), rays.scatter(br, N), ok_s)
    check(out, "g_sigma", g_sigma.view(-1), rays.scatter(vs, N), rays.scatter(bs, N), ok_s)
    show("volume_render_nerf %s (%d rays stop early, %d excluded)" % (cname, int((f["use"].sum(1) < rays.cnt).sum()), int(f["ambiguous"].sum())), out)


# ================================================================================================ the autograd wrappers
def test_autograd_wrappers_under_the_same_bar(dev):
    """neus_composite / nerf_composite once each on a container with holes and an overflowing tail, so the host plumbing (the
    zero fill of `_per_sample` on non-dense containers, the need_* routing) sits under the same per-entry bar"""
    from permuto_sdf import VolumeRendering as VR
    from permuto_sdf_amd import _lib as L
    from permuto_sdf_amd.neus import nerf_composite, neus_composite
    c, host, rs, dv, a, om, rays = _neus_setup(dev, "overflow", "cross", 300.0, "dense")
    sdf, dirs, grad, dt, rgb, g_pred, g_bg = host
    N, out = c["N"], []
    compat = bool(VR.reference_compat)
    sdf_g, grad_g, rgb_g = dv["sdf"].clone().requires_grad_(True), dv["grad"].clone().requires_grad_(True), dv["rgb"].clone().requires_grad_(True)
    inv_g = dv["inv"].clone().requires_grad_(True)
    pred, bg = neus_composite(rs, c["max_per_ray"], sdf_g, grad_g, rgb_g, inv_g, RATIO)
    ((pred * dv["g_pred"]).sum() + (bg * dv["g_bg"]).sum()).backward()
    st, back, op, ga, bar_ga = _fused_neus_bars(c, host, a, om, rays, 300.0, compat, True)
    keep = ~op["kink"]
    checkq(out, "pred", pred, st.radiance(rgb), c64.R_PRED)
    checkq(out, "bg", bg, st.transmittance()[1], c64.R_T)
    check(out, "sdf.grad", sdf_g.grad, ga * op["D_sdf"], c64.compose_bar(ga, bar_ga, op["D_sdf"], op["E_sdf"], op["uf"]), keep)
    check(out, "gradients.grad", grad_g.grad, ga[:, None] * op["D_grad"],
          c64.compose_bar(ga[:, None], bar_ga[:, None], op["D_grad"], op["E_grad"], op["uf"][:, None]), keep)
    checkq(out, "rgb.grad", rgb_g.grad, back["g_rgb"], c64.R_GRGB, rays, N)
    assert inv_g.grad is not None and inv_g.grad.shape == (1,)
    t = ga * op["D_inv"]
    assert int(op["kink"][t != 0].sum()) == 0                       # condition of this one case (seeded on the CPU): no kink entry
    bar = c64.compose_bar(ga, bar_ga, op["D_inv"], op["E_inv"], op["uf"]).sum() + int((t != 0).sum()) * c64.U * c64.SLACK * t.abs().sum()
    check(out, "inv_s.grad[m = %d]" % int((t != 0).sum()), inv_g.grad, t.sum().reshape(1), bar.reshape(1))
    # only sdf needs a gradient: the others come back as None, sdf.grad keeps its bits
    sdf_h = dv["sdf"].clone().requires_grad_(True)
    pred2, bg2 = neus_composite(rs, c["max_per_ray"], sdf_h, dv["grad"], dv["rgb"], dv["inv"], RATIO)
    ((pred2 * dv["g_pred"]).sum() + (bg2 * dv["g_bg"]).sum()).backward()
    assert torch.equal(sdf_h.grad, sdf_g.grad)
    untouched = ~rays.touched(N)
    assert float(sdf_g.grad.cpu().view(-1)[untouched].abs().max()) == 0.0 and float(rgb_g.grad.cpu()[untouched].abs().max()) == 0.0
    show("neus_composite (autograd) overflow cross 300", out)

    out = []
    raw, dtb = cc.nerf_family(c)
    rs.samples_dt = dtb.to(dev)
    g = torch.Generator().manual_seed(9)
    fg_pred, fg_bg = torch.rand(c["R"], 3, generator=g), torch.rand(c["R"], 1, generator=g)
    raw_g, rgb_g = raw.to(dev).requires_grad_(True), dv["rgb"].clone().requires_grad_(True)
    fp_g, fb_g = fg_pred.to(dev).requires_grad_(True), fg_bg.to(dev).requires_grad_(True)
    p = nerf_composite(rs, c["max_per_ray"], raw_g, rgb_g, fp_g, fb_g)
    (p * dv["g_pred"]).sum().backward()
    an, omn = torch.empty(N, device=dev), torch.empty(N, device=dev)
    L.call("psdf_nerf_alpha_forward", L.c_l(N), L.ptr(raw.to(dev)), L.ptr(dtb.view(-1).contiguous().to(dev)), L.ptr(an), L.ptr(omn), L.stream())
    st = c64.RayStage(rays, an, omn)
    opn = c64.nerf_opacity(raw, dtb)
    back = st.backward(rgb, fg_bg.double() * g_pred.double(), None, compat)
    gan = rays.scatter_q(back["g_alpha"], N)
    bar = c64.error_bar(gan, c64.R_RAY_BWD + 1)
    check(out, "raw.grad", raw_g.grad, gan.val * opn["D"], c64.compose_bar(gan.val, bar, opn["D"], opn["E_D"], opn["uf"]))
    checkq(out, "rgb.grad", rgb_g.grad, back["g_rgb"], c64.R_GRGB + 1, rays, N)
    assert torch.equal(fp_g.grad, dv["g_pred"]) and fb_g.grad.shape == (c["R"], 1)
    assert float(raw_g.grad.cpu()[untouched].abs().max()) == 0.0
    show("nerf_composite (autograd) overflow", out)
