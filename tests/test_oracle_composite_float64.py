"""CPU: the float64 evaluator of the compositing stage (oracle/composite_float64.py) is pinned before any GPU test trusts it.

  * where the conventions coincide (no clamp active, reference_compat off, equal counts) it equals float64 autograd through the
    reference's torch expressions (oracle/neus_oracle.py) to 1e-9;
  * where they do not -- a surface crossing at inv_s 1000, where 1 - alpha + 1e-7 falls below 1e-6 -- it differs from autograd
    by exactly the clamp factor om / max(om, 1e-6) on exactly the clamped samples;
  * the per-operator forward / backward kernels of the C restatement (and of the reference's own kernels where they were built)
    stay inside the per-operator bars on a ragged container with holes and an overflowing pool;
  * a SERIAL fp32 restatement (numpy, one sample after the other) of the ray stage stays inside the bar of the same form with
    ITS rounding counts (i multiplications for T_i), and torch's fp32 evaluation of the two opacities inside the running-error
    bounds: the form of the bar holds with no kernel in the loop;
  * the exclusion cap (relu kinks: 0.1 % of a case) and the "bites" share (>= 50 % of the ray-stage entries of the surface
    crossing cases have a bar below 1e-3 of the entry, with the KERNELS' rounding counts) hold for every input family of
    tests/test_gpu_composite_float64.py.
Nothing is tuned to a measured figure; the measured worst error / bar and the shares are printed (-s)."""
import numpy as np
import pytest
import torch

from oracle import composite_cases as cc
from oracle import composite_float64 as c64
from oracle import neus_oracle as no

f32 = np.float32


def worst(got, q, r, name, bar=None):
    bar = c64.error_bar(q, r) if bar is None else bar
    val = q.val if isinstance(q, c64.Q) else q
    err = (torch.as_tensor(got).double().reshape(val.shape) - val).abs()
    ratio = float((err / bar.clamp_min(1e-300)).max()) if err.numel() else 0.0
    assert bool((err <= bar).all()), "%s: worst error / bar %.3g" % (name, ratio)
    return ratio


def test_equals_float64_autograd_where_the_conventions_coincide(monkeypatch):
    # (the evaluator holds 1e-5 and 1e-7 as the fp32 numbers the kernels hold; autograd through the float64 expressions holds the
    #  float64 ones: 2.5e-8 apart, relatively.  For this comparison alone the evaluator gets the float64 constants.)
    monkeypatch.setattr(c64, "C_1EM5", 1e-5)
    monkeypatch.setattr(c64, "C_1EM7", 1e-7)
    c = cc.container("equal48")
    R, n, N = c["R"], 48, c["N"]
    sdf, dirs, grad, dt = cc.neus_family(c, "noise")
    rgb, g_pred, g_bg = cc.upstream(c, "dense")
    inv_s, ratio = torch.tensor(300.0), 0.6
    s64, gr64, rgb64 = sdf.double().requires_grad_(True), grad.double().requires_grad_(True), rgb.double().requires_grad_(True)
    inv64 = inv_s.double().requires_grad_(True)
    a, om = no.neus_alpha(s64, dirs.double(), gr64, dt.double(), inv64, c64._f32(ratio))
    assert float(om.detach().min()) > 1e-6                              # the clamp of the reference's backward is inactive
    pred, w, T = no.composite_equal(a, om, rgb64, R, n, reference_compat=False)
    bg = T.view(R, n)[:, -1:]
    ((pred * g_pred.double()).sum() + (bg * g_bg.double()).sum()).backward()
    op = c64.neus_opacity(sdf, dirs, grad, dt, inv_s, ratio)
    rays = c64.Rays(c["start_end"], N)
    st = c64.RayStage(rays, op["alpha"], 1 - op["alpha"] + 1e-7)     # the float64 opacity of the autograd chain, not an fp32 one
    back = st.backward(rgb, g_pred, g_bg, compat=False)
    ga = rays.scatter(back["g_alpha"].val, N)

    def same(x, ref, name):
        assert float((x - ref.reshape(x.shape)).abs().max()) <= 1e-9 * float(ref.abs().max()), name
    same(op["alpha"], a.detach(), "alpha")
    same(rays.scatter(st.transmittance()[0].val, N), T.detach(), "T")
    same(rays.scatter(st.weights().val, N), w.detach(), "w")
    same(st.radiance(rgb).val, pred.detach(), "pred")
    same(rays.scatter(back["g_rgb"].val, N), rgb64.grad, "g_rgb")
    same(ga * op["D_sdf"], s64.grad, "g_sdf")
    same(ga[:, None] * op["D_grad"], gr64.grad, "g_gradients")
    same((ga * op["D_inv"]).sum(), inv64.grad, "g_inv_s")
    assert int(op["kink"].sum()) == 0


def test_differs_from_autograd_by_the_clamp_factor_on_the_clamped_samples():
    c = cc.container("equal128")
    R, n, N = c["R"], 128, c["N"]
    sdf, dirs, grad, dt = cc.neus_family(c, "cross")
    rgb, g_pred, g_bg = cc.upstream(c, "dense")
    a32, om32 = no.neus_alpha(sdf, dirs, grad, dt, torch.tensor(1000.0), 0.6)             # fp32, as the kernels hand them on
    clamped = om32.view(-1) < 1e-6
    assert float(clamped.float().mean()) > 0.2
    a64, om64 = a32.double().requires_grad_(True), om32.double().requires_grad_(True)
    pred, w, T = no.composite_equal(a64, om64, rgb.double(), R, n, reference_compat=False)
    ((pred * g_pred.double()).sum() + (T.view(R, n)[:, -1:] * g_bg.double()).sum()).backward()
    rays = c64.Rays(c["start_end"], N)
    back = c64.RayStage(rays, a32, om32).backward(rgb, g_pred, g_bg, compat=False)
    g_om = rays.scatter(back["g_om"].val, N)
    auto = om64.grad.view(-1)
    last = torch.zeros(N, dtype=torch.bool)
    last[n - 1::n] = True
    factor = om32.double().view(-1) / om32.double().view(-1).clamp_min(c64.C_1EM6)
    assert float((g_om - auto * factor)[~last].abs().max()) <= 1e-9 * float(g_om.abs().max())
    differs = ((g_om - auto).abs() > 1e-9 * auto.abs()) & ~last         # (float64 noise of two evaluation orders aside)
    assert bool((differs <= clamped).all())                         # only clamped samples differ ...
    touched = clamped & (auto != 0) & ~last
    assert bool((g_om[touched].abs() < auto[touched].abs()).all()) and int(touched.sum()) > 100     # ... and every one of them does
    # the weight path is the same in both
    ga = rays.scatter(back["g_alpha"].val, N)
    assert float((ga + g_om - a64.grad.view(-1)).abs().max()) <= 1e-9 * float(a64.grad.abs().max())


def _samples(c):
    from oracle import oracle as O
    s = O.Samples(c["R"], c["N"])
    s.start_end[:] = c["start_end"].numpy()
    return s


@pytest.mark.parametrize("name", ["ragged", "overflow"])
def test_per_operator_kernels_of_the_c_restatement_stay_inside_the_operator_bars(name):
    from oracle import oracle as O
    c = cc.container(name)
    N = c["N"]
    rays = c64.Rays(c["start_end"], N)
    assert int((~rays.valid).sum()) >= (24 if name == "overflow" else 20)     # empty rays (and the pool's overflowing tail)
    sdf, dirs, grad, dt = cc.neus_family(c, "cross")
    rgb, g_pred, g_bg = cc.upstream(c, "dense")
    a32, om32 = no.neus_alpha(sdf, dirs, grad, dt, torch.tensor(300.0), 0.6)
    s = _samples(c)
    kinds = ["port"] + (["ref"] if O.have_ref() else [])
    for kind in kinds:
        orc = O.Oracle(kind)
        st = c64.RayStage(rays, a32, om32, t_mults=c64.serial_mults)
        T, bg = orc.cumprod(s, om32.numpy())
        qT, qbg = st.transmittance()
        out = {"T": worst(T[:, 0], rays.scatter_q(qT, N), c64.R_T, "T"), "bg": worst(bg[:, 0], qbg, c64.R_T, "bg")}
        assert bool((bg[~rays.valid.numpy()] == 1).all()) and bool((T[~rays.touched(N).numpy()] == 0).all())
        w = torch.from_numpy(T) * a32
        pred = orc.integrate(s, rgb.numpy(), w.numpy())
        out["pred"] = worst(pred, c64.op_integrate(rays, rgb, w), c64.R_OP_INTEGRATE, "pred")
        for compat in ((True, False) if kind == "port" else (True,)):
            g_rgb, g_w = orc.integrate_backward(s, g_pred.numpy(), rgb.numpy(), w.numpy(), compat) if kind == "port" else \
                orc.integrate_backward(s, g_pred.numpy(), rgb.numpy(), w.numpy())
            q_rgb, q_w = c64.op_integrate_backward(rays, g_pred, rgb, w, compat)
            out["g_rgb"] = worst(g_rgb, rays.scatter_q(q_rgb, N), c64.R_OP_GRGB, "g_rgb")
            out["g_w c%d" % compat] = worst(g_w[:, 0], rays.scatter_q(q_w, N), c64.R_GW, "g_w")
        g_w = torch.from_numpy(g_w)
        v = (g_w * a32) * torch.from_numpy(T)
        for inverse in (False, True):
            cs = orc.cumsum(s, v.numpy(), inverse)
            out["cumsum%d" % inverse] = worst(cs[:, 0], rays.scatter_q(c64.op_cumsum(rays, v, inverse), N), c64.R_OP_SUM, "cumsum")
        cdf = orc.compute_cdf(s, w.numpy())
        out["cdf"] = worst(cdf[:, 0], rays.scatter_q(c64.op_cumsum(rays, w, False, True), N), c64.R_OP_SUM, "cdf")
        s_ray, s_smp = orc.sum_over_each_ray(s, rgb.numpy())
        q_ray, q_smp = c64.op_sum(rays, rgb)
        out["sum"] = max(worst(s_ray, q_ray, c64.R_OP_SUM, "sum per ray"), worst(s_smp, rays.scatter_q(q_smp, N), c64.R_OP_SUM, "sum per sample"))
        g_om = orc.cumprod_backward(s, (g_w * a32).numpy(), g_bg.numpy(), om32.numpy(), T, bg, cs)
        out["g_om"] = worst(g_om[:, 0], rays.scatter_q(c64.op_cumprod_backward(rays, g_bg, om32, torch.from_numpy(bg), torch.from_numpy(cs)), N),
                            c64.R_OP_CUMPROD_BWD, "g_om")
        print("%s / %s: worst error / bar " % (name, kind) + ", ".join("%s %.3f" % kv for kv in out.items()))


def serial_fp32(c, a, om, rgb, g_pred, g_bg, compat):
    """the ray stage one sample after the other in numpy fp32 (T_i = T_{i-1} * om_{i-1}: the reference's loop order,
    VolumeRenderingGPU.cuh:401-417, :1160-1190) -> packed fp32 arrays"""
    N = c["N"]
    a, om, rgb = a.numpy().reshape(-1).astype(f32), om.numpy().reshape(-1).astype(f32), rgb.numpy().astype(f32)
    T, w, g_alpha, g_rgb = np.zeros(N, f32), np.zeros(N, f32), np.zeros(N, f32), np.zeros((N, 3), f32)
    pred, bg = np.zeros((c["R"], 3), f32), np.ones(c["R"], f32)
    for r in range(c["R"]):
        s, e = int(c["start_end"][r, 0]), int(c["start_end"][r, 1])
        if e > N or e == s:
            continue
        t = f32(1.0)
        for i in range(s, e):
            T[i] = t
            w[i] = a[i] * t
            pred[r] += w[i] * rgb[i]
            if i < e - 1:
                t = f32(t * om[i])
        bg[r] = T[e - 1]
        gp = g_pred[r].numpy().astype(f32)
        gb = f32(f32(g_bg[r, 0].item()) * bg[r])
        cs = f32(0.0)
        for i in range(e - 1, s - 1, -1):
            cq = np.array([rgb[i, 0], rgb[i, 1], rgb[i, 1] if compat else rgb[i, 2]], f32)
            gw = f32(f32(f32(gp[0] * cq[0]) + f32(gp[1] * cq[1])) + f32(gp[2] * cq[2]))
            g_rgb[i] = gp * w[i]
            g_om = f32(0.0)
            if i < e - 1:
                omc = max(om[i], f32(1e-6))
                g_om = f32(f32(cs / omc) + f32(gb / omc))
            g_alpha[i] = f32(f32(gw * T[i]) - g_om)
            cs = f32(cs + f32(f32(gw * a[i]) * T[i]))
    return dict(T=T, w=w, pred=pred, bg=bg, g_alpha=g_alpha, g_rgb=g_rgb)


CROSS = [("equal48", 1000.0), ("equal65", 1000.0), ("cap128", 1000.0), ("equal128", 64.0), ("equal128", 300.0), ("equal256", 1000.0), ("ragged", 300.0), ("equal193", 1e6), ("overflow", 1000.0)]


@pytest.mark.parametrize("name,inv_s", CROSS)
@pytest.mark.parametrize("up", ["dense", "needle"])
def test_serial_fp32_restatement_inside_the_bar_and_the_bar_bites(name, inv_s, up):
    c = cc.container(name)
    N = c["N"]
    rays = c64.Rays(c["start_end"], N)
    sdf, dirs, grad, dt = cc.neus_family(c, "cross")
    rgb, g_pred, g_bg = cc.upstream(c, up)
    a32, om32 = no.neus_alpha(sdf, dirs, grad, dt, torch.tensor(inv_s), 0.6)
    live = rays.touched(N)
    saturated = float((a32.view(-1)[live] == 1).float().mean())
    # the regime: saturated opacity ... (from inv_s 300 on: at 64 the sigmoid arguments of this family end at -22, and alpha == 1.0f
    # needs the second sigmoid below half an ulp of 1e-5, an argument below -28: the share there is 0 and is only printed)
    assert saturated >= 0.2 or inv_s < 300
    for compat in (True, False):
        lo = serial_fp32(c, a32, om32, rgb, g_pred, g_bg, compat)
        st = c64.RayStage(rays, a32, om32, t_mults=c64.serial_mults)
        qT, qbg = st.transmittance()
        back = st.backward(rgb, g_pred, g_bg, compat)
        out = {"T": worst(lo["T"], rays.scatter_q(qT, N), c64.R_T, "T"), "bg": worst(lo["bg"], qbg, c64.R_T, "bg"),
               "w": worst(lo["w"], rays.scatter_q(st.weights(), N), c64.R_W, "w"),
               "pred": worst(lo["pred"], st.radiance(rgb), c64.R_PRED, "pred"),
               "g_rgb": worst(lo["g_rgb"], rays.scatter_q(back["g_rgb"], N), c64.R_GRGB, "g_rgb"),
               "g_alpha": worst(lo["g_alpha"], rays.scatter_q(back["g_alpha"], N), c64.R_RAY_BWD, "g_alpha")}
        assert float(lo["T"][live.numpy()].min()) < c64.TINY or inv_s < 300   # ... and a transmittance that leaves the fp32 normals
    # the bars the KERNELS are held to (scan_mults) bite
    st = c64.RayStage(rays, a32, om32)
    back = st.backward(rgb, g_pred, g_bg, True)
    shares = {}
    for k, q, r in (("T", st.transmittance()[0], c64.R_T), ("w", st.weights(), c64.R_W), ("g_alpha", back["g_alpha"], c64.R_RAY_BWD)):
        shares[k] = c64.bites(q.val, c64.error_bar(q, r))
        if up == "dense":
            assert shares[k][0] >= 0.5, (k, shares[k])
    print("%s inv_s %g %s: alpha == 1 on %.1f%%; serial fp32 worst error / bar " % (name, inv_s, up, 100 * saturated) + ", ".join("%s %.3f" % kv for kv in out.items()) +
          " | kernel-count bars: bites / saturated " + ", ".join("%s %.1f%% / %.1f%%" % (k, 100 * v[0], 100 * v[1]) for k, v in shares.items()))


FAMILIES = [("noise", 300.0), ("cross", 64.0), ("cross", 300.0), ("cross", 1000.0), ("cross", 1e6), ("grazing", 300.0)]


@pytest.mark.parametrize("family,inv_s", FAMILIES)
def test_opacity_bounds_hold_for_torch_fp32_and_the_exclusion_cap_is_met(family, inv_s):
    c = cc.container("ragged")
    sdf, dirs, grad, dt = cc.neus_family(c, family)
    N = c["N"]
    op = c64.neus_opacity(sdf, dirs, grad, dt, torch.tensor(inv_s), 0.6)
    assert int(op["kink"].sum()) <= 1e-3 * N, int(op["kink"].sum())
    assert float(op["q"].min()) > 0 and float(op["q"].max()) <= 1    # section(): ic <= 0, so nc <= pc and q lies in (0, 1]
    if family == "grazing":
        tc = op["tc"]
        assert float((tc < 0).float().mean()) > 0.05 and float((tc > 1).float().mean()) > 0.05
    keep = ~op["kink"]
    s_, g_ = sdf.clone().requires_grad_(True), grad.clone().requires_grad_(True)
    inv = torch.full((N, 1), inv_s).requires_grad_(True)
    a, om = no.neus_alpha(s_, dirs, g_, dt, inv, 0.6)
    a.sum().backward()
    out = {"alpha": worst(a.detach().view(-1)[keep], op["alpha"][keep], 0, "alpha", op["E_alpha"][keep]),
           "om": worst(om.detach().view(-1)[keep], op["om"][keep], 0, "om", op["E_om"][keep]),
           "d/d sdf": worst(s_.grad.view(-1)[keep], op["D_sdf"][keep], 0, "D_sdf", op["E_sdf"][keep] + c64.TINY * op["uf"][keep]),
           "d/d gradients": worst(g_.grad[keep], op["D_grad"][keep], 0, "D_grad", op["E_grad"][keep] + c64.TINY * op["uf"][keep, None]),
           "d/d inv_s": worst(inv.grad.view(-1)[keep], op["D_inv"][keep], 0, "D_inv", op["E_inv"][keep] + c64.TINY * op["uf"][keep])}
    sh = {k: c64.bites(op[v][keep], op[e][keep]) for k, v, e in (("alpha", "alpha", "E_alpha"), ("d/d sdf", "D_sdf", "E_sdf"), ("d/d tc", "D_tc", "E_tc"))}
    print("%s inv_s %g: excluded (kink) %d of %d; torch fp32 worst error / bound " % (family, inv_s, int(op["kink"].sum()), N) +
          ", ".join("%s %.3f" % kv for kv in out.items()) + " | bites / saturated " +
          ", ".join("%s %.1f%% / %.1f%%" % (k, 100 * v[0], 100 * v[1]) for k, v in sh.items()))


def test_nerf_opacity_bounds_hold_for_torch_fp32():
    c = cc.container("ragged")
    raw, dt = cc.nerf_family(c)
    assert float(raw.min()) < -29 and float(raw.max()) > 24 and int((dt == 1e10).sum()) == int((c["counts"] > 0).sum())
    op = c64.nerf_opacity(raw, dt)
    x = raw.clone().requires_grad_(True)
    a = 1.0 - torch.exp(-torch.nn.functional.softplus(x) * dt.view(-1))
    om = 1 - a + 1e-7
    a.sum().backward()
    out = {"alpha": worst(a.detach(), op["alpha"], 0, "alpha", op["E_alpha"]), "om": worst(om.detach(), op["om"], 0, "om", op["E_om"]),
           "d/d raw": worst(x.grad, op["D"], 0, "D", op["E_D"] + c64.TINY * op["uf"])}
    print("nerf opacity: torch fp32 worst error / bound " + ", ".join("%s %.3f" % kv for kv in out.items()) +
          " | bites / saturated alpha %.1f%% / %.1f%%, d/d raw %.1f%% / %.1f%%" % tuple(
              100 * v for v in c64.bites(op["alpha"], op["E_alpha"]) + c64.bites(op["D"], op["E_D"])))


RENDER_NERF = ["equal1", "equal65", "equal129", "equal256", "ragged", "overflow"]


@pytest.mark.parametrize("name", RENDER_NERF)
def test_volume_render_nerf_of_the_c_restatement_inside_the_bar_and_the_exclusion_cap(name):
    """volume_render_nerf and its backward: the serial fp32 C restatement (and the reference's own kernel where built) against the
    evaluator, with the serial rounding counts and libm's expf; rays whose transmittance comes within its own bar of the 1e-4
    early-out are left out, and the float64 evaluator alone shows that they stay under 1 % of the rays of every GPU case."""
    from oracle import oracle as O
    c = cc.container(name)
    N = c["N"]
    rays = c64.Rays(c["start_end"], N)
    sigma, z, dt = cc.render_nerf_family(c)
    rgb, g_pred, g_bg = cc.upstream(c, "dense")
    s = _samples(c)
    s.z[:], s.dt[:] = z.numpy(), dt.numpy()
    kernel_view = c64.render_nerf(rays, rgb, sigma, z, dt)             # the counts and the __expf figure the GPU test uses
    assert int(kernel_view["ambiguous"].sum()) <= 0.01 * c["R"]
    stopped = int((kernel_view["use"].sum(1) < rays.cnt).sum())
    assert stopped >= (1 if c["max_per_ray"] >= 65 else 0)
    for kind in ["port"] + (["ref"] if O.have_ref() else []):
        orc = O.Oracle(kind)
        f = c64.render_nerf(rays, rgb, sigma, z, dt, c64.serial_mults, c64.ULP_EXPF)
        ok = ~f["ambiguous"]
        assert int(f["ambiguous"].sum()) <= 0.01 * c["R"]
        ok_s = (rays.scatter(ok[:, None].expand(-1, rays.nmax).double(), N) > 0) | ~rays.touched(N)
        pred, depth, bg, w = orc.volume_render_nerf(s, rgb.numpy(), sigma.numpy())
        out = {"pred": worst(pred[ok], f["pred"][0][ok], 0, "pred", f["pred"][1][ok]),
               "depth": worst(depth[:, 0][ok], f["depth"][0][ok], 0, "depth", f["depth"][1][ok]),
               "bg": worst(bg[:, 0][ok], f["bg"][0][ok], 0, "bg", f["bg"][1][ok]),
               "w": worst(w[:, 0][ok_s], rays.scatter(f["w"][0], N)[ok_s], 0, "w", rays.scatter(f["w"][1], N)[ok_s])}
        g_rgb, g_sigma = orc.volume_render_nerf_backward(s, g_pred.numpy(), g_bg.numpy(), pred, bg, rgb.numpy(), sigma.numpy())
        (vr, br), (vs, bs) = c64.render_nerf_backward(rays, f, g_pred, g_bg, torch.from_numpy(pred), torch.from_numpy(bg))
        out["g_rgb"] = worst(g_rgb[ok_s], rays.scatter(vr, N)[ok_s], 0, "g_rgb", rays.scatter(br, N)[ok_s])
        out["g_sigma"] = worst(g_sigma[:, 0][ok_s], rays.scatter(vs, N)[ok_s], 0, "g_sigma", rays.scatter(bs, N)[ok_s])
        print("volume_render_nerf %s / %s: %d rays stop early, %d excluded; worst error / bar " % (name, kind, stopped, int(f["ambiguous"].sum())) +
              ", ".join("%s %.3f" % kv for kv in out.items()))
