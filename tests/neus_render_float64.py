"""FLOAT64 EVALUATOR of the NeuS render with its per-ray weight sum and of the masked step's loss tail (csrc/neus_render.hip).  A
helper of tests/test_neus_render_host.py and tests/test_gpu_neus_render.py: no test lives here.

Plain torch float64 on the CPU, NO AUTOGRAD: values and gradients are written out.  Inputs are fp32 tensors taken exactly.  Built on
oracle/composite_float64.py: `Rays` (the padded view of a packed container), `neus_opacity` (section() + clip and the backward
expressions for g = 1, each with its running error bound), `RayStage` + `error_bar` (pred and bg of a ray stage on exact fp32
opacities, the bars the fused composite kernels are already held to) and `compose_bar`.

THE RENDER (render).  For a ray of n samples with the section-point opacity a_i = clip01(q_i) (composite_device.h):
    om_i = (1 - a_i) + 1e-7,   T_i = prod_{j < i} om_j,   w_i = a_i T_i
    pred = sum w_i c_i,   weights_sum = sum w_i,   bg = T_{n-1}       (the LAST sample's factor never enters: cumprod_fwd_kernel)
and for upstream gradients g_pred [3], g_ws, g_bg of the ray (each may be absent = 0):
    g_w_i = <g_pred, c_i> + g_ws         (reference_compat: the third colour channel is read as the second, VolumeRenderingGPU.cuh:1247)
    v_i = g_w_i a_i T_i,   g_om_i = (sum_{j > i} v_j + g_bg bg) / max(om_i, 1e-6) for i < n - 1, 0 for the last sample
    g_alpha_i = g_w_i T_i - g_om_i,   g_rgb_i = g_pred w_i
    g_sdf_i = g_alpha_i D_sdf_i,  g_gradients_i = g_alpha_i D_tc_i dir_i,  g_inv_s = sum_i g_alpha_i D_inv_i      (neus_opacity's D)
Empty rays and rays whose range passes the pool: pred 0, weights_sum 0, bg 1, their samples untouched.  With the floor 1e-6
inactive and reference_compat off this is the derivative of the forward (tests/test_neus_render_host.py holds it against torch
autograd of VolumeRenderingNeus.compute_weights + integrate restated in torch operators).

BARS.  u = 2^-24.  The first-order running error analysis of tests/nerf_render_float64.py (same ray stage, same formulas: T, w, the
sums in any order, g_w with its four terms, v, the suffix sums, g_om, g_alpha) on top of neus_opacity's E_alpha, E_om; the
composition with the opacity backward is compose_bar of the oracle; g_inv_s is a signed sum of m terms in no fixed order: the sum
of the terms' bars + m u sum |t|.  The analysis is valid while E_om / om stays small: `family("float64")` keeps every om above 1e-4
(checked on the CPU) and every true_cos away from the relu kinks of section() (neus_opacity's `kink`: none in this family).  With
`alpha=, om=` given -- the fp32 values psdf_neus_alpha_forward returned, whose bits the fused kernels form
(test_gpu_composite_float64.py::test_fused_kernels_form_the_opacity_bits_of_the_opacity_kernels) -- the same formulas run as a pure
RAY STAGE on exact inputs (E_a = E_om = 0, the floor evaluated as the kernels evaluate it): valid at any saturation; pred and bg
then carry RayStage's bars.

THE LOSS TAIL (mask_loss).  loss = base + mean over 3 R of |pred - gt| hit + weight mean over R of -(t log c + (1 - t) log(1 - c)),
c = clip(ws, lo, hi) with the fp32 bounds the kernel holds;  g_pred = sign(pred - gt) hit / (3 R);  g_ws = weight (c - t) / ((1 - c)
c) / R where lo <= ws <= hi (torch.clamp passes the gradient AT a bound), else 0.  Rows are fp32, the sums double: an absolute
error row 1 rounding, the two fp32 scales 1 each, a g_pred entry 1 (the scale); log: ULP_LOGF ulps on an argument that is exact (c)
or carries u (1 - c); a g_ws entry 7 roundings on a quotient whose factors are bounded away from 0 by the clip; the sum is
converted to fp32 and added to the accumulator: 2 roundings of the result."""
import torch

from oracle import composite_float64 as c64
from oracle.composite_float64 import SLACK, TINY, U, _f32
from tests.nerf_render_float64 import RAY_COUNTS, SUBSETS, container, rays_of, upstream   # the containers and upstreams of the NeRF render

C_1EM5, C_1EM6, C_1EM7 = c64.C_1EM5, c64.C_1EM6, c64.C_1EM7
CLIP_LO, CLIP_HI = _f32(1e-3), _f32(1.0 - 1e-3)
ULP_LOGF = 2
RATIO = 0.6
INV_S = 64.0
__all__ = ["RAY_COUNTS", "SUBSETS", "container", "rays_of", "upstream", "family", "render", "render_torch", "mask_loss",
           "mask_loss_torch", "mask_loss_cases"]


def family(c, kind="float64", seed=0):
    """-> sdf [N, 1], dirs [N, 3], gradients [N, 3], dt [N, 1], rgb [N, 3], inv_s [1]
    float64   : sdf in [-0.05, 0.1], the SDF gradient within 0.2 of -0.9 dir (true_cos near -0.9: far from the relu kinks at 0 and
                1), dt in [1e-3, 0.01], inv_s 64: alpha <= 0.45, om >= 0.55
    saturated : sdf falling from 0.3 to -0.3 along every ray at inv_s 1000: alpha == 1.0f behind the surface, T underflows"""
    g = torch.Generator().manual_seed(7100 + seed)
    N = c["N"]
    rgb = torch.rand(N, 3, generator=g)
    dirs = torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=-1)
    grad = -0.9 * dirs + 0.2 * (torch.rand(N, 3, generator=g) - 0.5)
    if kind == "float64":
        sdf = torch.rand(N, 1, generator=g) * 0.15 - 0.05
        dt = torch.rand(N, 1, generator=g) * 0.009 + 1e-3
        return sdf, dirs, grad, dt, rgb, torch.tensor([INV_S])
    if kind != "saturated":
        raise ValueError(kind)
    rays = rays_of(c)
    frac = (rays.pos.double() / rays.cnt.clamp_min(2)[:, None].double())
    sdf = rays.scatter(0.3 - 0.6 * frac, N).float().view(N, 1) + 0.01 * torch.randn(N, 1, generator=g)
    dt = torch.rand(N, 1, generator=g) * 0.004 + 1e-3
    return sdf, dirs, grad, dt, rgb, torch.tensor([1000.0])


def _d(t):
    return t.detach().cpu().double()


# ------------------------------------------------------------------------------------------------------------- the render
def render(rays, sdf, dirs, gradients, dt, rgb, inv_s, ratio=RATIO, g_pred=None, g_ws=None, g_bg=None, compat=False, alpha=None, om=None):
    """-> dict name -> (float64 value, bar): pred [R, 3], weights_sum [R], bg [R], and with an upstream gradient g_sdf [N],
    g_gradients [N, 3], g_rgb [N, 3], g_inv_s [1] (0 with bar 0 on slots no processed ray owns); `min_om`: the smallest
    1 - alpha + 1e-7 of a processed sample; `kink` [N] bool: entries neus_opacity excludes.
    alpha, om (fp32, from psdf_neus_alpha_forward): run as a ray stage on these exact inputs (see the module docstring)."""
    N = sdf.shape[0]
    op = c64.neus_opacity(sdf, dirs, gradients, dt, inv_s, ratio)
    k, R, nmax = rays.mask, rays.R, rays.nmax
    kd = k.double()
    stage = alpha is not None
    if not stage:
        A, E_A = rays.gather(op["alpha"]), rays.gather(op["E_alpha"])
        OM, E_OM = rays.gather(op["om"]), rays.gather(op["E_om"])
    else:
        A, OM = rays.gather(_d(alpha)), rays.gather(_d(om))
        E_A = E_OM = torch.zeros_like(A)
    OM = torch.where(k, OM, torch.ones_like(OM))
    inner = k & ~rays.is_last
    fac = torch.where(inner, OM, torch.ones_like(OM))
    one = torch.ones(R, 1, dtype=torch.float64)
    T = torch.cat([one, torch.cumprod(fac, 1)[:, :-1]], 1) * kd
    rel_om = torch.where(inner, E_OM / OM, torch.zeros_like(OM))
    RT = c64.scan_mults(rays.pos).double().expand(R, nmax)
    relT = torch.cat([0 * one, torch.cumsum(rel_om, 1)[:, :-1]], 1) + RT * U
    E_T = (T * torch.expm1(relT.clamp_max(700.0)) * SLACK + RT * TINY) * kd
    C = rays.gather(rgb)
    w = A * T
    E_w = (E_A * T + A.abs() * E_T + U * w.abs() + TINY) * kd
    m = rays.cnt.double()

    def ray_sum(t, E, r):          # t, E [R, nmax(, c)] -> value and bar of the sum over the ray, any order
        return t.sum(1), (E.sum(1) + ((m + r) * U).view(-1, *([1] * (t.dim() - 2))) * t.abs().sum(1)) * SLACK + \
            (m * TINY).view(-1, *([1] * (t.dim() - 2)))
    valid = rays.valid.double()
    last = (rays.cnt - 1).clamp_min(0)[:, None]
    bg = torch.gather(T, 1, last)[:, 0] * valid + (1 - valid)
    E_bg = torch.gather(E_T, 1, last)[:, 0] * valid
    out = {"pred": ray_sum(w[:, :, None] * C, E_w[:, :, None] * C.abs(), 1), "weights_sum": ray_sum(w, E_w, 0), "bg": (bg, E_bg),
           "min_om": float(OM[k].min()) if bool(k.any()) else 1.0, "kink": op["kink"]}
    if stage:                      # exact fp32 opacities: pred and bg under the bars the composite kernels are held to
        st = c64.RayStage(rays, alpha, om)
        q_pred, q_bg = st.radiance(rgb), st.transmittance()[1]
        out["pred"] = (q_pred.val, c64.error_bar(q_pred, c64.R_PRED))
        out["bg"] = (q_bg.val, c64.error_bar(q_bg, c64.R_T))
    if g_pred is None and g_ws is None and g_bg is None:
        return out
    z3, z1 = torch.zeros(R, 3, dtype=torch.float64), torch.zeros(R, 1, dtype=torch.float64)
    gp = z3 if g_pred is None else _d(g_pred)
    gs = z1 if g_ws is None else _d(g_ws).view(-1, 1)
    gbg = z1 if g_bg is None else _d(g_bg).view(-1, 1)
    Cq = torch.stack([C[..., 0], C[..., 1], C[..., 1] if compat else C[..., 2]], -1)
    tw = gp[:, None, :] * Cq
    gw = (tw.sum(2) + gs) * kd
    gw_mag = (tw.abs().sum(2) + gs.abs()) * kd
    E_gw = 4 * U * gw_mag
    g_rgb = gp[:, None, :] * w[:, :, None]
    E_rgb = (gp.abs()[:, None, :] * E_w[:, :, None] + U * g_rgb.abs() + TINY) * kd[:, :, None]
    v = gw * w
    E_v = (E_gw * w.abs() + gw.abs() * (E_A * T + A.abs() * E_T) + 2 * U * v.abs() + 2 * TINY) * kd

    def suffix_next(X):                                             # sum_{j > i} X_j
        s = torch.flip(torch.cumsum(torch.flip(X, [1]), 1), [1])
        return torch.cat([s[:, 1:], torch.zeros(R, 1, dtype=torch.float64)], 1)
    S, S_abs, n_behind = suffix_next(v), suffix_next(v.abs()), suffix_next(kd)
    E_S = suffix_next(E_v) + n_behind * U * S_abs + n_behind * TINY
    gb = gbg * bg[:, None]
    E_gb = gbg.abs() * E_bg[:, None] + U * gb.abs() + TINY
    floor_on = OM < C_1EM6
    omc = torch.where(floor_on, torch.full_like(OM, C_1EM6), OM)
    E_omc = torch.where(floor_on, torch.zeros_like(OM), E_OM)
    z = torch.zeros_like(v)
    g_om = torch.where(inner, (S + gb) / omc, z)
    E_gom = torch.where(inner, (E_S + E_gb) / omc + (S.abs() + gb.abs()) * E_omc / omc ** 2 + 3 * U * (S.abs() + gb.abs()) / omc + TINY / omc, z)
    g_alpha = (gw * T - g_om) * kd
    E_ga = (E_gw * T + gw.abs() * E_T + U * (gw * T).abs() + E_gom + U * g_alpha.abs()) * SLACK * kd
    ga, bar_ga = rays.scatter(g_alpha, N), rays.scatter(E_ga, N)
    out["g_alpha"] = (ga, bar_ga)
    out["g_sdf"] = (ga * op["D_sdf"], c64.compose_bar(ga, bar_ga, op["D_sdf"], op["E_sdf"], op["uf"]))
    out["g_gradients"] = (ga[:, None] * op["D_grad"],
                          c64.compose_bar(ga[:, None], bar_ga[:, None], op["D_grad"], op["E_grad"], op["uf"][:, None]))
    t = ga * op["D_inv"]
    n_terms = int((t != 0).sum())
    out["g_inv_s"] = (t.sum().reshape(1), (c64.compose_bar(ga, bar_ga, op["D_inv"], op["E_inv"], op["uf"]).sum()
                                           + n_terms * U * SLACK * t.abs().sum()).reshape(1))
    out["g_rgb"] = (rays.scatter(g_rgb, N), rays.scatter(E_rgb * SLACK, N))
    return out


def render_torch(rays, sdf, dirs, gradients, dt, rgb, inv_s, ratio=RATIO, dtype=torch.float64, drop_ws=False, ws_from_bg=False):
    """VolumeRenderingNeus.compute_weights + integrate (volume_rendering_modules.py:129-190) restated in torch operators on the
    padded [R, nmax] view of the container, in `dtype`, differentiable by autograd -> (pred [R, 3], weights_sum [R], bg [R]).
    cumprod_alpha2transmittance is the exclusive product along the ray whose last factor never enters.
    drop_ws: the weight sum cut from the graph (what a backward that forgets g_weights_sum gives); ws_from_bg: the weight sum
    replaced by 1 - bg."""
    k, idx = rays.mask, rays.idx
    c32 = lambda v: torch.tensor(v, dtype=torch.float32).to(dtype)

    def pad(x):
        g = x[idx]
        return g * (k if g.dim() == 2 else k[:, :, None]).to(x.dtype)
    r = c32(ratio)
    tc = (dirs.to(dtype) * gradients.to(dtype)).sum(-1)
    ic = -(torch.relu(-tc * 0.5 + 0.5) * (1.0 - r) + torch.relu(-tc) * r)
    half = ic * dt.to(dtype).reshape(-1) * 0.5
    s = sdf.to(dtype).reshape(-1)
    inv = inv_s.to(dtype).reshape(-1)[0]
    pc, nc = torch.sigmoid((s - half) * inv), torch.sigmoid((s + half) * inv)
    alpha = ((pc - nc + c32(1e-5)) / (pc + c32(1e-5))).clip(0.0, 1.0)
    om = 1 - alpha + c32(1e-7)
    A, OM, C = pad(alpha), pad(om), pad(rgb.to(dtype))
    inner = k & ~rays.is_last
    fac = torch.where(inner, OM, torch.ones_like(OM))
    T = torch.cat([torch.ones(rays.R, 1, dtype=dtype), torch.cumprod(fac, 1)[:, :-1]], 1) * k.to(dtype)
    w = A * T
    pred = (w[:, :, None] * C).sum(1)
    ws = w.sum(1)
    valid = rays.valid.to(dtype)
    bg = torch.gather(T, 1, (rays.cnt - 1).clamp_min(0)[:, None])[:, 0] * valid + (1 - valid)
    if ws_from_bg:
        ws = 1 - bg
    return pred, ws.detach() if drop_ws else ws, bg


# --------------------------------------------------------------------------------------------------------------- the loss
def mask_loss_cases(R, hit_mode="mixed", seed=0):
    """-> pred, gt [R, 3], hit [R] uint8 or None (hit_mode: None, "zero", "mixed"), ws [R], gt_mask [R] in {0, 1}: weight sums
    0, one step below / AT / one step above both clip bounds, 0.5 and 1, cycled over the rays against both mask values"""
    g = torch.Generator().manual_seed(9100 + seed)
    pred, gt = torch.rand(R, 3, generator=g), torch.rand(R, 3, generator=g)
    pred[::7, 1] = gt[::7, 1]                                      # entries with pred == gt: the sign's zero arm
    hit = None if hit_mode is None else (torch.zeros(R, dtype=torch.uint8) if hit_mode == "zero"
                                         else (torch.rand(R, generator=g) < 0.8).to(torch.uint8))
    lo, hi = torch.tensor(1e-3, dtype=torch.float32), torch.tensor(1.0 - 1e-3, dtype=torch.float32)
    special = torch.stack([torch.tensor(0.0), torch.nextafter(lo, lo * 0), lo, torch.nextafter(lo, lo + 1), torch.tensor(0.5),
                           torch.nextafter(hi, hi * 0), hi, torch.nextafter(hi, hi + 1), torch.tensor(1.0)])
    i = torch.arange(R)
    ws = special[i % 9].clone()
    gt_mask = ((i // 9) % 2).float()
    return pred, gt, hit, ws, gt_mask


def mask_loss(pred, gt, hit, ws, gt_mask, mask_weight=0.1, lo=CLIP_LO, hi=CLIP_HI, base=0.0):
    """-> dict name -> (value, bar): loss [1] (= base + colour term + mask_weight * mask term), terms [2], g_pred [R, 3], g_ws [R]"""
    p, g = _d(pred), _d(gt)
    R = p.shape[0]
    h = torch.ones(R, 1, dtype=torch.float64) if hit is None else _d(hit).reshape(-1, 1).ne(0).double()
    d = p - g
    t0 = (d.abs() * h).mean()
    bar0 = 3 * U * SLACK * t0.abs() + TINY
    g_pred = torch.sign(d) * h / (3.0 * R)
    wgt = float(mask_weight)
    w, t = _d(ws).reshape(-1), _d(gt_mask).reshape(-1)
    c = w.clamp(lo, hi)
    om = 1.0 - c
    lc, lo_ = torch.log(c), torch.log(om)
    E_lc = 2 * ULP_LOGF * U * lc.abs()
    E_lo = U + 2 * ULP_LOGF * U * lo_.abs()
    row = -(t * lc + (1 - t) * lo_)
    E_row = t.abs() * E_lc + (1 - t).abs() * E_lo + 3 * U * ((t * lc).abs() + ((1 - t) * lo_).abs()) + U * row.abs()
    t1 = row.mean()
    bar1 = E_row.mean() * SLACK + 2 * U * t1.abs() + TINY          # (the fp32 scale mask_weight / R: one rounding, + 1)
    inside = (w >= lo) & (w <= hi)
    g_ws = torch.where(inside, wgt * (c - t) / (om * c) / R, torch.zeros_like(w))
    total = base + t0 + wgt * t1
    return {"g_pred": (g_pred, 2 * U * SLACK * g_pred.abs()), "g_ws": (g_ws, 7 * U * SLACK * g_ws.abs() + TINY),
            "terms": (torch.stack([t0, t1]), torch.stack([bar0, bar1])),
            "loss": (total.reshape(1), (bar0 + abs(wgt) * bar1 + 2 * U * (abs(base) + total.abs())).reshape(1))}


def mask_loss_torch(pred, gt, hit, ws, gt_mask, mask_weight=0.1, lo=CLIP_LO, hi=CLIP_HI, use_hit=True, clip=True):
    """train_permuto_sdf.py:372,381-383 in torch operators, in the dtype of `pred` -> (loss, terms [2]).  use_hit=False / clip=False:
    the two ways of getting it wrong that the bars must see."""
    ad = (pred - gt).abs()
    if hit is not None and use_hit:
        ad = ad * hit.reshape(-1, 1).ne(0).to(pred.dtype)
    loss_rgb = ad.mean()
    c = ws.clip(lo, hi) if clip else ws.clip(1e-12, 1.0 - 1e-7)       # (unclipped: kept finite only)
    loss_mask = torch.nn.functional.binary_cross_entropy(c.reshape(-1), gt_mask.to(pred.dtype).reshape(-1))
    return loss_rgb + loss_mask * mask_weight, torch.stack([loss_rgb.detach(), loss_mask.detach()])
