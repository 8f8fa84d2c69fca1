"""FLOAT64 EVALUATOR of the NeRF foreground render, its loss tail and the head join (csrc/nerf_render.hip).  A helper of
tests/test_nerf_host.py, tests/test_gpu_nerf_render.py: no test lives here.

Plain torch float64 on the CPU, NO AUTOGRAD: values and gradients are written out.  Inputs are fp32 tensors taken exactly.

THE RENDER (render).  For a ray of n samples, with dens = softplus(raw) (linear above 20), e = exp(-dens dt):
    a_i = 1 - e_i,   om_i = (1 - a_i) + 1e-7,   T_i = prod_{j < i} om_j,   w_i = a_i T_i
    pred = sum w_i c_i,   weights_sum = sum w_i,   bg = T_{n-1}       (the LAST sample's factor never enters: cumprod_fwd_kernel)
and for upstream gradients g_pred [3], g_ws, g_bg of the ray (each may be absent = 0):
    g_w_i = <g_pred, c_i> + g_ws         (reference_compat: the third colour channel is read as the second, VolumeRenderingGPU.cuh:1247)
    v_i = g_w_i a_i T_i,   g_om_i = (sum_{j > i} v_j + g_bg bg) / max(om_i, 1e-6) for i < n - 1, 0 for the last sample
    g_alpha_i = g_w_i T_i - g_om_i,   g_raw_i = g_alpha_i e_i dt_i sigmoid(raw_i) (1 above 20),   g_rgb_i = g_pred w_i
Empty rays and rays whose range passes the pool: pred 0, weights_sum 0, bg 1, their samples untouched.  With the floor 1e-6
inactive and reference_compat off this is the derivative of the forward (tests/test_nerf_host.py holds it against torch autograd).

BARS.  u = 2^-24.  A first-order running error analysis in the manner of oracle/composite_float64.py, whose opacity stage
(`nerf_opacity`: a, om, D = e dt sigmoid(raw) with their bounds E_a, E_om, E_D from the measured accuracy of expf / log1pf) is taken
as it is.  On top of it, per ray:
    T_i      relT_i = sum_{j < i} E_om_j / om_j + (i + 1) u  (scan_mults: the multiplication nodes behind T_i);  E_T = T expm1(relT) + (i + 1) 2^-126
    w_i      E_w = E_a T + a E_T + u w + 2^-126
    sums     of m terms t_i with bars E_i, in ANY order:  sum E_i + (m + r) u sum |t_i| + m 2^-126   (r: roundings forming a term)
    g_w      four terms, three additions: 4 u (sum_c |g_c c_c| + |g_ws|)
    v_i      E_v = E_gw a T + |g_w| (E_a T + a E_T) + 2 u |v| + 2 2^-126
    g_om_i   S = sum_{j > i} v_j with its sum bar E_S;  gb = g_bg bg, E_gb = |g_bg| E_bg + u |gb| + 2^-126;
             E = (E_S + E_gb) / omc + (|S| + |gb|) E_om / omc^2 [floor inactive] + 3 u (|S| + |gb|) / omc + 2^-126 / omc
    g_alpha  E = E_gw T + |g_w| E_T + u |g_w T| + E_gom + u |g_alpha|;      g_raw: compose_bar(g_alpha, E, D, E_D) of the oracle
    g_rgb    |g_c| E_w + u |g_c w| + 2^-126
everything times SLACK = 1 / (1 - 2048 u) for the dropped second-order terms.  The analysis is valid while E_om / om stays small:
the float64 family (`family("float64")`) keeps every om above 1e-4 (checked on the CPU), so the floor max(om, 1e-6) is inactive
and E_om / om <= 1e-3.  With `alpha=, om=` given -- the fp32 values an opacity kernel returned -- the same formulas run as a
pure RAY STAGE on exact inputs (E_a = E_om = 0, the floor evaluated as the kernels evaluate it): valid at any saturation, which is
how the saturated family is held against the unfused operator chain (two fp32 evaluations of one formula lie within the sum of
their bars of each other).

THE LOSS (loss).  terms[0] = mean over 3 R of (gt - pred)^2 hit;  terms[1] = mean over R of -(t log c + (1 - t) log(1 - c)),
c = clip(ws, lo, hi) with the fp32 bounds the kernel holds;  g_pred = -2 (gt - pred) hit / (3 R);  g_ws = weight (c - t) /
((1 - c) c) / R where lo <= ws <= hi (torch.clamp passes the gradient AT a bound), else 0.  Rows are fp32, the sums double:
    a squared-error row 3 roundings, a g_pred entry 3 (+ 1 for the coefficient);  log: ULP_LOGF ulps (1 documented for the device
    logf, + 1 as the oracle does for what is not measured here) on an argument that is exact (c) or carries u (1 - c);
    a g_ws entry 7 roundings on a quotient whose factors are bounded away from 0 by the clip.

THE HEAD JOIN (gelu_bars).  gelu(z) = z cdf, cdf = fma(0.5, erf(z / sqrt 2), 0.5), erf within 1 ulp (gelu_device.h: erf_fast) of
an argument within 2 u: |d erf| <= 2 u + 2 u max x erf'(x) <= 3 u, cdf within 2.5 u, the value within 3.5 u |z| -> 4 u |z|.
gelu'(z) = fma(z, pdf, cdf), pdf = 0.39894 __expf(-z^2 / 2): the fast exponential's measured ulps of the oracle
(ULP_FAST_EXPF_NEAR / _FAR by argument range) and the argument's 2 roundings: |z| pdf ((2 ulps + 2) u + z^2 u) + 2.5 u + u |gelu'|.
The reference values are torch's gelu / gelu_backward in float64."""
import math

import torch

from oracle import composite_float64 as c64
from oracle.composite_float64 import SLACK, TINY, U, _f32

C_1EM6, C_1EM7 = c64.C_1EM6, c64.C_1EM7
CLIP_LO, CLIP_HI = _f32(1e-3), _f32(1.0 - 1e-3)
ULP_LOGF = 2
RAY_COUNTS = (0, 1, 63, 64, 65, 128, 129, 256)


# ------------------------------------------------------------------------------------------------------------ containers
def container(name="borders"):
    """borders : rays of 0, 1, 63, 64, 65, 128, 129 and 256 samples, a second empty ray, then rays of 70 and 40 samples whose
                 range passes the pool (it ends 17 samples into the first of them): both kinds of invalid ray
       equalK  : 6 rays of K samples in the equal-count mode of RayIndex (start_end is not read)"""
    if name.startswith("equal"):
        fixed = int(name[5:])
        counts = torch.full((6,), fixed, dtype=torch.int64)
        equal = True
    else:
        counts = torch.tensor(list(RAY_COUNTS) + [0, 70, 40])
        equal, fixed = False, 0
    ends = torch.cumsum(counts, 0)
    starts = ends - counts
    N = int(ends[-1]) if equal else int(starts[-2]) + 17
    return dict(name=name, counts=counts, start_end=torch.stack([starts, ends], 1).to(torch.int32), N=N, total=int(ends[-1]), equal=equal,
                fixed=fixed, R=len(counts), max_per_ray=int(counts.max()) if equal else max(RAY_COUNTS))


def rays_of(c):
    return c64.Rays(c["start_end"], c["N"], equal=c["equal"], fixed=c["fixed"], nr_rays=c["R"])


def family(c, kind, seed=0):
    """-> raw [N], dt [N, 1], rgb [N, 3]
    float64   : the trained regime, raw ~ 3 N(0, 1) - 2 clipped to [-12, 4], dt in [1e-3, 0.05]: dens dt <= 0.21, om >= 0.8
    saturated : raw from -30 to +30 (the softplus is linear above 20), dt up to 4 (alpha == 1.0f needs dens dt above 16.6) with
                1e10 on every ray's last sample: alpha = 1 exactly on a fifth of the samples, om = 1e-7 below the backward's floor"""
    g = torch.Generator().manual_seed(7000 + seed)
    N = c["N"]
    rgb = torch.rand(N, 3, generator=g)
    if kind == "float64":
        raw = (torch.randn(N, generator=g) * 3.0 - 2.0).clamp(-12.0, 4.0)
        dt = torch.rand(N, 1, generator=g) * 0.049 + 1e-3
        return raw, dt, rgb
    if kind != "saturated":
        raise ValueError(kind)
    raw = torch.rand(N, generator=g) * 60.0 - 30.0
    raw[::3] = torch.randn(len(raw[::3]), generator=g) * 3
    dt = torch.rand(N, 1, generator=g) * 4.0 + 1e-3
    cnt = c["counts"]
    last = (torch.cumsum(cnt, 0) - 1)[cnt > 0]
    dt[last[last < N]] = 1e10
    return raw, dt, rgb


def upstream(c, seed=0):
    """-> g_pred [R, 3], g_ws [R, 1], g_bg [R, 1]"""
    g = torch.Generator().manual_seed(8000 + seed)
    R = c["R"]
    return torch.randn(R, 3, generator=g), torch.randn(R, 1, generator=g), torch.randn(R, 1, generator=g)


SUBSETS = [(p, w, b) for p in (True, False) for w in (True, False) for b in (True, False) if p or w or b]


# ------------------------------------------------------------------------------------------------------------- the render
def _d(t):
    return t.detach().cpu().double()


def render(rays, raw, dt, rgb, g_pred=None, g_ws=None, g_bg=None, compat=False, alpha=None, om=None):
    """-> dict name -> (float64 value, bar): pred [R, 3], weights_sum [R], bg [R], and with an upstream gradient g_raw [N],
    g_rgb [N, 3] (0 with bar 0 on slots no processed ray owns); `min_om`: the smallest 1 - alpha + 1e-7 of a processed sample.
    alpha, om (fp32, from an opacity kernel): run as a ray stage on these exact inputs (see the module docstring)."""
    N = raw.numel()
    op = c64.nerf_opacity(raw, dt)
    k, R, nmax = rays.mask, rays.R, rays.nmax
    kd = k.double()
    if alpha is None:
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
           "min_om": float(OM[k].min()) if bool(k.any()) else 1.0}
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
    num = S + gb
    g_om = torch.where(inner, num / omc, z)
    E_gom = torch.where(inner, (E_S + E_gb) / omc + (S.abs() + gb.abs()) * E_omc / omc ** 2 + 3 * U * (S.abs() + gb.abs()) / omc + TINY / omc, z)
    g_alpha = (gw * T - g_om) * kd
    E_ga = (E_gw * T + gw.abs() * E_T + U * (gw * T).abs() + E_gom + U * g_alpha.abs()) * SLACK * kd
    ga, bar_ga = rays.scatter(g_alpha, N), rays.scatter(E_ga, N)
    D, E_D = op["D"], op["E_D"]            # e dt sigmoid(raw) from raw itself: its running bound holds at any saturation
    out["g_alpha"] = (ga, bar_ga)
    out["D"] = (D, E_D)
    out["g_raw"] = (ga * D, c64.compose_bar(ga, bar_ga, D, E_D, op["uf"]))
    out["g_rgb"] = (rays.scatter(g_rgb, N), rays.scatter(E_rgb * SLACK, N))
    return out


def render_torch(rays, raw, dt, rgb, dtype=torch.float64, drop_ws=False, drop_bg=False):
    """VolumeRenderingNerf.compute_weights + integrate (volume_rendering_modules.py:72-90) behind NerfHash's softplus, restated in
    torch operators on the padded [R, nmax] view of the container, in `dtype`, differentiable by autograd -> (pred [R, 3],
    weights_sum [R], bg [R]).  cumprod_alpha2transmittance is the exclusive product along the ray whose last factor never enters.
    drop_ws / drop_bg: the weight sum / background transmittance cut from the graph (what a backward that forgets the term gives)."""
    k = rays.mask
    idx = rays.idx

    def pad(x):
        g = x[idx]
        return g * (k if g.dim() == 2 else k[:, :, None]).to(x.dtype)
    dens = torch.nn.functional.softplus(raw.to(dtype))
    alpha = 1.0 - torch.exp(-dens * dt.to(dtype).reshape(-1))
    om = 1 - alpha + torch.tensor(1e-7, dtype=torch.float32).to(dtype)
    A, OM, C = pad(alpha), pad(om), pad(rgb.to(dtype))
    inner = k & ~rays.is_last
    fac = torch.where(inner, OM, torch.ones_like(OM))
    T = torch.cat([torch.ones(rays.R, 1, dtype=dtype), torch.cumprod(fac, 1)[:, :-1]], 1) * k.to(dtype)
    w = A * T
    pred = (w[:, :, None] * C).sum(1)
    ws = w.sum(1)
    valid = rays.valid.to(dtype)
    bg = torch.gather(T, 1, (rays.cnt - 1).clamp_min(0)[:, None])[:, 0] * valid + (1 - valid)
    return pred, ws.detach() if drop_ws else ws, bg.detach() if drop_bg else bg


# --------------------------------------------------------------------------------------------------------------- the loss
def loss_cases(R, seed=0):
    """-> pred, gt [R, 3], hit [R] uint8, ws [R], gt_mask [R]: weight sums below, AT and above both clip bounds and away from them
    (an empty ray gives exactly 0, a saturated one 1 and beyond by rounding), masks of 0, 1 and values in between"""
    g = torch.Generator().manual_seed(9000 + seed)
    pred, gt = torch.rand(R, 3, generator=g), torch.rand(R, 3, generator=g)
    hit = (torch.rand(R, generator=g) < 0.8).to(torch.uint8)
    ws = torch.rand(R, generator=g)
    lo, hi = torch.tensor(1e-3, dtype=torch.float32), torch.tensor(1.0 - 1e-3, dtype=torch.float32)
    special = torch.stack([lo, hi, torch.nextafter(lo, lo * 0), torch.nextafter(lo, lo + 1), torch.nextafter(hi, hi * 0), torch.nextafter(hi, hi + 1),
                           torch.tensor(0.0), torch.tensor(1.0), torch.tensor(1.0 + 3e-7), torch.tensor(5e-4), torch.tensor(0.5)])
    n = min(R, len(special))
    ws[torch.randperm(R, generator=g)[:n]] = special[torch.randperm(len(special), generator=g)[:n]]
    gt_mask = (torch.rand(R, generator=g) < 0.5).float()
    gt_mask[::5] = torch.rand(len(gt_mask[::5]), generator=g)
    return pred, gt, hit, ws, gt_mask


def loss(pred, gt, hit=None, ws=None, gt_mask=None, mask_weight=0.1, lo=CLIP_LO, hi=CLIP_HI, base=0.0):
    """-> dict name -> (value, bar): terms [2], loss (= base + terms[0] + mask_weight terms[1]), g_pred [R, 3], g_ws [R]"""
    p, g = _d(pred), _d(gt)
    R = p.shape[0]
    h = torch.ones(R, 1, dtype=torch.float64) if hit is None else _d(hit).reshape(-1, 1).ne(0).double()
    d = g - p
    sq = d * d * h
    t0 = sq.mean()
    bar0 = 4 * U * SLACK * t0.abs() + TINY
    g_pred = -2.0 * d * h / (3.0 * R)
    out = {"g_pred": (g_pred, 4 * U * SLACK * g_pred.abs() + TINY)}
    wgt = _f32(mask_weight)
    if ws is None:
        t1, bar1 = torch.zeros((), dtype=torch.float64), torch.zeros((), dtype=torch.float64)
    else:
        w, t = _d(ws).reshape(-1), _d(gt_mask).reshape(-1)
        c = w.clamp(lo, hi)
        om = 1.0 - c
        lc, lo_ = torch.log(c), torch.log(om)
        E_lc = 2 * ULP_LOGF * U * lc.abs()
        E_lo = U + 2 * ULP_LOGF * U * lo_.abs()
        row = -(t * lc + (1 - t) * lo_)
        E_row = t.abs() * E_lc + (1 - t).abs() * E_lo + 3 * U * ((t * lc).abs() + ((1 - t) * lo_).abs()) + U * row.abs()
        t1 = row.mean()
        bar1 = E_row.mean() * SLACK + TINY
        inside = (w >= lo) & (w <= hi)
        g_ws = torch.where(inside, wgt * (c - t) / (om * c) / R, torch.zeros_like(w))
        out["g_ws"] = (g_ws, 7 * U * SLACK * g_ws.abs() + TINY)
    out["terms"] = (torch.stack([t0, t1]), torch.stack([bar0, bar1]) + U * torch.stack([t0, t1]).abs())     # (stored as fp32)
    total = base + t0 + wgt * t1
    out["loss"] = (total, bar0 + abs(wgt) * bar1 + 3 * U * (abs(base) + t0.abs() + abs(wgt) * t1.abs()) + U * total.abs())
    return out


def loss_torch(pred, gt, hit, ws, gt_mask, mask_weight=0.1, lo=CLIP_LO, hi=CLIP_HI, use_hit=True, clip=True):
    """train_nerf.py:203-207 in torch operators, in the dtype of `pred` -> (loss, terms [2]).  use_hit=False / clip=False: the two
    ways of getting it wrong that the bars must see."""
    sq = (gt - pred) ** 2
    if hit is not None and use_hit:
        sq = sq * hit.reshape(-1, 1).ne(0).to(pred.dtype) * 1.0
    loss_rgb = sq.mean()
    if ws is None:
        return loss_rgb, torch.stack([loss_rgb.detach(), loss_rgb.new_zeros(())])
    c = ws.clip(lo, hi) if clip else ws.clip(1e-12, 1.0 - 1e-7)       # (unclipped: kept finite only)
    loss_mask = torch.nn.functional.binary_cross_entropy(c, gt_mask.to(pred.dtype))
    return loss_rgb + loss_mask * mask_weight, torch.stack([loss_rgb.detach(), loss_mask.detach()])


# ---------------------------------------------------------------------------------------------------------- the head join
def gelu_bars(z):
    """z fp32 -> (gelu, bar), (gelu', bar) in float64: torch's gelu / gelu_backward, and the bars of the module docstring"""
    x = _d(z)
    val = torch.nn.functional.gelu(x)
    der = torch.ops.aten.gelu_backward(torch.ones_like(x), x)
    pdf = torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    ulp = torch.where(0.5 * x * x <= 20.0, torch.full_like(x, float(c64.ULP_FAST_EXPF_NEAR)), torch.full_like(x, float(c64.ULP_FAST_EXPF_FAR)))
    bar_val = 4 * U * x.abs() + TINY
    bar_der = x.abs() * pdf * ((2 * ulp + 2) * U + x * x * U) + 2.5 * U + U * der.abs() + TINY
    return (val, bar_val), (der, bar_der)
