"""FLOAT64 EVALUATOR of the compositing stage.  TEST INFRASTRUCTURE ONLY (imported by ``tests/`` alone).

Plain torch float64 on the CPU, no autograd.  It restates the FORMULAS THE KERNELS AND THE REFERENCE'S BACKWARD KERNELS
IMPLEMENT (csrc/neus.hip, csrc/volume_rendering.hip, csrc/composite_fused.hip; the reference: VolumeRenderingGPU.cuh:371-417
and :1135-1206 cumprod_alpha2transmittance and its backward with ``clamp_min(alpha_cur, 1e-6)`` at :1177,1184, :425-481 and
:1208-1268 integrate_with_weights and its backward with the channel quirk at :1247, :566-760 the per-ray sums,
volume_rendering_modules.py:72-86,129-172 the two opacities), not the derivative of the forward:

  * the factor of a ray's LAST sample never enters the product, ``bg`` is the ``T`` of the last sample;
  * the transmittance backward divides by ``max(1 - alpha + 1e-7, 1e-6)``;
  * ``reference_compat`` selects (r, g, G) or (r, g, b) in the weight gradient;
  * empty rays and rays whose range passes ``max_nr_samples`` are skipped: ``pred = 0``, ``bg = 1``, their samples untouched.

Inputs are fp32 tensors taken exactly; containers are packed with arbitrary ``start_end`` (``Rays``).

WHAT COMES BACK.  Every output is a ``Q``: the float64 value and, entry by entry, what the bar needs --
  ``mag``  sum of the absolute values of the finest-grain terms (single products, no cancelling sum inside),
  ``m``    their number (bounds the additions of ANY summation order),
  ``rw``   sum over the terms of (roundings spent on the transmittance of that term) x |term|: the only rounding count that
           differs from term to term; the caller supplies the count per sample (``scan_mults`` for the kernels' Hillis-Steele
           scans, ``serial_mults`` for a serial product),
  ``uf``   the float64 magnitude of everything that multiplies an fp32 intermediate (T, scan partials, v = g_w a T, suffix sums)
           on its way to the entry: each such intermediate may lose up to 2^-126 to gradual underflow or flush-to-zero.
``error_bar(q, r)`` = ((m + r) mag + rw) u / (1 - 2048 u) + 2^-126 uf, r = the roundings on one term apart from its
transmittance, counted from the kernel expressions (the R_* constants below).

THE OPACITY STAGE is elementwise and nonlinear: its bar is a first-order RUNNING ERROR ANALYSIS.  Every intermediate x of
``section()`` (composite_device.h) is evaluated in float64 together with a bound E(x) of |fp32 x - float64 x|:
    z = x op y rounded once:   E(z) = |dz/dx| E(x) + |dz/dy| E(y) + u |z|
    tc = d . g (3 products, 2 sums):          E = 3 u sum|d_k g_k|
    relu: E unchanged where active, 0 where not -- valid because entries whose tc lies within E(tc) of a kink (tc = 0, tc = 1)
          are EXCLUDED (``kink``), so fp32 and float64 take the same arm
    expf(y):  E = e^y (expm1(E(y)) + ULP_EXPF 2u) + 2^-126;   sigmoid s = 1 / (1 + expf(-x)):
          E(s) = s ((1 - s) (expm1(E(x)) + ULP_EXPF 2u) + 2u) + 2^-126      (1 + e and the reciprocal: one rounding each)
    log1pf(y): E = ULP_LOG1PF 2u log1p(y) + E(y) / (1 + y)
    clip to [0, 1]: 1-Lipschitz, E unchanged.
The formula, not the kernel, is ill-conditioned in three places, and there the bound is ABSOLUTE (u times the operands, not
times the result): ``p = pc - nc`` (both near 1 in front of the surface, both near 0 behind it), ``1 - pc`` as pc -> 1 (the
sigmoid derivative; fp32 gives an exact 0 where float64 keeps 1e-30), and ``g_p + g_c = (den - p - 1e-5) / den^2`` (= nc /
den^2, cancelling as nc -> 0).  Entries that only these absolute terms cover are reported as "saturated" by the tests.
The backward expressions are linear in the upstream g: the analysis runs on g = 1 (``D``: d alpha / d sdf, d alpha / d tc,
the per-sample term of d alpha / d inv_s), and the composition with a ray-stage gradient that has a bar of its own is
    bar(g D) = bar(g) |D| + |g| E(D) + bar(g) E(D) + 2^-126 uf.

ULP_EXPF / ULP_LOG1PF / ULP_FAST_EXPF_*: maximum error of the device functions in ulps (1 ulp <= 2u relative).  No HIP math
accuracy table is installed with the toolchain used here, so they were MEASURED on an MI355X against float64 over the
argument ranges the kernels use (tools/probes/libm_ulp_probe.hip; LABNOTES.md has the figures): worst observed error rounded
up to the next whole ulp, plus one, because a sample is not a bound.  They are not tuned to what the kernels under test give.
"""
import collections
import math

import torch

U = 2.0 ** -24            # unit roundoff of fp32
TINY = 2.0 ** -126        # smallest normal fp32
SLACK = 1.0 / (1.0 - 2048 * U)     # (1 + u)^k - 1 <= k u / (1 - k u) for the k < 2048 roundings of any entry here

ULP_EXPF = 2              # measured worst 0.848 ulp on [1e-8, 88.7], 0.843 on [-87.3, -1e-8]  -> 1, + 1   (LABNOTES.md)
ULP_LOG1PF = 2            # measured worst 0.567 ulp on [1e-14, 5e8]                            -> 1, + 1
# __expf (volume_render_nerf only) is exp2(x log2(e)) with the product rounded: its error grows with |x|
ULP_FAST_EXPF_NEAR = 17   # measured worst 15.698 ulp on [-20, -1e-8]                           -> 16, + 1
ULP_FAST_EXPF_FAR = 65    # measured worst 63.744 ulp on [-87.3, -20]                           -> 64, + 1


def _f32(x):
    """the fp32 constant the kernels hold, as a float64 number"""
    return float(torch.tensor(x, dtype=torch.float32).double())


C_1EM4, C_1EM5, C_1EM6, C_1EM7 = _f32(1e-4), _f32(1e-5), _f32(1e-6), _f32(1e-7)

# ---- roundings per finest-grain term, APART from the transmittance of the term (that is `rw`), from the kernel expressions
R_T = 0           # T itself: everything is in rw
R_W = 1           # w = a * T
R_PRED = 2        # w = a * T;  acc += w * rgb                      (integrate_fwd_kernel / the fused forward)
R_GRGB = 2        # w = a * T;  g_rgb = g * w
R_GW = 1          # g_w = gx * cx + gy * cy + gz * cz: one product per term
R_RAY_BWD = 6     # g_c * c_c (1);  (g_w * a) * T (2);  cs / om (1);  + g_bg bg / om (1);  g_w T - g_om (1)
R_GB = 3          # the g_bg term of the same entry: g_bg * bg (1), / om (1), the two additions are already in the 6 above
# per-operator kernels on fp32 inputs of their own
R_OP_INTEGRATE = 1      # acc += w * rgb
R_OP_GRGB = 1           # g * w
R_OP_CUMPROD_BWD = 2    # cs / a;  g_bg * bg then / a  (the addition is in m)
R_OP_SUM = 0
# volume_render_nerf (render_nerf_fwd_kernel / render_nerf_bwd_kernel); the transmittance carries the opacity error (render_nerf)
R_RN_W = 1              # wi = a * Ti
R_RN_SUM = 1            # r += wi * rgb: one product per term, the m additions beside it
R_RN_GSIGMA = 8         # longest path of one term of g_sigma: gx * d (1), Tn * cx (1), fx - px (1), Tn cx - (.) (1), the product
                        # (1), gr += over three channels and the g_bg term (<= 4 additions; the g_bg term itself: -d * lastT, * gbg)
R_RN_UF = 8             # fp32 intermediates of one g_sigma entry that may leave the normals (each times |g d| or 1)


def scan_mults(i):
    """roundings on the path to T_i in the kernels.  A product is unlike a sum: every multiplication NODE of the expression tree
    that forms T_i puts its (1 + delta) on the whole result, so what counts is the number of nodes, not the depth of the tree (in
    a sum a node's delta weighs only its own partial sum, and the depth bounds the error; counting "6 scan steps per 64-sample
    chunk plus the carry" would be that bound, and the kernels -- like any fp32 product of i factors -- exceed it: measured 1.19x
    on T at 64 samples, LABNOTES.md).  wave_incl_scan_mul forms lane l's inclusive product of l + 1 inputs with l
    multiplications (a binary tree over disjoint lane ranges), the exclusive value of lane l is lane l - 1's: max(l - 1, 0);
    `carry * excl` is one more; every finished chunk costs the carry 63 + 1.  In all 64 k + max(l - 1, 0) + 1 <= i + 1 for sample
    i = 64 k + l: the count of a serial product, plus one."""
    return i + 1


def serial_mults(i):
    """T_i = T_{i-1} * om_{i-1}: i multiplications"""
    return i


Q = collections.namedtuple("Q", "val mag m rw uf")


def error_bar(q, r):
    m = q.m if torch.is_tensor(q.m) else torch.as_tensor(float(q.m), dtype=torch.float64)
    return ((m + float(r)) * q.mag + q.rw) * (U * SLACK) + TINY * q.uf


def _q1(val, rt=None, uf=None):
    """a single-term entry"""
    z = torch.zeros_like(val)
    return Q(val, val.abs(), torch.ones_like(val), z if rt is None else rt * val.abs(), z + 1 if uf is None else uf)


class Rays:
    """start_end [R, 2] integer (ignored for equal counts), the pool size `max_nr_samples`, and the padded [R, nmax] view of the
    samples of the rays the kernels process (RayIndex::valid in composite_device.h: not empty, end <= max_nr_samples)."""

    def __init__(self, start_end, max_nr_samples, equal=False, fixed=0, nr_rays=None):
        if equal:
            s = torch.arange(nr_rays, dtype=torch.int64) * int(fixed)
            e = s + int(fixed)
        else:
            se = torch.as_tensor(start_end).detach().cpu().to(torch.int64)
            s, e = se[:, 0].clone(), se[:, 1].clone()
        self.R = s.numel()
        self.start, self.end = s, e
        self.valid = ~((e > int(max_nr_samples)) | (e == s))
        self.cnt = torch.where(self.valid, e - s, torch.zeros_like(s))
        self.nmax = max(1, int(self.cnt.max())) if self.R else 1
        self.pos = torch.arange(self.nmax, dtype=torch.int64)[None, :]
        self.mask = self.pos < self.cnt[:, None]
        self.idx = torch.where(self.mask, s[:, None] + self.pos, torch.zeros_like(self.pos))
        self.is_last = self.pos == (self.cnt[:, None] - 1)

    def gather(self, x):
        """[N] / [N, 1] / [N, C] fp32 -> float64 [R, nmax] / [R, nmax, C], zero outside the rays"""
        x = x.detach().cpu().double()
        if x.dim() == 2 and x.shape[1] == 1:
            x = x[:, 0]
        g = x[self.idx]
        return g * (self.mask if g.dim() == 2 else self.mask[:, :, None])

    def scatter(self, X, N):
        """padded -> packed [N] / [N, C] float64; slots no processed ray owns stay 0"""
        out = torch.zeros((N,) + tuple(X.shape[2:]), dtype=torch.float64)
        out[self.idx[self.mask]] = X[self.mask]
        return out

    def scatter_q(self, q, N):
        return Q(*[self.scatter(t if torch.is_tensor(t) and t.dim() >= 2 else torch.as_tensor(t, dtype=torch.float64).expand(
            self.R, self.nmax).clone(), N) for t in q])

    def touched(self, N):
        t = torch.zeros(N, dtype=torch.bool)
        t[self.idx[self.mask]] = True
        return t


# ======================================================================================================= ray stage
class RayStage:
    """Scans and sums of one container given the fp32 opacity `alpha` and `om` = 1 - alpha + 1e-7 that the opacity kernels
    return ([N] or [N, 1]).  `t_mults(i)`: roundings on the path to T_i (scan_mults / serial_mults).  Results are PADDED
    [R, nmax(, 3)] per-sample and [R(, 3)] per-ray; `rays.scatter_q` packs them."""

    def __init__(self, rays, alpha, om, t_mults=scan_mults):
        self.rays = r = rays
        self.A = r.gather(alpha)
        self.OM = r.gather(om)
        fac = torch.where(r.pos < (r.cnt[:, None] - 1), self.OM, torch.ones_like(self.OM))
        incl = torch.cumprod(fac, 1)
        self.T = torch.cat([torch.ones(r.R, 1, dtype=torch.float64), incl[:, :-1]], 1) * r.mask
        self.RT = t_mults(r.pos).double().clamp_min(0).expand(r.R, r.nmax) * r.mask
        self.last = (r.cnt - 1).clamp_min(0)[:, None]

    def _per_ray(self, X):
        return torch.gather(X, 1, self.last)[:, 0]

    def transmittance(self):
        """-> T [R, nmax], bg [R] (1 exactly for skipped rays)"""
        T = Q(self.T, self.T.abs(), torch.ones_like(self.T), self.RT * self.T.abs(), self.RT)
        v = self.rays.valid.double()
        bg = self._per_ray(self.T) * v + (1 - v)
        rt = self._per_ray(self.RT) * v
        return T, Q(bg, bg * v, v, rt * bg, rt)

    def weights(self):
        w = self.A * self.T
        return Q(w, w.abs(), torch.ones_like(w), self.RT * w.abs(), self.RT * self.A.abs() + 1)

    def radiance(self, rgb):
        """pred [R, 3] = sum_i a_i T_i rgb_i (0 exactly for skipped rays)"""
        C = self.rays.gather(rgb)
        t = (self.A * self.T)[:, :, None] * C
        cnt = self.rays.cnt.double()[:, None].expand(-1, 3)
        return Q(t.sum(1), t.abs().sum(1), cnt, (self.RT[:, :, None] * t.abs()).sum(1),
                 ((self.RT * self.A.abs())[:, :, None] * C.abs()).sum(1) + 2 * cnt)

    def backward(self, rgb, g_pred, g_bg=None, compat=True):
        """-> dict of padded Q: g_rgb [R, nmax, 3], g_w, g_om, g_alpha [R, nmax].
        g_w = <g_pred, (r, g, G or b)>;  v = g_w a T;  cs_i = sum_{j >= i} v_j;
        g_om_i = (cs_{i+1} + g_bg bg) / max(om_i, 1e-6) for all but the ray's last sample (0 there);  g_alpha = g_w T - g_om"""
        r = self.rays
        C = r.gather(rgb)
        gp = g_pred.detach().cpu().double()
        Cq = torch.stack([C[..., 0], C[..., 1], C[..., 1] if compat else C[..., 2]], -1)
        tw = gp[:, None, :] * Cq                                    # the three terms of g_w
        gw, gw_mag = tw.sum(2), tw.abs().sum(2)
        A, T, RT = self.A, self.T, self.RT
        w = A * T
        g_rgb = gp[:, None, :] * w[:, :, None]
        q_rgb = Q(g_rgb, g_rgb.abs(), torch.ones_like(g_rgb), RT[:, :, None] * g_rgb.abs(),
                  (RT * A.abs())[:, :, None] * gp.abs()[:, None, :] + 2)
        q_gw = Q(gw, gw_mag, torch.full_like(gw, 3.0), torch.zeros_like(gw), torch.full_like(gw, 3.0))

        def suffix_next(X):                                         # sum_{j > i} X_j
            s = torch.flip(torch.cumsum(torch.flip(X, [1]), 1), [1])
            return torch.cat([s[:, 1:], torch.zeros(r.R, 1, dtype=torch.float64)], 1)
        v, v_mag = gw * w, gw_mag * w.abs()
        omc = self.OM.clamp_min(C_1EM6)
        omc = torch.where(r.mask, omc, torch.ones_like(omc))
        inner = r.mask & ~r.is_last
        bgT, bgRT = self._per_ray(T)[:, None], self._per_ray(RT)[:, None]
        gb = (torch.zeros(r.R, 1, dtype=torch.float64) if g_bg is None else g_bg.detach().cpu().double().view(-1, 1)) * bgT
        nterm = suffix_next(r.mask.double())                        # samples behind i
        z = torch.zeros_like(v)
        g_om = torch.where(inner, (suffix_next(v) + gb) / omc, z)
        om_mag = torch.where(inner, (suffix_next(v_mag) + gb.abs()) / omc, z)
        om_rw = torch.where(inner, (suffix_next(RT * v_mag) + bgRT * gb.abs()) / omc, z)
        om_m = torch.where(inner, 3 * nterm + 1, z)
        # underflow: T_j (RT_j scan partials) times |g_w a| / om;  (g_w a), v_j, the suffix partial: 3 per sample;  g_bg bg; the quotient
        gbg_abs = 0.0 if g_bg is None else g_bg.detach().cpu().double().view(-1, 1).abs()
        om_uf = torch.where(inner, (suffix_next(RT * gw_mag * A.abs() + 3 * r.mask) + bgRT * gbg_abs + 1) / omc + 1, z)
        q_om = Q(g_om, om_mag, om_m, om_rw, om_uf)
        a_mag = gw_mag * T.abs()
        q_ga = Q(gw * T - g_om, a_mag + om_mag, 3 * r.mask.double() + om_m, RT * a_mag + om_rw,
                 (RT * gw_mag + 2) * r.mask + om_uf)
        return {"g_rgb": q_rgb, "g_w": q_gw, "g_om": q_om, "g_alpha": q_ga}


# ---- the plain per-ray operators on fp32 inputs of their own
def op_integrate(rays, rgb, w):
    t = rays.gather(w)[:, :, None] * rays.gather(rgb)
    cnt = rays.cnt.double()[:, None].expand(-1, 3)
    return Q(t.sum(1), t.abs().sum(1), cnt, torch.zeros(rays.R, 3, dtype=torch.float64), cnt.clone())


def op_integrate_backward(rays, g_pred, rgb, w, compat):
    C, W, gp = rays.gather(rgb), rays.gather(w), g_pred.detach().cpu().double()
    Cq = torch.stack([C[..., 0], C[..., 1], C[..., 1] if compat else C[..., 2]], -1)
    tw = gp[:, None, :] * Cq
    g_rgb = gp[:, None, :] * W[:, :, None]
    return _q1(g_rgb), Q(tw.sum(2), tw.abs().sum(2), torch.full_like(W, 3.0), torch.zeros_like(W), torch.full_like(W, 3.0))


def op_cumsum(rays, vals, inverse=False, exclusive=False):
    """cumsum_over_each_ray (inclusive, from the ray's start or its end) / compute_cdf (exclusive, from the start)"""
    V = rays.gather(vals)
    if inverse:                                                     # reverse each ray in place: padded slots hold 0 and stay behind
        s = torch.flip(torch.cumsum(torch.flip(V, [1]), 1), [1])
        sa = torch.flip(torch.cumsum(torch.flip(V.abs(), [1]), 1), [1])
        m = torch.flip(torch.cumsum(torch.flip(rays.mask.double(), [1]), 1), [1])
    else:
        s, sa, m = torch.cumsum(V, 1), torch.cumsum(V.abs(), 1), torch.cumsum(rays.mask.double(), 1)
    if exclusive:
        # cumsum_kernel forms the exclusive sum as (inclusive scan) - v_i: v_i is a term twice, once with each sign, and the entry
        # errs by u (sum_{j <= i} |v_j| + |v_i|), not by u times itself (the reference's serial loop adds v_i afterwards and is exact
        # there; for a cdf in [0, 1] that is 6e-8 absolute in front of a dominant weight)
        s, sa, m = s - V, sa + V.abs(), m + 1
    k = rays.mask.double()
    return Q(s * k, sa * k, m * k, torch.zeros_like(s), m * k)


def op_sum(rays, vals):
    """sum_over_each_ray: -> per ray [R, C], per sample (padded) [R, nmax, C]"""
    V = rays.gather(vals)
    if V.dim() == 2:
        V = V[:, :, None]
    cnt = rays.cnt.double()[:, None].expand(-1, V.shape[2])
    per_ray = Q(V.sum(1), V.abs().sum(1), cnt, torch.zeros_like(cnt), cnt.clone())
    k = rays.mask[:, :, None].double()
    per_sample = Q(*[(t[:, None, :] * k) for t in per_ray])
    return per_ray, per_sample


def op_cumprod_backward(rays, g_bg, om, bg, cs):
    """cumprod_bwd_kernel on ITS inputs: g_i = cs_{i+1} / max(om_i, 1e-6) + g_bg bg / max(om_i, 1e-6), 0 on a ray's last sample"""
    OM, CS = rays.gather(om), rays.gather(cs)
    nxt = torch.cat([CS[:, 1:], torch.zeros(rays.R, 1, dtype=torch.float64)], 1)
    gb = (g_bg.detach().cpu().double().view(-1, 1) * bg.detach().cpu().double().view(-1, 1))
    omc = torch.where(rays.mask, OM.clamp_min(C_1EM6), torch.ones_like(OM))
    inner = (rays.mask & ~rays.is_last).double()
    val = (nxt + gb) / omc * inner
    return Q(val, (nxt.abs() + gb.abs()) / omc * inner, 2 * inner, torch.zeros_like(val), 3 * inner / omc)


# =================================================================================================== opacity stage
def _sigmoid(x, Ex, ulp):
    s, oms = torch.sigmoid(x), torch.sigmoid(-x)
    return s, oms, s * (oms * (torch.expm1(Ex) + 2 * ulp * U) + 2 * U) + TINY


def neus_opacity(sdf, dirs, gradients, dt, inv_s, ratio, ulp_expf=ULP_EXPF):
    """section() + clip + 1 - alpha + 1e-7 (composite_device.h, neus_alpha_fwd_kernel) and the backward expressions for g = 1
    (neus_alpha_bwd_kernel), each value with its running error bound.  -> dict of float64 [N] tensors:
      alpha, E_alpha, om, E_om, q, kink (bool: excluded, see the module docstring), and the derivatives with their bounds
      D_sdf, E_sdf (d alpha / d sdf), D_tc, E_tc (d alpha / d true_cos: g_gradients = g D_tc dir, E_grad [N, 3]),
      D_inv, E_inv (the per-sample term of d alpha / d inv_s), uf (what a 2^-126 loss inside the backward is multiplied by)."""
    c = lambda t: t.detach().cpu().double()
    sdf, dt = c(sdf).reshape(-1), c(dt).reshape(-1)
    d, g = c(dirs), c(gradients)
    inv_s, r = float(c(inv_s).reshape(-1)[0]), _f32(ratio)
    u = U
    tc = (d * g).sum(1)
    E_tc = 3 * u * (d * g).abs().sum(1)
    kink = (tc.abs() <= E_tc) | ((tc - 1).abs() <= E_tc)
    pre_a, pre_b = -tc * 0.5 + 0.5, -tc
    on_a, on_b = pre_a > 0, pre_b > 0
    ra, E_ra = pre_a * on_a, (0.5 * E_tc + u * pre_a.abs()) * on_a
    rb, E_rb = pre_b * on_b, E_tc * on_b
    ta, tb = ra * (1 - r), rb * r
    E_ta, E_tb = E_ra * (1 - r) + 2 * u * ta.abs(), E_rb * r + u * tb.abs()
    ic = -(ta + tb)
    E_ic = E_ta + E_tb + u * ic.abs()
    half = ic * dt * 0.5
    E_half = E_ic * dt.abs() * 0.5 + u * half.abs() + TINY
    en, ep = sdf + half, sdf - half
    E_en, E_ep = E_half + u * en.abs(), E_half + u * ep.abs()
    xn, xp = en * inv_s, ep * inv_s
    E_xn, E_xp = E_en * inv_s + u * xn.abs(), E_ep * inv_s + u * xp.abs()
    pc, ompc, E_pc = _sigmoid(xp, E_xp, ulp_expf)
    nc, omnc, E_nc = _sigmoid(xn, E_xn, ulp_expf)
    p = pc - nc
    E_p = E_pc + E_nc + u * p.abs()
    num, den = p + C_1EM5, pc + C_1EM5
    E_num, E_den = E_p + u * num.abs(), E_pc + u * den
    q = num / den
    E_q = E_num / den + q.abs() * E_den / den + u * q.abs()
    alpha = q.clamp(0.0, 1.0)
    om1 = 1 - alpha
    E_om1 = E_q + u * om1.abs()
    om = om1 + C_1EM7
    E_om = E_om1 + u * om
    # ---- backward for g = 1 (the clip passes the gradient on the closed interval; q is in (0, 1] for finite inputs, dt >= 0)
    gq = ((q >= 0) & (q <= 1)).double()
    g_p = gq / den
    E_gp = gq * (E_den / den ** 2 + u / den)
    den2 = den * den
    E_den2 = 2 * den * E_den + u * den2
    g_c = -gq * num / den2
    E_gc = gq * (E_num / den2 + g_c.abs() * E_den2 / den2 + 2 * u * g_c.abs())
    sm = g_p + g_c
    E_sm = E_gp + E_gc + u * sm.abs()
    dpc, dnc = pc * ompc, nc * omnc
    E_dpc = E_pc * ompc + pc * (E_pc + u * ompc) + u * dpc
    E_dnc = E_nc * omnc + nc * (E_nc + u * omnc) + u * dnc
    g_up, g_un = sm * dpc, -g_p * dnc
    E_up = E_sm * dpc + sm.abs() * E_dpc + u * g_up.abs()
    E_un = E_gp * dnc + g_p.abs() * E_dnc + u * g_un.abs()
    g_ep, g_en = g_up * inv_s, g_un * inv_s
    E_gep, E_gen = E_up * inv_s + u * g_ep.abs(), E_un * inv_s + u * g_en.abs()
    D_sdf = g_ep + g_en
    E_sdf = E_gep + E_gen + u * D_sdf.abs()
    t1, t2 = g_up * ep, g_un * en
    D_inv = t1 + t2
    E_inv = (E_up * ep.abs() + g_up.abs() * E_ep + u * t1.abs()) + (E_un * en.abs() + g_un.abs() * E_en + u * t2.abs()) \
        + u * D_inv.abs()
    diff = g_en - g_ep
    E_diff = E_gen + E_gep + u * diff.abs()
    g_ic = diff * (dt * 0.5)
    E_gic = E_diff * dt.abs() * 0.5 + u * g_ic.abs()
    coef = on_a * (0.5 * (1 - r)) + on_b * r
    D_tc = g_ic * coef
    E_Dtc = E_gic * coef + g_ic.abs() * 2 * u * coef + u * D_tc.abs()
    E_grad = E_Dtc[:, None] * d.abs() + u * (D_tc[:, None] * d).abs()
    uf = 8.0 * max(inv_s, 1.0) * torch.maximum(torch.ones_like(ep), torch.maximum(ep.abs(), en.abs()))
    return dict(alpha=alpha, E_alpha=E_q, om=om, E_om=E_om, q=q, kink=kink, tc=tc, D_sdf=D_sdf, E_sdf=E_sdf, D_tc=D_tc, E_tc=E_Dtc,
                D_grad=D_tc[:, None] * d, E_grad=E_grad, D_inv=D_inv, E_inv=E_inv, uf=uf, dirs=d)


def nerf_opacity(raw, dt, ulp_expf=ULP_EXPF, ulp_log1pf=ULP_LOG1PF):
    """softplus (linear above 20: softplus20 in neus.hip) -> alpha = 1 - exp(-dens dt) -> 1 - alpha + 1e-7, and for g = 1 the
    backward D = d alpha / d raw = e dt sigmoid(raw) (1 above 20) of nerf_alpha_kernel, with running error bounds.
    dt = 1e10 (the last background sample) gives alpha = 1, D = 0 unless dens dt stays below ~100."""
    c = lambda t: t.detach().cpu().double().reshape(-1)
    x, d = c(raw), c(dt)
    u = U
    lin = x > 20.0
    ex = torch.exp(x.clamp_max(20.0))
    dens = torch.where(lin, x, torch.log1p(ex))
    E_dens = torch.where(lin, torch.zeros_like(x), 2 * ulp_log1pf * u * dens + ex / (1 + ex) * 2 * ulp_expf * u + TINY)
    y = -dens * d
    E_y = E_dens * d.abs() + u * y.abs()
    e = torch.exp(y)
    E_e = e * (torch.expm1(E_y.clamp_max(700.0)) + 2 * ulp_expf * u) + TINY
    a = 1 - e
    E_a = E_e + u * a.abs()
    om = (1 - a) + C_1EM7
    E_om = E_a + u * (1 - a).abs() + u * om
    sig, oms, E_sig = _sigmoid(x, torch.zeros_like(x), ulp_expf)
    sig = torch.where(lin, torch.ones_like(x), sig)
    E_sig = torch.where(lin, torch.zeros_like(x), E_sig)
    D = e * d * sig
    E_D = E_e * d.abs() * sig + e * d.abs() * E_sig + 3 * u * D.abs()
    uf = 3.0 * torch.maximum(torch.ones_like(d), d.abs())
    return dict(alpha=a, E_alpha=E_a, om=om, E_om=E_om, D=D, E_D=E_D, uf=uf)


def compose_bar(g, bar_g, D, E_D, uf):
    """bar of g D where g carries bar_g and D carries E_D (see the module docstring)"""
    return bar_g * D.abs() + g.abs() * E_D + bar_g * E_D + TINY * uf


def bites(ref, bar):
    """share of the non-zero reference entries whose bar is below 1e-3 of the entry, and the share the bar cannot tell from zero
    ("saturated": bar >= |entry|)"""
    nz = ref != 0
    n = max(1, int(nz.sum()))
    return float((bar[nz] < 1e-3 * ref[nz].abs()).sum()) / n, float((bar[nz] >= ref[nz].abs()).sum()) / n


# ============================================================================================= volume_render_nerf
def render_nerf(rays, rgb, sigma, z, dt, t_mults=scan_mults, ulp_exp=None):
    """psdf_volume_render_nerf (render_nerf_fwd_kernel; the reference: VolumeRenderingGPU.cuh:68-156): alpha_i = 1 - exp(-sigma_i
    dt_i), om_i = 1 - alpha_i (no 1e-7 here, and EVERY sample's factor enters), w_i = alpha_i T_i, and the ray STOPS at the first
    sample whose incoming T is below 1e-4: that sample and everything behind it contribute nothing, bg = the T that reached it.
    There is no kernel that returns this alpha, so the opacity error is carried into T: rel(T_i) = sum_{j<i} E(om_j) / om_j +
    r_T u.  A ray with some incoming T_i (up to its stop) within E(T_i) of 1e-4 may stop elsewhere in fp32: `ambiguous` [R]
    marks it, and the tests leave it out (cap: 1 % of the rays of a case).
    -> dict: pred [R,3], depth [R], bg [R], w (padded [R, nmax]) as (value, bar) pairs; `use` (padded bool), `ambiguous` [R];
    and what the backward needs."""
    u = U
    S, D, Z, C = rays.gather(sigma), rays.gather(dt), rays.gather(z), rays.gather(rgb)
    k = rays.mask
    y = -S * D
    e = torch.exp(y)
    if ulp_exp is None:                                             # the device __expf: by argument range
        ulp_exp = torch.where(y.abs() <= 20.0, torch.full_like(y, ULP_FAST_EXPF_NEAR), torch.full_like(y, ULP_FAST_EXPF_FAR))
    E_e = e * (torch.expm1((u * y.abs()).clamp_max(700.0)) + 2 * ulp_exp * u) + TINY
    a = 1 - e
    E_a = E_e + u * a.abs()
    om = torch.where(k, 1 - a, torch.ones_like(a))
    E_om = torch.where(k, E_a + u * om, torch.zeros_like(a))
    rel_om = E_om / om.clamp_min(1e-300)
    incl = torch.cumprod(om, 1)
    one = torch.ones(rays.R, 1, dtype=torch.float64)
    Tin = torch.cat([one, incl[:, :-1]], 1)
    RT = t_mults(rays.pos).double().clamp_min(0).expand(rays.R, rays.nmax)
    relT = torch.cat([0 * one, torch.cumsum(rel_om, 1)[:, :-1]], 1) + RT * u
    E_T = Tin * torch.expm1(relT.clamp_max(700.0)) * SLACK + RT * TINY
    dead = k & (Tin < C_1EM4)
    n_before = torch.cumsum(dead.double(), 1) - dead.double()
    stopped = n_before > 0                                          # behind the first dead sample
    use = k & ~dead & ~stopped
    first_dead = dead & ~stopped
    relevant = k & ~stopped                                         # samples whose test against 1e-4 decides the ray
    ambiguous = (relevant & ((Tin - C_1EM4).abs() <= E_T)).any(1)
    w = a * Tin * use
    bar_w = (E_a * Tin + a.abs() * E_T + R_RN_W * u * w.abs() + TINY) * use
    m = use.double().sum(1)

    def ray_sum(X):                                                 # sum_i w_i X_i, X [R, nmax, c]
        t = w[:, :, None] * X
        return t.sum(1), (bar_w[:, :, None] * X.abs()).sum(1) + ((m + R_RN_SUM) * u * SLACK)[:, None] * t.abs().sum(1) + (m * TINY)[:, None]
    pred, bar_pred = ray_sum(C)
    depth, bar_depth = ray_sum(Z[:, :, None])
    Tn = Tin * om
    E_Tn = Tn * torch.expm1((relT + rel_om + u).clamp_max(700.0)) * SLACK + (RT + 1) * TINY
    any_dead = first_dead.any(1)
    last = (rays.cnt - 1).clamp_min(0)[:, None]
    bg = torch.where(any_dead, (Tin * first_dead).sum(1), torch.gather(Tn, 1, last)[:, 0])
    bar_bg = torch.where(any_dead, (E_T * first_dead).sum(1), torch.gather(E_Tn, 1, last)[:, 0])
    v = rays.valid
    bg, bar_bg = torch.where(v, bg, torch.ones_like(bg)), bar_bg * v
    return dict(pred=(pred, bar_pred), depth=(depth[:, 0], bar_depth[:, 0]), bg=(bg, bar_bg), w=(w, bar_w), use=use, ambiguous=ambiguous & v,
                _C=C, _D=D, _Tn=Tn, _E_Tn=E_Tn, _m=m)


def render_nerf_backward(rays, fwd, g_pred, g_bg, pred_rgb, bg):
    """render_nerf_bwd_kernel (the reference's suffix trick, VolumeRenderingGPU.cuh:262-287) on the fp32 pred_rgb / bg the forward
    KERNEL returned:  g_rgb_i = g w_i;  g_sigma_i = sum_c g_c dt_i (T_{i+1} c_ic - (pred_c - p_ic)) - g_bg dt_i bg, with p_i the
    colour integrated up to and including sample i; zero from the stop on.  -> (g_rgb, bar), (g_sigma, bar), padded."""
    u = U
    c = lambda t: t.detach().cpu().double()
    G, gb, f, lastT = c(g_pred), c(g_bg).view(-1, 1), c(pred_rgb), c(bg).view(-1, 1)
    w, bar_w = fwd["w"]
    use, C, D, Tn, E_Tn, m = fwd["use"], fwd["_C"], fwd["_D"], fwd["_Tn"], fwd["_E_Tn"], fwd["_m"]
    g_rgb = G[:, None, :] * w[:, :, None]
    bar_rgb = G.abs()[:, None, :] * bar_w[:, :, None] + u * g_rgb.abs()
    t = w[:, :, None] * C
    p = torch.cumsum(t, 1)
    cnt = torch.cumsum(use.double(), 1)[:, :, None]
    bar_p = torch.cumsum(bar_w[:, :, None] * C.abs(), 1) + (cnt + R_RN_SUM) * u * SLACK * torch.cumsum(t.abs(), 1) + cnt * TINY
    gd = G[:, None, :] * D[:, :, None]
    t1, t2, t3 = gd * Tn[:, :, None] * C, gd * f[:, None, :], gd * p
    val = (t1 - t2 + t3).sum(2) - gb * D * lastT
    bar = (gd.abs() * (E_Tn[:, :, None] * C.abs() + bar_p)).sum(2) + R_RN_GSIGMA * u * SLACK * (t1.abs() + t2.abs() + t3.abs()).sum(2) \
        + R_RN_GSIGMA * u * (gb * D * lastT).abs() + TINY * (R_RN_UF + 4 * gd.abs().sum(2))
    k = use.double()
    return (g_rgb * k[:, :, None], bar_rgb * k[:, :, None]), (val * k, bar * k)
