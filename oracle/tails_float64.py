"""FLOAT64 EVALUATORS of the loss tails (second block of csrc/neus.hip) and of AdamW (csrc/optim.hip).  TEST INFRASTRUCTURE ONLY.

Plain torch float64 on the CPU, no autograd, no HIP.  Inputs are fp32 tensors taken exactly.  Every function returns the
float64 value together with a PER-ENTRY BAR on |fp32 kernel - float64|, in the manner of oracle/composite_float64.py (whose
U, TINY, SLACK, ULP_EXPF and bites are reused).

ELEMENTWISE OUTPUTS: a first-order running error analysis of the expressions as csrc/neus.hip writes them.  Every intermediate
z carries a bound E(z) of |fp32 z - float64 z|:
    z = x op y, rounded once:     E(z) = |dz/dx| E(x) + |dz/dy| E(y) + u |z|   (+ 2^-126 where a product or quotient may underflow)
    a.b of 3-vectors:             E = sum_k (|b_k| E(a_k) + |a_k| E(b_k)) + 3 u sum_k |a_k b_k| + 3 * 2^-126
    sqrtf, correctly rounded:     E = min(E(x) / (sqrt(x) + sqrt(max(x - E(x), 0))), sqrt(E(x))) + u sqrt(x)
                                  (|sqrt(x') - sqrt(x)| = |x' - x| / (sqrt(x') + sqrt(x)); both bounds hold for every x, x' >= 0)
    x / y, correctly rounded:     E = (E(x) + |x / y| E(y)) / (|y| - E(y)) + u |x / y|  (rigorous in y; infinite when E(y) >= |y|:
                                  fp32 may then hold any quotient, e.g. the 0 it returns for |g| = 1e-25 in the eikonal gradient)
    expf within ULP_EXPF, acosf within ULP_ACOSF ulps; acos(clamp(d)) moves by at most
                                  max |acos(clamp(d +- E(d))) - acos(clamp(d))| (monotone: no linearisation at the steep ends).
A fused multiply-add only removes a rounding, so the bounds hold with and without contraction.  Where the FORMULA is ill
conditioned the terms above are absolute by construction and dominate: e = |g| - 1 of the eikonal gradient (E(e) ~ 2.5 u against
e -> 0), (1 - d)(1 + d) and the dot d of two normalised vectors of the curvature gradient (E(d) ~ 8 u against 1 - d), and
inv gy - s n.y of normalize_bwd (both terms ~ |gy| / |x| when gy is nearly parallel to x).

BRANCHES.  `norm > 1e-12` (normalize_bwd) and `lo <= d <= hi` (curvature) are decided by fp32 values: an entry whose float64
value lies within its E of the edge may take either arm.  normalize: the bar is widened by the distance between the arms.
curvature: the entry is reported in `edge`, with the open-arm value and bar; it passes when it is inside that bar or EXACTLY the
clamped-arm value (0).

LOSS SCALARS.  loss = loss0 + scale sum_n t_n, summed as: per-thread accumulation over the grid-stride passes, 6 wave steps,
4 wave partials, one product by scale, one atomicAdd per workgroup in any order.
    bar = ((m + r) u |scale| sum |t| + |scale| sum E(t) + grid u |loss0|) SLACK,
    m = ceil(N / (grid 256)) + 6 + 4 + grid additions at most on the path of any term, r = 1 (the product by scale),
    grid from the documented launch rule (`stream_grid`: min(ceil(N / 256), 4096); L1: min(ceil(R C / 1024), 256)).
    The last term exists only for a pre-filled accumulator: what it held goes through the `grid` atomic additions.  The tests
    check the losses from a zero accumulator, where the bar is a fraction of what the kernel added and of nothing else; the
    pre-filled case is checked once per kernel with a contribution comparable to loss0.

ADAMW.  The update rule of adamw_range with hyper-parameters as the C ABI receives them (fp32).  The bias corrections are
evaluated in float64 from those values; the host's fp32 `1 - powf(beta, step)` is within (2 u b^s) / (1 - b^s) + u relative of
it (powf within one ulp = 2 u relative, one subtraction), halved through sqrtf for beta2.  Bars of m', v' come from the rounding
of each operation (2^-126 terms for g^2, b2 v and the products that may underflow); the update D = (lr / bc1) m' / denom is
evaluated from the float64 m', v' and its bar carries E(m'), E(v') (through min(E / sqrt(v'), sqrt(E))), so the kernel's own
fp32 moments are covered; p' = p (1 - lr wd) - D has the bar 3 u |p| + E(D) + u |p'|.

No constant of any bar is fitted to what the kernels produce.
"""
import math

import torch

from oracle.composite_float64 import SLACK, TINY, U, ULP_EXPF, _f32, _sigmoid, bites  # noqa: F401  (bites: re-exported)

ULP_ACOSF = 3             # measured worst 1.425 ulp on [1e-30, 1 - 1e-6], 1.304 on [-1 + 1e-6, -1e-30]  -> 2, + 1   (LABNOTES.md)

C_EPS12 = _f32(1e-12)                                  # F.normalize's eps as the kernels hold it
C_LO = _f32(-1.0 + _f32(1e-6))                         # -1.0f + 1e-6f, rounded once
C_HI = _f32(1.0 - _f32(1e-6))
C_INV_PI = _f32(1.0 / math.pi)
INF = float("inf")
BLOCK = 256
STREAM_GRID_CAP, L1_GRID_CAP = 4096, 256


def _d(t):
    return t.detach().cpu().double()


def _z(x):
    return torch.zeros_like(x)


def _fin(E):
    """a bound that came out as nan (inf * 0, inf - inf) bounds nothing"""
    return torch.where(torch.isnan(E), torch.full_like(E, INF), E)


# ------------------------------------------------------------------------------------------------ running-error primitives
def _mul(a, Ea, b, Eb):
    z = a * b
    return z, _fin(Ea * b.abs() + a.abs() * Eb + Ea * Eb + U * z.abs() + TINY)


def _add(a, Ea, b, Eb, sign=1.0):
    z = a + sign * b
    return z, _fin(Ea + Eb + U * z.abs())


def _sqrt(x, Ex):
    s = x.clamp_min(0).sqrt()
    lin = torch.where(s > 0, Ex / (s + (x - Ex).clamp_min(0).sqrt()).clamp_min(1e-300), torch.full_like(s, INF))
    return s, _fin(torch.minimum(lin, Ex.sqrt()) + U * s)


def _div(a, Ea, b, Eb):
    q = a / torch.where(b == 0, torch.ones_like(b), b)
    room = b.abs() - Eb
    E = torch.where(room > 0, (Ea + q.abs() * Eb) / room.clamp_min(1e-300) + U * q.abs() + TINY, torch.full_like(q, INF))
    return q, _fin(E)


def _dot3(a, Ea, b, Eb):
    t = a * b
    return t.sum(-1), _fin((Ea * b.abs() + a.abs() * Eb + Ea * Eb).sum(-1) + 3 * U * t.abs().sum(-1) + 3 * TINY)


def _cross3(a, Ea, b, Eb):
    def comp(i, j):
        p, q = a[..., i] * b[..., j], a[..., j] * b[..., i]
        E = Ea[..., i] * b[..., j].abs() + a[..., i].abs() * Eb[..., j] + Ea[..., j] * b[..., i].abs() + a[..., j].abs() * Eb[..., i] \
            + Ea[..., i] * Eb[..., j] + Ea[..., j] * Eb[..., i]
        return p - q, E + 2 * U * (p.abs() + q.abs()) + 2 * TINY
    v, E = zip(comp(1, 2), comp(2, 0), comp(0, 1))
    return torch.stack(v, -1), _fin(torch.stack(E, -1))


class _Nrm:
    """normalize_eps: y = x / max(|x|, 1e-12)"""

    def __init__(self, x, Ex=None):
        Ex = _z(x) if Ex is None else Ex
        d, Ed = _dot3(x, Ex, x, Ex)
        self.norm, self.E_norm = _sqrt(d, Ed)
        # max(., c) is 1-Lipschitz; below the clamp by more than E(norm) both precisions hold the constant itself
        self.denom = self.norm.clamp_min(C_EPS12)
        self.E_denom = torch.where(self.norm + self.E_norm <= C_EPS12, _z(self.norm), self.E_norm)
        den, Eden = self.denom[..., None].expand_as(x), self.E_denom[..., None].expand_as(x)
        self.y, self.E_y = _div(x, Ex, den, Eden)
        self.above = self.norm > C_EPS12
        self.near = (self.norm - C_EPS12).abs() <= self.E_norm


def _normalize_bwd(n, gy, Egy):
    """normalize_bwd: inv gy - [norm > eps] (gy . y inv) y"""
    one = torch.ones_like(n.denom)
    inv, Einv = _div(one, _z(one), n.denom, n.E_denom)
    g0, Eg0 = _mul(inv[..., None].expand_as(gy), Einv[..., None].expand_as(gy), gy, Egy)
    dt, Edt = _dot3(gy, Egy, n.y, n.E_y)
    s, Es = _mul(dt, Edt, inv, Einv)
    t, Et = _mul(s[..., None].expand_as(gy), Es[..., None].expand_as(gy), n.y, n.E_y)
    g1, Eg1 = _add(g0, Eg0, t, Et, -1.0)
    ab = n.above[..., None].expand_as(gy)
    val = torch.where(ab, g1, g0)
    bar = torch.where(ab, Eg1, Eg0)
    near = n.near[..., None].expand_as(gy)
    bar = torch.where(near, torch.maximum(Eg0, Eg1) + (g1 - g0).abs(), bar)        # either arm
    return val, _fin(bar)


# ------------------------------------------------------------------------------------------------------ the loss scalar
def stream_grid(N):
    return max(1, min(-(-int(N) // BLOCK), STREAM_GRID_CAP))


def l1_grid(total):
    return max(1, min(-(-int(total) // (BLOCK * 4)), L1_GRID_CAP))


def chain_length(N, grid):
    """longest addition chain on the way of one term into the loss (see the module docstring)"""
    return -(-int(N) // (grid * BLOCK)) + 6 + 4 + grid


def loss_scalar(t, Et, scale, N, grid, loss0=0.0):
    """-> (float64 loss, bar) of loss0 + scale sum t"""
    scale, loss0 = _f32(scale), float(loss0)
    val = loss0 + scale * float(t.sum())
    m, r = chain_length(N, grid), 1
    bar = ((m + r) * U * abs(scale) * float(t.abs().sum()) + abs(scale) * float(Et.sum()) + grid * U * abs(loss0)) * SLACK + TINY
    return val, bar


# --------------------------------------------------------------------------------------------------------------- L1
def l1_loss(pred, gt, mask, scale, loss0=0.0):
    """l1_loss_kernel.  -> dict(loss, loss_bar, grad [R, C] EXACT: +-scale or 0)"""
    p, g = _d(pred), _d(gt)
    R, C = p.shape
    m = torch.ones(R, 1, dtype=torch.float64) if mask is None else (_d(mask).reshape(R, 1) != 0).double()
    d = p - g
    t, Et = d.abs() * m, U * d.abs() * m
    loss, bar = loss_scalar(t, Et, scale, R * C, l1_grid(R * C), loss0)
    return dict(loss=loss, loss_bar=bar, grad=torch.sign(d) * _f32(scale) * m)


# ---------------------------------------------------------------------------------------------------------- eikonal
def eikonal_loss(gradients, scale, loss0=0.0):
    """eikonal_loss_kernel: sum (|g| - 1)^2;  grad = (|g| > 0 ? scale 2 e / |g| : 0) g"""
    g = _d(gradients)
    N = g.shape[0]
    sc = _f32(scale)
    dd, Edd = _dot3(g, _z(g), g, _z(g))
    nrm, Enrm = _sqrt(dd, Edd)
    e, Ee = nrm - 1.0, Enrm + U * (nrm - 1.0).abs()
    t = e * e
    Et = 2 * e.abs() * Ee + Ee * Ee + U * t
    loss, bar = loss_scalar(t, Et, scale, N, stream_grid(N), loss0)
    a, Ea = 2 * sc * e, 2 * abs(sc) * Ee + U * (2 * sc * e).abs()
    c, Ec = _div(a, Ea, nrm, Enrm)
    c, Ec = torch.where(nrm > 0, c, _z(c)), torch.where(nrm > 0, Ec, _z(Ec))       # g = 0: exactly 0
    grad, Eg = _mul(c[:, None].expand_as(g), Ec[:, None].expand_as(g), g, _z(g))
    Eg = torch.where(g == 0, _z(Eg), Eg)
    return dict(loss=loss, loss_bar=bar, grad=grad, grad_bar=Eg)


# -------------------------------------------------------------------------------------------------------- normalize3
def normalize3(x):
    n = _Nrm(_d(x))
    return n.y, n.E_y


def normalize3_backward(x, gy):
    return _normalize_bwd(_Nrm(_d(x)), _d(gy), _z(_d(gy)))


# --------------------------------------------------------------------------------------------------- curvature shift
def curvature_shift(points, gradients, rnd, eps):
    p, a, r = _d(points), _Nrm(_d(gradients)), _Nrm(_d(rnd))
    eps = torch.full_like(p, _f32(eps))
    t, Et = _cross3(a.y, a.E_y, r.y, r.E_y)
    et, Eet = _mul(eps, _z(eps), t, Et)
    return _add(p, _z(p), et, Eet)


def curvature_shift_backward(gradients, rnd, eps, g_shifted):
    a, r, gs = _Nrm(_d(gradients)), _Nrm(_d(rnd)), _d(g_shifted)
    eps = torch.full_like(gs, _f32(eps))
    gt, Egt = _mul(eps, _z(eps), gs, _z(gs))
    c, Ec = _cross3(r.y, r.E_y, gt, Egt)
    return _normalize_bwd(a, c, Ec)


# ---------------------------------------------------------------------------------------------------- curvature loss
def curvature_loss(a, b, scale, loss0=0.0, ulp_acosf=None):
    """curvature_loss_kernel.  -> dict(loss, loss_bar, ga, ga_bar, gb, gb_bar [N, 3], dot, E_dot, clamped, edge [N] bool,
    ga_open, ga_open_bar, gb_open, gb_open_bar: what the open arm gives, for the `edge` rows)"""
    ulp = ULP_ACOSF if ulp_acosf is None else ulp_acosf
    na, nb = _Nrm(_d(a)), _Nrm(_d(b))
    N = na.norm.shape[0]
    sc = _f32(scale)
    dot, Edot = _dot3(na.y, na.E_y, nb.y, nb.E_y)
    cl = lambda x: x.clamp(C_LO, C_HI)
    u = cl(dot)
    ac = torch.acos(u)
    Eac = torch.maximum((torch.acos(cl(dot - Edot)) - ac).abs(), (torch.acos(cl(dot + Edot)) - ac).abs()) + 2 * ulp * U * ac
    t, Et = ac * C_INV_PI, Eac * C_INV_PI + 2 * U * ac * C_INV_PI                  # the fp32 1/pi and the product
    loss, bar = loss_scalar(t, Et, scale, N, stream_grid(N), loss0)
    clamped = (dot < C_LO) | (dot > C_HI)
    edge = ((dot - C_LO).abs() <= Edot) | ((dot - C_HI).abs() <= Edot)
    # the open arm, evaluated for every row (u = the clamped dot keeps it finite where the row is clamped)
    c0 = sc * C_INV_PI
    Ec0 = 2 * U * abs(c0)
    w1, w2 = 1.0 - u, 1.0 + u
    pr, Epr = _mul(w1, Edot + U * w1.abs(), w2, Edot + U * w2.abs())
    sq, Esq = _sqrt(pr, Epr)
    gu, Egu = _div(torch.full_like(sq, -c0), torch.full_like(sq, Ec0), sq, Esq)

    def side(n, other):
        gy, Egy = _mul(gu[:, None].expand_as(other.y), Egu[:, None].expand_as(other.y), other.y, other.E_y)
        return _normalize_bwd(n, gy, Egy)
    ga_o, Ea_o = side(na, nb)
    gb_o, Eb_o = side(nb, na)
    k = clamped[:, None].expand_as(ga_o)
    zero = _z(ga_o)
    return dict(loss=loss, loss_bar=bar, dot=dot, E_dot=Edot, clamped=clamped, edge=edge, term=t,
                ga=torch.where(k, zero, ga_o), ga_bar=torch.where(k, zero, Ea_o), gb=torch.where(k, zero, gb_o), gb_bar=torch.where(k, zero, Eb_o),
                ga_open=ga_o, ga_open_bar=Ea_o, gb_open=gb_o, gb_open_bar=Eb_o)


# -------------------------------------------------------------------------------------------------------- offsurface
def offsurface_loss(sdf, sharp, scale, loss0=0.0, ulp_expf=ULP_EXPF):
    """offsurface_loss_kernel: sum exp(-sharp |s|);  grad = scale e (-sharp sign(s))"""
    s = _d(sdf).reshape(-1)
    N = s.numel()
    sh, sc = _f32(sharp), _f32(scale)
    y = -sh * s.abs()
    Ey = U * y.abs()
    e = torch.exp(y)
    Ee = e * (torch.expm1(Ey) + 2 * ulp_expf * U) + TINY
    loss, bar = loss_scalar(e, Ee, scale, N, stream_grid(N), loss0)
    se, Ese = sc * e, abs(sc) * Ee + U * (sc * e).abs() + TINY
    grad = se * (-sh * torch.sign(s))
    Eg = torch.where(s == 0, _z(s), Ese * abs(sh) + U * grad.abs() + TINY)
    return dict(loss=loss, loss_bar=bar, grad=grad, grad_bar=Eg)


# ------------------------------------------------------------------------------------------------------ sigmoid rows
def sigmoid_rows(x_fm, ulp_expf=ULP_EXPF):
    """[C, N] -> sigmoid as [N, C]"""
    x = _d(x_fm).t().contiguous()
    s, _, E = _sigmoid(x, _z(x), ulp_expf)
    return s, E


def sigmoid_rows_backward(g_y, y):
    """[N, C], [N, C] -> g y (1 - y) as [C, N]"""
    g, y = _d(g_y), _d(y)
    a, Ea = _mul(g, _z(g), y, _z(y))
    b = 1.0 - y
    out, E = _mul(a, Ea, b, U * b.abs())
    return out.t().contiguous(), E.t().contiguous()


# ------------------------------------------------------------------------------------------------------------- AdamW
def bias_corrections(beta1, beta2, step):
    """float64 bc1 = 1 - b1^s, sqrt(bc2) from the fp32 betas, and the relative bound of the host's fp32 values of both"""
    b1, b2, s = _f32(beta1), _f32(beta2), int(step)
    p1, p2 = b1 ** s, b2 ** s
    bc1, bc2 = 1.0 - p1, 1.0 - p2
    rel1 = 2 * U * p1 / bc1 + U
    rel2s = 0.5 * (2 * U * p2 / bc2 + U) + U                                       # + the rounding of sqrtf
    return bc1, math.sqrt(bc2), rel1, rel2s


def adamw(p, g, m, v, lr, beta1, beta2, eps, wd, step, grad_scale, _variant=None):
    """adamw_range for one step.  -> dict(p, p_bar, m, m_bar, v, v_bar, delta, delta_bar).
    `_variant`: deliberately WRONG update rules for the CPU test of the bars ("no_eps", "no_grad_scale_in_v", "step_off_by_one")"""
    p, g, m, v = _d(p), _d(g), _d(m), _d(v)
    lr, b1, b2, eps, wd, gs = _f32(lr), _f32(beta1), _f32(beta2), _f32(eps), _f32(wd), _f32(grad_scale)
    bc1, bc2s, rel1, rel2s = bias_corrections(beta1, beta2, step + (1 if _variant == "step_off_by_one" else 0))
    if _variant == "no_eps":
        eps = 0.0
    gk = g * gs
    Egk = _z(gk) if gs == 1.0 else U * gk.abs() + TINY
    p1 = p * (1.0 - lr * wd)
    omb1, omb2 = 1.0 - b1, 1.0 - b2
    t1, Et1 = b1 * m, U * (b1 * m).abs() + TINY
    t2 = omb1 * gk
    Et2 = gk.abs() * U * omb1 + omb1 * Egk + U * t2.abs() + TINY
    m1, Em1 = _add(t1, Et1, t2, Et2)
    gv, Egv = (g, _z(g)) if _variant == "no_grad_scale_in_v" else (gk, Egk)
    s1 = omb2 * gv
    Es1 = gv.abs() * U * omb2 + omb2 * Egv + U * s1.abs() + TINY
    s2, Es2 = _mul(s1, Es1, gv, Egv)
    bv = b2 * v
    v1, Ev1 = _add(bv, U * bv.abs() + TINY, s2, Es2)
    sq, Esq = _sqrt(v1, Ev1)
    q1 = sq / bc2s
    Eq1 = Esq / bc2s + q1 * rel2s + U * q1 + TINY
    den = q1 + eps
    Eden = Eq1 + U * den
    r, Er = _div(m1, Em1, den, Eden)
    r, Er = torch.where(m1 == 0, _z(r), r), torch.where((m1 == 0) & (Em1 == 0), _z(Er), Er)
    c = lr / bc1
    Ec = abs(c) * (rel1 + U)
    delta = c * r
    Edelta = _fin(r.abs() * Ec + abs(c) * Er + U * delta.abs() + TINY)
    p2 = p1 - delta
    return dict(p=p2, p_bar=3 * U * p.abs() + Edelta + U * p2.abs(), m=m1, m_bar=Em1, v=v1, v_bar=Ev1, delta=delta, delta_bar=Edelta)
