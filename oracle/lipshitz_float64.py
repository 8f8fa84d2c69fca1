"""FLOAT64 EVALUATOR of the Lipschitz weight normalisation of the colour network (lipshitz_norm_fwd_kernel, lipshitz_norm_bwd_kernel
and lipshitz_norm_multi_kernel in csrc/mlp_wide.hip).  TEST INFRASTRUCTURE ONLY.

Plain torch float64 on the CPU, no autograd, no HIP.  Inputs are fp32 tensors taken exactly.  Every function returns the float64
value together with a PER-ENTRY BAR on |fp32 kernel - float64|, in the manner of oracle/tails_float64.py (whose running-error
primitives are reused, with U, TINY, SLACK, ULP_EXPF, ULP_LOG1PF and bites of oracle/composite_float64.py).

One wave per row r of W [out, in]; every intermediate z carries a bound E(z) of |fp32 z - float64 z|:
    A  = sum_j |W_rj|      each lane adds ceil(in / 64) terms, six butterfly steps follow (psdf::wave_sum; every lane ends with the
                           same bits because the addition commutes):  E(A) = (ceil(in / 64) + 6) u A SLACK.
                           E(A) = 0 where every |W_rj| is a multiple of one power of two q and A / q <= 2^24: every partial sum
                           of every order is then an fp32 number (the `ties` family of oracle/lipshitz_cases.py).
    gw = sum_j G_rj W_rj   the same path, one rounding more per product:  E(gw) = (ceil(in / 64) + 7) u sum |G W| SLACK + in 2^-126
    sp = softplus_t(c)     c itself for c > 20 (E = 0), else log1pf(expf(c)):  E(e) = 2 ULP_EXPF u e + 2^-126,
                           E(sp) = E(e) / (1 + e - E(e)) + 2 ULP_LOG1PF u sp + 2^-126
    ratio = sp / A         the quotient rule of tails_float64._div; its rounding term is dropped where sp and A are exact and the
                           float64 quotient is an fp32 number (a correctly rounded division then returns it)
    sigma(c)               1 for c > 20, else 1 / (1 + expf(-c)): composite_float64._sigmoid

FORWARD   Wn = W min(ratio, 1).  A row with ratio - E(ratio) >= 1 has scale 1 in fp32 whatever the order: Wn = W BIT FOR BIT, bar 0
          (so does a row of zeros: A = 0, ratio = inf, or nan when sp underflowed too, and fminf returns 1).  Otherwise
          E(Wn) = |W| E(ratio) + u |Wn| + 2^-126 -- min(., 1) is 1-Lipschitz, so this holds on either side of the branch.
BACKWARD  active rows (ratio <= 1, as torch's clamp backward):  dW_j = g ratio - gw sp / (a a) sgn(w), sgn(0) = 0, in the kernel's
          order ((gw sp) / (a a)) sgn, one product, one quotient, one product, one difference, each through the rules above; a
          fused multiply-add only removes a rounding.  Entries with w = 0: g ratio alone.  Inactive rows: dW = G exactly, bar 0.
          The formula cancels where G is nearly orthogonal to its row (gw ~ 0 against sum |G W|): the terms above are absolute.
dc        dc0 + sum over active rows of t_r = (gw / a) sigma(c), one float atomic per active row in any order:
          bar = (n u sum |t_r| + sum E(t_r) + n u |dc0|) SLACK, n = number of active rows.
BRANCH    a row whose float64 ratio lies within E(ratio) > 0 of 1 may take either arm in fp32: reported in `edge`, with the values
          and bars of the active arm (`dW_open`); its term widens the bar of dc by |t_r| + E(t_r).

No constant of any bar is fitted to what the kernels produce.
"""
import math

import torch

from oracle.composite_float64 import SLACK, TINY, U, ULP_EXPF, ULP_LOG1PF, _sigmoid, bites  # noqa: F401  (bites: re-exported)
from oracle.tails_float64 import INF, _add, _d, _div, _fin, _mul, _z

MAX_LAYERS = 8            # LIP_MAX_LAYERS of csrc/mlp_wide.hip
THRESHOLD = 20.0          # torch's softplus threshold, as softplus_t holds it


def lane_trips(n_in):
    return -(-int(n_in) // 64)


def _scalar(x):
    return torch.tensor(float(x), dtype=torch.float64)


def bound_value(c):
    """the fp32 bound as a python float, taken exactly"""
    return float(_d(c).reshape(-1)[0]) if torch.is_tensor(c) else float(torch.tensor(c, dtype=torch.float32).double())


def softplus_t(c):
    """-> (sp, E) as python floats"""
    c = bound_value(c)
    if c > THRESHOLD:
        return c, 0.0
    e = math.exp(c)
    Ee = 2 * ULP_EXPF * U * e + TINY
    sp = math.log1p(e)
    return sp, Ee / (1.0 + e - Ee) + 2 * ULP_LOG1PF * U * sp + TINY


def sigma_t(c):
    """-> (sigma, E) as python floats"""
    c = bound_value(c)
    if c > THRESHOLD:
        return 1.0, 0.0
    x = _scalar(c)
    s, _, E = _sigmoid(x, _z(x), ULP_EXPF)
    return float(s), float(E)


def exact_sum_rows(absW):
    """[out] bool: every |W_rj| is a multiple of one power of two q and sum / q <= 2^24, so every partial sum is an fp32 number"""
    mant, exp = torch.frexp(absW)
    mi = (mant * 2.0 ** 24).to(torch.int64)                       # fp32 values: 24 significant bits at the most
    low = (mi & -mi).double() * torch.exp2((exp - 24).double())    # the lowest set bit of each entry
    q = torch.where(absW == 0, torch.full_like(absW, INF), low).min(dim=1).values
    A = absW.sum(1)
    return (A == 0) | (A / q <= 2.0 ** 24)


class Rows:
    """what both directions share: A, sp, ratio with their bounds, and which arm each row takes"""

    def __init__(self, W, c):
        w = _d(W)
        assert w.dim() == 2
        self.w, self.n_out, self.n_in = w, w.shape[0], w.shape[1]
        self.m = lane_trips(self.n_in) + 6
        aw = w.abs()
        self.A = aw.sum(1)
        self.E_A = torch.where(exact_sum_rows(aw), _z(self.A), self.m * U * self.A * SLACK)
        self.c = bound_value(c)
        self.sp, self.E_sp = softplus_t(self.c)
        self.zero = self.A == 0
        a = torch.where(self.zero, torch.ones_like(self.A), self.A)
        spv, Espv = torch.full_like(a, self.sp), torch.full_like(a, self.E_sp)
        ratio, Er = _div(spv, Espv, a, self.E_A)
        exact = (self.E_A == 0) & (Espv == 0) & (ratio.float().double() == ratio)
        self.a, self.spv, self.E_spv = a, spv, Espv
        self.ratio = torch.where(self.zero, torch.full_like(ratio, INF), ratio)
        self.E_ratio = torch.where(self.zero | exact, _z(Er), Er)
        self.edge = ~self.zero & (self.E_ratio > 0) & ((self.ratio - 1.0).abs() <= self.E_ratio)
        self.active = ~self.zero & (self.ratio <= 1.0)
        self.one = self.zero | (self.ratio - self.E_ratio >= 1.0)   # scale is exactly 1 in fp32


def forward(W, c):
    """lipshitz_norm_fwd_kernel / the forward arm of the multi kernel.  -> dict(Wn, Wn_bar [out, in], ratio, E_ratio, edge, active,
    one [out])"""
    r = Rows(W, c)
    w = r.w
    scale = torch.where(r.one, torch.ones_like(r.ratio), r.ratio.clamp_max(1.0))
    Wn = w * scale[:, None]
    bar = w.abs() * r.E_ratio[:, None] + U * Wn.abs() + TINY
    bar = torch.where(r.one[:, None] | (w == 0), _z(bar), bar)
    return dict(Wn=Wn, Wn_bar=_fin(bar), ratio=r.ratio, E_ratio=r.E_ratio, edge=r.edge, active=r.active, one=r.one)


def backward(W, c, G, dc0=0.0):
    """lipshitz_norm_bwd_kernel / the backward arm of the multi kernel.  -> dict(dW, dW_bar [out, in]: the arm float64 takes;
    dW_open, dW_open_bar: the active arm for every row (what an `edge` row may hold instead of G); dc, dc_bar (python floats);
    terms, E_terms, gw, E_gw, ratio, E_ratio, edge, active [out])"""
    r = Rows(W, c)
    w, g = r.w, _d(G).reshape(r.w.shape)
    t = g * w
    gw = t.sum(1)
    E_gw = (r.m + 1) * U * t.abs().sum(1) * SLACK + r.n_in * TINY
    ratio = torch.where(r.zero, torch.ones_like(r.ratio), r.ratio)
    # ---- the active arm: g ratio - ((gw sp) / (a a)) sgn
    t1, Et1 = _mul(gw, E_gw, r.spv, r.E_spv)
    aa, Eaa = _mul(r.a, r.E_A, r.a, r.E_A)
    t2, Et2 = _div(t1, Et1, aa, Eaa)
    p, Ep = _mul(g, _z(g), ratio[:, None].expand_as(g), r.E_ratio[:, None].expand_as(g))
    sgn = torch.sign(w)
    t3, Et3 = t2[:, None] * sgn, Et2[:, None] * sgn.abs()
    op, Eop = _add(p, Ep, t3, Et3, -1.0)
    Eop = torch.where(sgn == 0, Ep, Eop)                            # (t2 * 0) is 0: the product alone
    act = r.active[:, None].expand_as(g)
    dW = torch.where(act, op, g)
    bar = torch.where(act, Eop, _z(Eop))
    # ---- dc
    sig, E_sig = sigma_t(r.c)
    q, Eq = _div(gw, E_gw, r.a, r.E_A)
    if r.c > THRESHOLD:
        term, E_term = q, Eq                                        # times 1.0f: exact
    else:
        term, E_term = _mul(q, Eq, torch.full_like(q, sig), torch.full_like(q, E_sig))
    sure = r.active & ~r.edge
    n = int((r.active | r.edge).sum())
    dc0 = float(dc0)
    dc = dc0 + float(term[r.active].sum())
    dc_bar = (n * U * float(term[r.active | r.edge].abs().sum()) + float(E_term[sure].sum()) + n * U * abs(dc0)) * SLACK \
        + float((term.abs() + E_term)[r.edge].sum())
    return dict(dW=dW, dW_bar=_fin(bar), dW_open=op, dW_open_bar=_fin(Eop), dc=dc, dc_bar=dc_bar, terms=term, E_terms=E_term, gw=gw,
                E_gw=E_gw, ratio=r.ratio, E_ratio=r.E_ratio, edge=r.edge, active=r.active)
