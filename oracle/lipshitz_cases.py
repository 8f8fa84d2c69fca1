"""Seeded input families of the Lipschitz-normalisation tests (tests/test_oracle_lipshitz_float64.py,
tests/test_gpu_lipshitz_float64.py).  Built on the CPU, deterministic, fp32.  TEST INFRASTRUCTURE ONLY.

SHAPES (out, in): one row of one entry; a lane loop of 1 (in = 1, 63, 64), 2 (65, 111, 128) and 4 (200) trips; tails below and above
one wave; up to 128 rows (one workgroup each).

A case is (W [out, in], c [1], three upstream gradients).  The row sums are PLACED: row r is scaled in float64 to
sum |W_r| = softplus(c) / rho_r for a chosen ratio rho_r, so the arm of every row is known and no row comes near the branch by
accident -- |log10 rho| >= 0.05 (rho <= 0.891 or >= 1.122) except where a family says otherwise:
  inactive     W ~ 0.1 randn times a row scale, c = 2 max row sum (the initialisation of LipshitzMLP): every ratio >= 2
  mixed        rho log-uniform over [0.1, 10] around the gap, about half the rows active, row sums over two decades; c = 1.5
  all_active   rho in [0.05, 0.89]; c = 8
  soft         c in SOFT_C (both sides of softplus's threshold at 20, and down to softplus = 9.4e-14), rows as `mixed`
  zeros        as `mixed` with a quarter of the entries exactly 0 or -0 and one row ALL zeros (it must stay zero, and its backward
               returns G); c = 2.5
  ties         c = 32 (softplus_t returns c), every |W| a multiple of 2^-16, row sums exactly 32, 32 (1 + 2^-20), 32 (1 - 2^-20) in
               turn: every fp32 summation order is exact, the arm is determined, and the row at exactly 32 is ACTIVE in the backward.
               These rows are 9.5e-7 from the branch on purpose; the evaluator's E(ratio) (one rounding of an exact quotient, 6e-8)
               still leaves no edge row
  near_edge    as `mixed` with PLANTED rows (row 0, and row out // 2 where out >= 3) placed at rho = 1 +- a few 1e-8: the only rows
               that may take either arm
Upstream gradients: `ordinary` randn, `small` 1e-6 randn, `orthogonal` randn with its component along the row removed in float64
(gw ~ 0: the formula cancels and the absolute terms of the bar carry it).
"""
import collections
import math

import torch

SHAPES = ((1, 1), (3, 64), (5, 63), (2, 65), (7, 200), (64, 128), (128, 111))
FAMILIES = ("inactive", "mixed", "all_active", "soft", "zeros", "ties", "near_edge")
SOFT_C = (-30.0, -5.0, 0.0, 5.0, 19.999998, 20.0, 20.000002, 40.0)
GRADS = ("ordinary", "small", "orthogonal")
MARGIN = 1e-3                                    # |ratio - 1| of every row that is not planted (and not of `ties`)
NETS = {
    "colour": ((128, 111), (128, 128), (64, 128), (3, 64)),
    "smallest_first": ((3, 64), (128, 111), (128, 128), (64, 128)),      # the grid is sized by the largest out: surplus rows return
    "one": ((7, 200),),
    "eight": SHAPES + ((3, 64),),                                        # the most the multi entries take
}
NET_FAMILIES = ("mixed", "ties", "zeros", "all_active", "inactive", "soft", "near_edge", "mixed")

Case = collections.namedtuple("Case", "label family W c G planted")


def gen(seed):
    return torch.Generator().manual_seed(int(seed))


def _softplus(c):
    c = float(torch.tensor(c, dtype=torch.float32).double())
    return c if c > 20.0 else math.log1p(math.exp(c))


def _rho(kind, n_out, g):
    u = torch.rand(n_out, generator=g, dtype=torch.float64) * 2 - 1
    if kind == "all_active":
        return 10.0 ** (-(0.05 + 1.25 * u.abs()))
    rho = 10.0 ** (torch.sign(u) * (0.05 + 0.95 * u.abs()))
    rho[0] = 10.0 ** (-(0.05 + 0.95 * float(u[0].abs())))          # an active row in every case
    if n_out >= 2:
        rho[1] = 10.0 ** (0.05 + 0.95 * float(u[1].abs()))          # and an inactive one where there is room
    return rho


def _rows(n_out, n_in, sums, g, zeros=False):
    """W with sum |W_r| = sums[r] (float64, then rounded to fp32)"""
    w = torch.randn(n_out, n_in, generator=g, dtype=torch.float64)
    w = torch.where(w == 0, torch.ones_like(w), w)
    if zeros:
        z = torch.rand(n_out, n_in, generator=g) < 0.25
        z[torch.arange(n_out), torch.arange(n_out) % n_in] = False   # every row keeps an entry
        w = torch.where(z, torch.zeros_like(w), w)
    w = (w * (sums / w.abs().sum(1))[:, None]).float()
    if zeros:
        neg = z & (torch.rand(n_out, n_in, generator=g) < 0.5)
        w = torch.where(neg, torch.full_like(w, -0.0), w)
        w[n_out - 1] = 0.0                                           # the all-zero row (the only row of a one-row shape)
        if n_in > 1:
            w[n_out - 1, 1] = -0.0
    return w.contiguous()


def _tie_rows(n_out, n_in, g):
    T0 = 32 * 2 ** 16                                                # 32 in units of 2^-16
    w = torch.empty(n_out, n_in, dtype=torch.float64)
    for r in range(n_out):
        T = T0 + (0, 2, -2)[r % 3]
        p = torch.rand(n_in, generator=g, dtype=torch.float64) + 0.1
        k = torch.floor(T * p / p.sum()).to(torch.int64)
        k[0] += T - int(k.sum())
        sgn = torch.where(torch.rand(n_in, generator=g) < 0.5, -1.0, 1.0).double()
        w[r] = sgn * k.double() * 2.0 ** -16
    assert bool((w.float().double() == w).all())
    return w.float().contiguous()


def grads(W, g):
    """-> dict of the three upstream gradients"""
    w = W.double()
    g0 = torch.randn(W.shape, generator=g, dtype=torch.float64)
    ww = (w * w).sum(1, keepdim=True)
    orth = g0 - torch.where(ww > 0, (g0 * w).sum(1, keepdim=True) / ww.clamp_min(1e-300), torch.zeros_like(ww)) * w
    return {"ordinary": torch.randn(W.shape, generator=g).contiguous(),
            "small": (1e-6 * torch.randn(W.shape, generator=g)).contiguous(),
            "orthogonal": orth.float().contiguous()}


def _case(label, family, W, c, g, planted=()):
    mask = torch.zeros(W.shape[0], dtype=torch.bool)
    for r in planted:
        mask[r] = True
    return Case(label, family, W, torch.tensor([c], dtype=torch.float32), grads(W, g), mask)


def cases(family, n_out, n_in):
    """-> [Case]: one, or one per bound of SOFT_C"""
    g = gen(7000 + 1009 * FAMILIES.index(family) + 31 * n_out + n_in)
    label = "%s %dx%d" % (family, n_out, n_in)
    if family == "inactive":
        scale = 10.0 ** (torch.rand(n_out, 1, generator=g) * 2 - 1)
        W = (0.1 * torch.randn(n_out, n_in, generator=g) * scale).contiguous()
        c = float(W.abs().sum(1).max() * 2)
        return [_case(label, family, W, c, g)]
    if family == "ties":
        return [_case(label, family, _tie_rows(n_out, n_in, g), 32.0, g)]
    if family == "soft":
        return [_case("%s c=%r" % (label, c), family, _rows(n_out, n_in, _softplus(c) / _rho("mixed", n_out, g), g), c, g) for c in SOFT_C]
    c = {"mixed": 1.5, "all_active": 8.0, "zeros": 2.5, "near_edge": 1.0}[family]
    rho = _rho("all_active" if family == "all_active" else "mixed", n_out, g)
    planted = ()
    if family == "near_edge":
        planted = (0,) if n_out < 3 else (0, n_out // 2)
        for i, r in enumerate(planted):
            rho[r] = 1.0 + (2e-8, -3e-8)[i]
    return [_case(label, family, _rows(n_out, n_in, _softplus(c) / rho, g, zeros=family == "zeros"), c, g, planted)]


def net(name):
    """-> [Case], one per layer of NETS[name]; the families change from layer to layer"""
    out = []
    for l, (o, i) in enumerate(NETS[name]):
        cs = cases(NET_FAMILIES[l], o, i)
        out.append(cs[2] if len(cs) > 1 else cs[0])                  # soft: c = 0
    return out
