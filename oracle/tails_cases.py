"""Seeded input families of the loss-tail and AdamW tests (tests/test_oracle_tails_float64.py, tests/test_gpu_tails_float64.py,
tests/test_gpu_optim_float64.py).  Built on the CPU, deterministic, fp32.  TEST INFRASTRUCTURE ONLY.

The families sit where training runs and where the formulas are ill conditioned (see oracle/tails_float64.py):
  curvature   a = unit vectors x (1 + 0.05 randn), b = a + delta randn, delta log-uniform: `parallel` [1e-6, 2e-4] (every row
              clamped), `training` [1e-2, 3e-1], `straddle` [5e-4, 3e-3] (both arms of the clamp at 1 - 1e-6); hand-placed rows
              a = b, a = -b, a = 0, |a| = 1e-20, |a| = 1e15 lead every case that has room for them
  eikonal     |g| = 1 + e, e log-uniform in +-[1e-7, 1e-1]; rows g = 0, |g| = 1 exactly, |g| = 1e-25
  normalize   magnitudes log-uniform over 1e-25 ... 1e15; rows at the 1e-12 clamp from both sides and the zero vector
  offsurface / sigmoid   expf arguments out to +-120 (underflow and overflow), exact zeros of both signs
  l1          pred - gt with exact zeros and values around +-1e-8; masks none / all-false / random
  adam        |g| and the moments log-uniform over 1e-30 ... 1e3, 20 % zero gradients, 10 % zero moments; p ~ 1e-4 U(-1, 1) or randn
"""
import math

import torch

SIZES = (1, 63, 64, 65, 255, 256, 257, 5001)
LARGE_N = 4096 * 256 + 257                       # past the first pass of a `stream_grid` launch, ragged end
LARGE_N3 = 3 * 4096 * 256 + 257                  # three full passes: per-thread accumulation carries the loss
CURVATURE_DELTA = {"parallel": (1e-6, 2e-4), "training": (1e-2, 3e-1), "straddle": (5e-4, 3e-3)}
EDGE_CAP = {"parallel": 0.02, "training": 0.02}  # share of rows within E(dot) of a clamp edge; `straddle` is printed, not capped
ADAM_HYPER = ((1e-15, 0.0, 1.0), (1e-8, 0.1, 0.125))        # (eps, weight_decay, grad_scale)
ADAM_STEPS = (1, 2, 3, 10, 1000, 100000)
ADAM_LR, ADAM_BETAS = 1e-3, (0.9, 0.99)


def gen(seed):
    return torch.Generator().manual_seed(int(seed))


def _loguniform(n, lo, hi, g):
    return torch.exp(torch.rand(n, generator=g, dtype=torch.float64) * (math.log(hi) - math.log(lo)) + math.log(lo))


def _units(n, g):
    v = torch.randn(n, 3, generator=g, dtype=torch.float64)
    return v / v.norm(dim=1, keepdim=True).clamp_min(1e-30)


def _sign(n, g):
    return torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0).double()


def curvature(family, N, seed=0):
    """-> a, b [N, 3] fp32"""
    g = gen(1000 + seed + 7 * N)
    lo, hi = CURVATURE_DELTA[family]
    a = _units(N, g) * (1 + 0.05 * torch.randn(N, 1, generator=g, dtype=torch.float64))
    b = a + _loguniform(N, lo, hi, g)[:, None] * torch.randn(N, 3, generator=g, dtype=torch.float64)
    a, b = a.float(), b.float()
    if N >= 64:                                                   # hand-placed rows
        b[0] = a[0]
        b[1] = -a[1]
        a[2] = 0.0
        a[3] = a[3] / a[3].norm() * 1e-20
        a[4] = a[4] / a[4].norm() * 1e15
        b[5] = 0.0
        b[6] = b[6] / b[6].norm() * 1e15
    return a.contiguous(), b.contiguous()


def eikonal(N, seed=0):
    g = gen(2000 + seed + 7 * N)
    e = _loguniform(N, 1e-7, 1e-1, g) * _sign(N, g)
    x = (_units(N, g) * (1 + e)[:, None]).float()
    if N >= 64:
        x[0] = 0.0
        x[1] = torch.tensor([1.0, 0.0, 0.0])
        x[2] = torch.tensor([0.0, -1.0, 0.0])
        x[3] = x[3] / x[3].norm() * 1e-25
        x[4, 1] = 0.0                                             # a zero component of a regular row
    return x.contiguous()


def normalize(N, seed=0):
    """-> x, gy [N, 3] fp32"""
    g = gen(3000 + seed + 7 * N)
    x = (_units(N, g) * _loguniform(N, 1e-25, 1e15, g)[:, None]).float()
    gy = torch.randn(N, 3, generator=g)
    if N >= 64:
        x[0] = 0.0
        x[1] = torch.tensor([1.0, 0.0, 0.0]) * 0.99e-12           # below the clamp
        x[2] = torch.tensor([0.0, 1.0, 0.0]) * 1.01e-12           # above it
        unit = lambda v: v.double() / v.double().norm()           # (a fp32 norm of a 1e-25 vector underflows to 0)
        x[3] = (unit(x[3]) * 0.5e-12).float()
        x[4] = (unit(x[4]) * 2e-12).float()
        gy[5] = unit(x[5]).float()                                # gy parallel to x: the s n.y subtraction cancels
        gy[6] = 0.0
    return x.contiguous(), gy.contiguous()


def shift(N, seed=0):
    """-> points, gradients, rand_directions, g_shifted [N, 3] fp32"""
    g = gen(3500 + seed + 7 * N)
    pts = torch.rand(N, 3, generator=g) - 0.5
    grad = (_units(N, g) * _loguniform(N, 1e-3, 1e2, g)[:, None]).float()
    rnd = torch.randn(N, 3, generator=g)
    gs = torch.randn(N, 3, generator=g) * _loguniform(N, 1e-6, 1e2, g)[:, None].float()
    if N >= 64:
        grad[0] = 0.0
        grad[1] = rnd[1] * 3.0                                    # cross product of parallel vectors
        rnd[2] = 0.0
    return pts.contiguous(), grad.contiguous(), rnd.contiguous(), gs.contiguous()


def offsurface(N, seed=0, sharp=100.0):
    """-> sdf [N] fp32 with sharp |sdf| out to 120"""
    g = gen(4000 + seed + 7 * N)
    arg = torch.cat([_loguniform(N - N // 2, 1e-6, 120.0, g), torch.rand(N // 2, generator=g, dtype=torch.float64) * 120.0])
    s = (arg[torch.randperm(N, generator=g)] * _sign(N, g) / sharp).float()
    if N >= 64:
        s[0], s[1], s[2], s[3] = 0.0, -0.0, 1.2, -1.2
    return s.contiguous()


def sigmoid(N, C=3, seed=0):
    """-> x_fm [C, N], g_y [N, C] fp32; arguments out to +-120"""
    g = gen(5000 + seed + 7 * N + C)
    x = torch.cat([_loguniform(C * N - (C * N) // 2, 1e-6, 120.0, g), torch.rand((C * N) // 2, generator=g, dtype=torch.float64) * 120.0])
    x = (x[torch.randperm(C * N, generator=g)] * _sign(C * N, g)).float().view(C, N)
    if N >= 64:
        x[0, 0], x[0, 1], x[0, 2], x[0, 3] = 0.0, -0.0, 120.0, -120.0
    gy = torch.randn(N, C, generator=g) * _loguniform(N * C, 1e-6, 1e2, g).float().view(N, C)
    return x.contiguous(), gy.contiguous()


def l1(R, C, mask="none", seed=0):
    """-> pred, gt [R, C] fp32, mask [R] bool or None"""
    g = gen(6000 + seed + 7 * R + C)
    gt = torch.rand(R, C, generator=g)
    kind = torch.randint(0, 4, (R, C), generator=g)
    diff = torch.where(kind == 0, torch.zeros(R, C), torch.where(kind == 1, 1e-8 * torch.randn(R, C, generator=g),
                                                                 0.3 * torch.randn(R, C, generator=g)))
    pred = torch.where(kind == 0, gt, gt + diff)
    m = None if mask == "none" else (torch.zeros(R, dtype=torch.bool) if mask == "false" else torch.rand(R, generator=g) < 0.6)
    return pred.contiguous(), gt.contiguous(), m


def adam(n, family="lattice", seed=0):
    """-> p, g, m, v [n] fp32"""
    g = gen(7000 + seed + 7 * n)
    lu = lambda: _loguniform(n, 1e-30, 1e3, g)
    grad = lu() * _sign(n, g)
    grad[torch.rand(n, generator=g) < 0.2] = 0.0
    m, v = lu() * _sign(n, g), lu()
    zm = torch.rand(n, generator=g) < 0.1
    m[zm], v[zm] = 0.0, 0.0
    p = 1e-4 * (2 * torch.rand(n, generator=g, dtype=torch.float64) - 1) if family == "lattice" else torch.randn(n, generator=g, dtype=torch.float64)
    return p.float().contiguous(), grad.float().contiguous(), m.float().contiguous(), v.float().contiguous()


def sample_rows(N, k=1000, seed=0):
    """first k, last k and k seeded random rows of N (sorted, unique)"""
    if N <= 3 * k:
        return torch.arange(N)
    g = gen(8000 + seed)
    return torch.unique(torch.cat([torch.arange(k), torch.arange(N - k, N), torch.randint(0, N, (k,), generator=g)]))
