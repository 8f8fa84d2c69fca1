"""FLOAT64 EVALUATOR of the per-image colour calibration with its sigmoid (csrc/colorcal.hip).  A helper of
tests/test_colorcal_host.py and tests/test_gpu_nerf_colorcal.py: no test lives here.

Plain torch float64 on the CPU, NO AUTOGRAD: values and gradients are written out.  Inputs are fp32 tensors taken exactly.

For sample s of ray r drawn from image i = img_idx[r], channel c:
    w = 1 + weight_delta[i, c],  b = bias[i, c]      (w = 1, b = 0 for the fixed image and for an image outside [0, I))
    z = raw w + b,   rgb = sigmoid(z)
and for an upstream g_rgb, with y the rgb the backward is HANDED (the forward's fp32 output, taken exactly):
    g_pre = g_rgb y (1 - y),   g_raw = g_pre w
    g_ray[r] = [sum_s g_pre raw (3 channels), sum_s g_pre (3 channels)]        (0 for rays that keep the identity)
    g_weight_delta[i] = sum over the rays of image i and over the branches of g_ray[r, 0:3],  g_bias[i] of g_ray[r, 3:6]
Slots no ray owns, empty rays and rays whose range leaves the pool: nothing is computed, their gradients are 0.

BARS.  u = 2^-24; every bar times SLACK = 1 / (1 - 2048 u) for the second-order terms, plus 2^-126 per operation for underflow.
    forward   w = 1 + weight_delta is formed in fp32: one rounding, relative u.  z = fl(fl(raw w) + b): the product carries w's
              rounding and its own, 2 u |raw w|, the sum one more, u |z|:  E_z = (2 |raw w| + |z|) u  (an identity ray: w exact,
              the product exact, the sum exact: E_z = 0).  Through the sigmoid: |d sigmoid| <= s (1 - s) |dz| (<= |dz| / 4), and
              the evaluation 1 / (1 + expf(-z)) itself as oracle/composite_float64.py states it for every sigmoid of the tree
              (`_sigmoid`: expf within ULP_EXPF ulps, 1 + e and the reciprocal one rounding each):
              E = s ((1 - s) (expm1(E_z) + 2 ULP_EXPF u) + 2 u).
    g_raw     g y, 1 - y, their product, times w, and w's own rounding: 5 u |g_raw|   (four multiply-class roundings and w).
    sums      of n terms t_i, each formed with r roundings, added in ANY order: at most n - 1 additions touch a term, so
              gamma_{n + r} sum |t_i| -> (n + r) u sum |t_i|.  g_ray: r = 4 for g_pre raw (g y, 1 - y, product, times raw), r = 3
              for g_pre.  The fold over k rays of an image and B branches adds B k terms with their own bars E_i:
              sum E_i + B k u sum |g_ray|.
The bars are derived from the arithmetic, not fitted to a kernel; tests/test_colorcal_host.py holds a plain fp32 torch
evaluation against them and checks that an error of a few bars is seen."""
import torch

from oracle import composite_float64 as c64
from oracle.composite_float64 import SLACK, TINY, U, ULP_EXPF

NR_IMAGES, IDX_FIXED = 4, 0
# the image of every ray: the fixed image (0), images 1 and 2, NO ray of image 3, one ray outside below and one above the tables
IMG_PATTERN = [1, 0, 2, 1, -1, 2, 0, NR_IMAGES, 1, 2, 1]
CONTAINERS = ["rows", "one", "equal32", "gap"]


def _d(t):
    return t.detach().cpu().double()


def container(name):
    """rows    : compacted, rays of 0, 1, 15, 16, 17, 31, 32, 33, 64, 3 and 0 samples: every border of a 16-lane row, M = 212 is
                 no multiple of 64, the first and the last ray are empty
       one     : one ray of one sample
       equal32 : 5 rays of 32 samples in the equal-count form (implicit ranges, start_end is not read)
       gap     : rays of 5, 20 and 7 samples at 0, 9 and 40 of a pool of 50: slots 5-8, 29-39 and 47-49 belong to no ray"""
    equal, fixed = False, 0
    if name == "rows":
        counts = torch.tensor([0, 1, 15, 16, 17, 31, 32, 33, 64, 3, 0])
        starts = torch.cumsum(counts, 0) - counts
        M = int(counts.sum())
    elif name == "one":
        counts, starts, M = torch.tensor([1]), torch.tensor([0]), 1
    elif name.startswith("equal"):
        fixed = int(name[5:])
        counts = torch.full((5,), fixed)
        starts = torch.cumsum(counts, 0) - counts
        equal, M = True, 5 * fixed
    elif name == "gap":
        counts, starts, M = torch.tensor([5, 20, 7]), torch.tensor([0, 9, 40]), 50
    else:
        raise ValueError(name)
    R = len(counts)
    ray_of = torch.full((M,), -1, dtype=torch.int64)
    for r in range(R):
        ray_of[int(starts[r]):int(starts[r] + counts[r])] = r
    return dict(name=name, counts=counts, start_end=torch.stack([starts, starts + counts], 1).to(torch.int32), M=M, R=R, equal=equal,
                fixed=fixed, ray_of=ray_of, img_idx=torch.tensor(IMG_PATTERN[:R], dtype=torch.int32))


def family(c, seed=0, zero_tables=False):
    """-> raw_fm [3, M] in +-6, g_rgb [M, 3], weight_delta and bias [I, 3] of order 0.3"""
    g = torch.Generator().manual_seed(4100 + seed)
    raw_fm = torch.rand(3, c["M"], generator=g) * 12.0 - 6.0
    g_rgb = torch.randn(c["M"], 3, generator=g)
    wd, bias = torch.randn(NR_IMAGES, 3, generator=g) * 0.3, torch.randn(NR_IMAGES, 3, generator=g) * 0.3
    if zero_tables:
        wd, bias = torch.zeros_like(wd), torch.zeros_like(bias)
    return raw_fm, g_rgb, wd, bias


def _per_sample(c, img_idx, wd, bias, idx_fixed):
    """-> owned [M], learned [M] (the tables are read), w [M, 3], b [M, 3]"""
    ray_of = c["ray_of"]
    owned = ray_of >= 0
    img = img_idx.long()[ray_of.clamp_min(0)]
    learned = owned & (img >= 0) & (img < wd.shape[0]) & (img != idx_fixed)
    at = img.clamp(0, wd.shape[0] - 1)
    one, zero = torch.ones(len(ray_of), 3, dtype=torch.float64), torch.zeros(len(ray_of), 3, dtype=torch.float64)
    w = torch.where(learned[:, None], 1.0 + _d(wd)[at], one)
    b = torch.where(learned[:, None], _d(bias)[at], zero)
    return owned, learned, w, b


def forward(c, raw_fm, img_idx, wd, bias, idx_fixed=IDX_FIXED):
    """-> (rgb [M, 3], bar): 0 with bar 0 on slots no ray owns"""
    owned, learned, w, b = _per_sample(c, img_idx, wd, bias, idx_fixed)
    raw = _d(raw_fm).t()
    z = raw * w + b
    E_z = torch.where(learned[:, None], (2 * (raw * w).abs() + z.abs()) * U, torch.zeros_like(z))
    s, _, E = c64._sigmoid(z, E_z, ULP_EXPF)
    k = owned[:, None].double()
    return s * k, E * SLACK * k


def backward(c, g_rgb, rgb, raw_fm, img_idx, wd, bias, idx_fixed=IDX_FIXED, rgb_bar=None):
    """rgb: what the backward is handed (any dtype, taken exactly) -> dict name -> (value, bar): g_raw_fm [3, M], g_ray [R, 6].
    rgb_bar: rgb is the float64 VALUE of the forward and the backward under test starts from an fp32 rgb within rgb_bar of it
    (a forward and a backward held together): y (1 - y) moves by |1 - 2 y| rgb_bar <= rgb_bar, so g_pre by |g_rgb| rgb_bar, which
    every bar below then carries (times |w|, times |raw|, summed)."""
    owned, learned, w, b = _per_sample(c, img_idx, wd, bias, idx_fixed)
    k = owned[:, None].double()
    raw, g, y = _d(raw_fm).t(), _d(g_rgb), _d(rgb)
    g_pre = g * y * (1.0 - y) * k
    g_raw = g_pre * w
    E_in = torch.zeros_like(g_pre) if rgb_bar is None else g.abs() * _d(rgb_bar) * k * SLACK
    out = {"g_raw_fm": (g_raw.t().contiguous(), (5 * U * SLACK * g_raw.abs() + E_in * w.abs() + TINY * k).t().contiguous())}
    R = c["R"]
    val, mag = torch.zeros(R, 6, dtype=torch.float64), torch.zeros(R, 6, dtype=torch.float64)
    lk = learned[:, None].double()
    terms = torch.cat([g_pre * raw, g_pre], 1) * lk                  # [M, 6]
    at = c["ray_of"].clamp_min(0)
    val.index_add_(0, at, terms)
    mag.index_add_(0, at, terms.abs())
    n = c["counts"].double()[:, None]
    r = torch.tensor([4.0, 4.0, 4.0, 3.0, 3.0, 3.0], dtype=torch.float64)[None, :]
    carried = torch.zeros(R, 6, dtype=torch.float64).index_add_(0, at, torch.cat([E_in * raw.abs(), E_in], 1) * lk)
    out["g_ray"] = (val, (n + r) * U * SLACK * mag + carried + n * TINY)
    return out


def fold(img_idx, branches, idx_fixed=IDX_FIXED, nr_images=NR_IMAGES):
    """branches: the (value, bar) pairs of g_ray of one or two branches -> dict: g_weight_delta [I, 3], g_bias [I, 3] as (value, bar)"""
    img = img_idx.long()
    val, bar = torch.zeros(nr_images, 6, dtype=torch.float64), torch.zeros(nr_images, 6, dtype=torch.float64)
    B = len(branches)
    for i in range(nr_images):
        rows = img == i
        k = int(rows.sum())
        if i == idx_fixed or k == 0:
            continue
        for v, e in branches:
            val[i] += v[rows].sum(0)
            bar[i] += e[rows].sum(0) + B * k * U * SLACK * v[rows].abs().sum(0) + k * TINY
    return {"g_weight_delta": (val[:, :3].contiguous(), bar[:, :3].contiguous()), "g_bias": (val[:, 3:].contiguous(), bar[:, 3:].contiguous())}
