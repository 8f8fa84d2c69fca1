"""GPU: EVERY ENTRY of every output of csrc/encode.hip against float64, on every kernel path, with a bar that is DERIVED.

Reference: oracle/encode_float64.py -- the simplex (rows, fp32 barycentrics, ranks) from the fp32 restatement, which the kernels
reproduce bit for bit, everything after it in float64 on the GPU without autograd; each entry comes with the sum of the
absolute values of its finest-grain terms and their number m.  Bar of every comparison in this file (no other tolerance):

    |kernel - float64| <= (m + r) u sum|t| + m 2^-126,      u = 2^-24

(m - 1) u sum|t| bounds ANY order of the fp32 additions; r is the number of roundings the kernel spends on forming one term,
counted from its expressions at the constants R_* below.  A row with 1e5 contributions has a wide bar: the NEEDLE cases (an
upstream gradient that is zero except on a few dozen samples on both sides of every tile / super-tile border) keep m small, so
that one lost contribution is far above it.  The worst error / bar of each comparison is printed (run with -s).

Paths are asserted through psdf_last_path(0) where the library reports one (1 plain lattice kernel, 2 queue + reduce, 3
position kernel alone); the queue-full fallback is proved from the tail counters of a workspace the test supplies itself
(`queue_plan` below is an independent restatement of queue_plan() in csrc/encode_plan.h, pinned to
psdf_encode_backward_workspace_bytes here and, on the CPU, to a recorded grid by tests/test_encode_host_plan.py).

Cases the library cannot be asked to confirm from outside (written here so that nobody assumes more): which of the slab / float-
atomic forms of the position kernel ran (decided by size and capture state inside launch_bwd_pos: the sizes below are chosen
from its rules -- >= 2 level groups and <= 256 MiB of slabs for the slab form), and whether a LevelPlan deal differed from equal
shares (the deal is read back; its effect on the numbers is what is checked).
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import encode_float64 as e64
from oracle import permuto_oracle as po

pytestmark = pytest.mark.gpu

INST = [(3, 2), (4, 2), (2, 2), (3, 4)]
LAYOUT = {(3, 2): 1, (4, 2): 2, (2, 2): 1, (3, 4): 2}     # both concatenation layouts are met (padded: 1, exactly P channels: 2)

# r, counted from the kernels' expressions (csrc/encode.hip):
R_FWD = 2    # encode_fwd_kernel: `bw = bary * w`, `fv * bw`                                   (concatenated: `pos * scaling`, 1)
R_LAT = 2    # encode_bwd_kernel: `bw = bary * w`, `g * bw`; cache / queue / reduce / DPP combine only add (the combine's fma
#              multiplies by exactly 1 or 0)
R_POS = 6    # `lattice * w`, `* g`, `(a - b) * invp` (the difference is a sum; the product rounds once, and invp = 1.0f / (P+1) is
#              itself rounded for P + 1 = 3, 5: one more), `dE * (float)(i + 1)`, `acc * sfl`     (concatenated: `g * scaling`, 1)
R_DBL = 6    # `u * sfl`, `us * (float)(k + 1)`, `aE * invp` (product + the constant, as above), `q * w`, `qw * g` or `qw * lattice`
#              (the direct gradient riding along costs `bary * w`, `g2 * bw2`: 2)


def _lib():
    from permuto_sdf_amd import _lib as L
    return L


def last_path():
    fn = _lib().lib().psdf_last_path
    fn.restype = ctypes.c_int
    return int(fn(ctypes.c_int(0)))


def workspace_bytes(s, N):
    fn = _lib().lib().psdf_encode_backward_workspace_bytes
    fn.restype = ctypes.c_int64
    L = _lib()
    return int(fn(L.c_i(s.P), L.c_i(s.F), L.c_l(N), L.c_i(s.L), L.c_i(s.T)))


def queue_plan(P, F, N, L, T):
    """mirror of queue_plan() in csrc/encode_plan.h (default environment): None = the plain path runs"""
    if N < (1 << 13):
        return None
    base = 14 if F <= 2 else 13
    shift = base - 1
    while shift < base and ((T + (1 << shift) - 1) >> shift) > 64:
        shift += 1
    np_ = (T + (1 << shift) - 1) >> shift
    if np_ > 64:
        return None
    c = (P + 1) * N
    cap = c // np_ + (c // np_) // 4 + 4096
    al = lambda x: (x + 255) & ~255
    entries = L * np_ * cap
    rows_b, vals_b = al(entries * 2), al(entries * F * 4)
    return {"np": np_, "cap": cap, "shift": shift, "tails_off": rows_b + vals_b, "bytes": rows_b + vals_b + al(L * np_ * 4) + 1024}


class Setup:
    """Parameters of one encoding on the device.  Scales are powers of two (finest ~ 2^-13: scale factors ~ 1e4), so that a point
    with integer elevated coordinates at level ZERO_SHIFT (whose random shift is zero) is a lattice vertex there."""
    ZERO_SHIFT = 1

    def __init__(self, dev, P, F, T, L=None, window="mixed", seed=0, concat=True):
        from permuto_sdf_amd.encoding import _Cfg, scale_factor_tensor
        self.dev, self.P, self.F, self.T = dev, P, F, T
        extra = po.nr_extra_levels(P, F, concat)
        self.L = L = (7 - extra) if L is None else L           # default: L + extra = 7, no multiple of 2, 4 or 8
        self.Lt = L + extra
        step = max(1, round(13 / max(1, L - 1)))
        sl = 2.0 ** -(np.arange(L) * float(step))
        layout = LAYOUT[(P, F)] if concat else None
        self.cfg = _Cfg(P, T, L, F, concat, 1e-3, layout)
        self.mode = int(self.cfg.concat_mode)
        g = torch.Generator().manual_seed(1000 * seed + 10 * P + F)
        self.sf_cpu = scale_factor_tensor(sl, P)
        assert torch.equal(self.sf_cpu, po.scale_factors(sl, P))
        self.sf = self.sf_cpu.to(dev)
        self.lat = (torch.randn(L, T, F, generator=g) * 0.5).to(dev)
        sh = torch.randn(L, P, generator=g) * 10.0
        if L > self.ZERO_SHIFT:
            sh[self.ZERO_SHIFT] = 0.0
        self.sh = sh.to(dev)
        if window == "open":
            w = torch.ones(L)
        elif window == "c2f":                                   # coarse-to-fine: open, fractional, then closed levels
            w = po.coarse2fine_window(0.55, L)
            assert float(w[-1]) == 0.0 and float(w[0]) == 1.0
        else:                                                   # open, fractional, CLOSED (level 2), open, fractional, ...
            w = torch.tensor(([1.0, 0.5, 0.0, 1.0, 0.25, 0.75] * 4)[:L])
        self.win = w.to(dev)
        self.C = self.cfg.channels
        self.gen = g

    def points(self, kind, N):
        g, P = self.gen, self.P
        if kind == "uniform":
            p = torch.rand(N, P, generator=g) - 0.5
        elif kind == "rays":                                    # consecutive points = consecutive samples of a ray
            R = (N + 95) // 96
            o = torch.rand(R, P, generator=g) - 0.5
            d = torch.nn.functional.normalize(torch.randn(R, P, generator=g), dim=1)
            t = torch.linspace(-0.3, 0.3, 96)
            p = (o[:, None, :] + t[None, :, None] * d[:, None, :]).reshape(-1, P)[:N]
        elif kind == "identical":
            p = (torch.rand(1, P, generator=g) - 0.5).repeat(N, 1)
        elif kind == "vertices":   # integer and half-integer scaled coordinates at the zero-shift level: lattice vertices and faces
            k = torch.randint(-6, 7, (N, P), generator=g).float() * 0.5         # (rank ties, zero barycentrics)
            p = k / self.sf_cpu[min(self.ZERO_SHIFT, self.L - 1)]
        elif kind == "big":
            p = (torch.rand(N, P, generator=g) * 2 - 1) * 1e3
        elif kind == "hard":       # all of them in one batch; the first sample is a lattice vertex
            parts = [self.points("vertices", 96), self.points("big", 96), self.points("identical", 100),
                     self.points("rays", max(1, N // 3)), self.points("uniform", N)]
            p = torch.cat(parts)[:N]
        else:
            raise ValueError(kind)
        return p.contiguous().to(self.dev)

    def grad(self, N, kind="dense", channels=None):
        """upstream gradient [N, C]; 'needle': zero except on samples at the batch ends and on both sides of tile (256) and
        super-tile (512) borders; channels: a slice outside of which it is zero (level isolation)"""
        g = torch.randn(N, self.C, generator=self.gen)
        if kind == "needle":
            keep = torch.zeros(N, dtype=torch.bool)
            keep[needles(N)] = True
            g[~keep] = 0.0
        if channels is not None:
            m = torch.zeros(self.C, dtype=torch.bool)
            m[channels] = True
            g[:, ~m] = 0.0
        return g.to(self.dev)

    def evaluator(self, pts, cache=True):
        return e64.Encoding64(pts, self.lat, self.sf, self.sh, self.win, self.mode, 1e-3, cache=cache)


def needles(N):
    s = {0, N - 1}
    for b in (256, 512):
        for k in (1, 2, 3, (N // b) // 2, N // b - 1, N // b):
            for d in (-1, 0):
                s.add(k * b + d)
    return sorted(i for i in s if 0 <= i < N)


def fm(g):
    return g.t().contiguous()


def check(tag, got, ref, r, prefill=None):
    """per entry; returns the worst error / bar.  An entry without terms (bar 0) must be exactly zero."""
    val, mag, cnt = ref
    if prefill is not None:                         # a running sum: the prefill is one more term
        val, mag, cnt = val + prefill.double(), mag + prefill.double().abs(), cnt + 1
    assert got.shape == val.shape, (tag, got.shape, val.shape)
    assert bool(torch.isfinite(got).all()), tag + ": non-finite output"
    bar = e64.error_bar(mag, cnt, r)
    err = (got.double() - val).abs()
    q = torch.where(bar > 0, err / bar.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    worst = float(q.max())
    at = np.unravel_index(int(q.argmax()), tuple(q.shape))
    print("    [err/bar] %-62s %.3f   (max m %d)" % (tag, worst, int(cnt.max())))
    assert worst <= 1.0, "%s: error / bar = %.4g at %s: got %r, float64 %r, terms %d, sum|t| %.6g" % (
        tag, worst, at, float(got[at]), float(val[at]), int(cnt.expand_as(val)[at]), float(mag[at]))
    return worst


def backward(s, pts, g, gl, gp, ws=True):
    """ws=True: psdf_encode_backward_ws with the workspace the plan asks for (queue path from 2^13 points on); False: without"""
    from permuto_sdf_amd.encoding import _head, _tail, encode_backward_raw
    L = _lib()
    if ws:
        encode_backward_raw(s.cfg, pts, s.lat, s.sf, s.sh, s.win, fm(g), gl, gp)
    else:
        L.call("psdf_encode_backward", *_head(s.cfg, pts.shape[0]), L.ptr(pts), L.ptr(s.lat), L.ptr(s.sf), L.ptr(s.sh), L.ptr(s.win),
               *_tail(s.cfg), L.ptr(fm(g)), L.ptr(gl), L.ptr(gp), L.stream())
    torch.cuda.synchronize()
    return last_path()


def tag_of(s, N, what):
    return "(%d,%d) T %d L %d N %d %s" % (s.P, s.F, s.T, s.L, N, what)


# ================================================================================================ forward
@pytest.mark.parametrize("P,F", INST)
def test_forward_plain_masked_marking(dev, P, F):
    from permuto_sdf_amd.encoding import encode_forward_raw
    N = 2 ** 13 + 1
    s = Setup(dev, P, F, 2 ** 14 + 37)
    pts = s.points("hard", N)
    ev = s.evaluator(pts)
    ref = ev.forward()
    out = torch.full((s.C, N), float("nan"), device=dev)
    encode_forward_raw(s.cfg, pts, s.lat, s.sf, s.sh, s.win, out=out)
    check(tag_of(s, N, "forward plain"), out.t(), ref, R_FWD)
    assert float(out[2 * F:3 * F].abs().max()) == 0.0                       # the closed level
    # masked: masked columns keep a sentinel bit for bit
    skip = (torch.rand(N, generator=s.gen) < 0.3).to(torch.uint8).to(dev)
    sentinel = torch.randn(s.C, N, generator=s.gen).to(dev)
    out = sentinel.clone()
    encode_forward_raw(s.cfg, pts, s.lat, s.sf, s.sh, s.win, skip=skip, out=out)
    keep = skip.bool()
    assert torch.equal(out[:, keep].view(torch.int32), sentinel[:, keep].view(torch.int32))
    live = ~keep
    check(tag_of(s, N, "forward masked"), out[:, live].t(), tuple(x[live] for x in ref), R_FWD)
    # marking: the touched map is exactly the set of blocks the open levels read
    for b in (0, 7, 20):                                                    # 2^20 > T: one block per level
        nb = (s.T + (1 << b) - 1) >> b
        touched = torch.zeros(s.L, nb, dtype=torch.uint8, device=dev)
        out = torch.full((s.C, N), float("nan"), device=dev)
        encode_forward_raw(s.cfg, pts, s.lat, s.sf, s.sh, s.win, out=out, touched=touched, block_rows_log2=b)
        want = torch.zeros_like(touched)
        for l in ev.open_levels():
            want[l, (ev.level(l)[0] >> b).reshape(-1)] = 1
        assert torch.equal(touched, want), (b, int(touched.sum()), int(want.sum()))
        assert int(want[2].sum()) == 0 and int(want.sum()) > 0              # a closed level marks nothing
        check(tag_of(s, N, "forward marking 2^%d" % b), out.t(), ref, R_FWD)


# ============================================================================= backward: sizes round the thresholds
@pytest.mark.parametrize("N", [1, 255, 257, 2 ** 13 - 1, 2 ** 13, 2 ** 13 + 1])
@pytest.mark.parametrize("P,F", INST)
def test_backward_at_the_size_thresholds(dev, P, F, N):
    T = 5000 if N < 8000 else (2 ** 14 if (P, F) == (3, 2) else 2 ** 14 + 4099)
    s = Setup(dev, P, F, T)
    pts = s.points("hard", N)
    ev = s.evaluator(pts)
    queue = queue_plan(P, F, N, s.L, T) is not None
    assert queue == (N >= 2 ** 13) and (workspace_bytes(s, N) > 0) == queue
    # lattice + positions in one call, with workspace, needles
    g = s.grad(N, "needle")
    gl, gp = torch.zeros_like(s.lat), torch.zeros_like(pts)
    assert backward(s, pts, g, gl, gp) == (2 if queue else 1)
    check(tag_of(s, N, "lattice (ws, needles)"), gl, ev.lattice_grad(g), R_LAT)
    check(tag_of(s, N, "position (ws, needles)"), gp, ev.position_grad(g), R_POS)
    # the same without workspace: plain kernel, fused position branch, dense
    g = s.grad(N)
    gl, gp = torch.zeros_like(s.lat), torch.zeros_like(pts)
    assert backward(s, pts, g, gl, gp, ws=False) == 1
    check(tag_of(s, N, "lattice (plain, dense)"), gl, ev.lattice_grad(g), R_LAT)
    check(tag_of(s, N, "position (plain fused, dense)"), gp, ev.position_grad(g), R_POS)
    # each gradient alone
    gl = torch.zeros_like(s.lat)
    assert backward(s, pts, g, gl, None) == (2 if queue else 1)
    check(tag_of(s, N, "lattice alone (ws, dense)"), gl, ev.lattice_grad(g), R_LAT)
    gp = torch.zeros_like(pts)
    assert backward(s, pts, g, None, gp) == 3
    check(tag_of(s, N, "position alone (dense)"), gp, ev.position_grad(g), R_POS)


# ============================================================================================= level isolation
@pytest.mark.parametrize("N", [3001, 2 ** 17])          # position kernel: 8 levels per thread / 2 per thread (slab form)
@pytest.mark.parametrize("P,F", INST)
def test_one_level_alone_carries_gradient(dev, P, F, N):
    """L + extra = 7: the last level group of the position kernel is partly filled in every form (2, 4, 8 levels per thread).
    Every level in turn, then the concatenated-point channels alone."""
    s = Setup(dev, P, F, 2 ** 14 + 4099, window="open")
    pts = s.points("rays", N)
    ev = s.evaluator(pts)
    blocks = [slice(l * F, (l + 1) * F) for l in range(s.L)] + [slice(s.L * F, s.C)]
    for i, ch in enumerate(blocks):
        g = s.grad(N, "needle" if i % 2 else "dense", channels=ch)
        gl, gp = torch.zeros_like(s.lat), torch.zeros_like(pts)
        assert backward(s, pts, g, gl, gp) == (2 if N >= 2 ** 13 else 1)
        name = "level %d alone" % i if i < s.L else "point channels alone"
        check(tag_of(s, N, "lattice, " + name), gl, ev.lattice_grad(g), R_LAT)
        check(tag_of(s, N, "position, " + name), gp, ev.position_grad(g), R_POS)
        others = [l for l in range(s.L) if l != i]
        assert float(gl[others].abs().max()) == 0.0


# ================================================================================================ point sets
@pytest.mark.parametrize("kind", ["identical", "vertices", "big", "uniform"])
@pytest.mark.parametrize("P,F", INST)
def test_point_sets(dev, P, F, kind):
    """all points identical (every contribution of a level on P + 1 rows), lattice vertices and faces, |coordinate| up to 1e3,
    unordered points: backward through the queue path and double backward, mixed window."""
    from permuto_sdf_amd.encoding import encode_double_backward_raw
    N = 20001
    s = Setup(dev, P, F, 2 ** 14 + 4099)
    pts = s.points(kind, N)
    ev = s.evaluator(pts)
    g = s.grad(N)
    gl, gp = torch.zeros_like(s.lat), torch.zeros_like(pts)
    assert backward(s, pts, g, gl, gp) == 2
    check(tag_of(s, N, "lattice, %s points" % kind), gl, ev.lattice_grad(g), R_LAT)
    check(tag_of(s, N, "position, %s points" % kind), gp, ev.position_grad(g), R_POS)
    u = torch.randn(N, P, generator=s.gen).to(dev)
    gl, gg = torch.zeros_like(s.lat), torch.full((s.C, N), float("nan"), device=dev)
    encode_double_backward_raw(s.cfg, pts, s.lat, s.sf, s.sh, s.win, u, fm(g), gl, gg)
    check(tag_of(s, N, "dbl scattered, %s points" % kind), gl, ev.double_backward_scattered(u, g), R_DBL)
    check(tag_of(s, N, "dbl gathered, %s points" % kind), gg.t(), ev.double_backward_gathered(u), R_DBL)


# ================================================================================== large batches, table sizes
TABLES = [(3, 2, T) for T in (5000, 2 ** 14, 2 ** 18, 2 ** 18 + 4099, 2 ** 19, 2 ** 22)] + \
         [(4, 2, 2 ** 18 + 4099), (2, 2, 2 ** 18 + 4099), (3, 4, 2 ** 18 + 4099)]
PARTITIONS = {(2, 5000): 1, (2, 2 ** 14): 2, (2, 2 ** 18): 32, (2, 2 ** 18 + 4099): 33, (2, 2 ** 19): 64, (2, 2 ** 22): None,
              (4, 2 ** 18 + 4099): 33}      # (features, rows) -> partitions; 33: the last one is only partly inside the table;
#                                             F = 4 has 8192-row slices at this size (4096 would need 65 partitions)


@pytest.mark.parametrize("P,F,T", TABLES)
def test_large_batch_over_table_sizes(dev, P, F, T):
    """600 001 points (no multiple of the 512-point super-tile): one partition, 64 partitions, a last partition partly outside
    the table, and a table the plan refuses (the plain path must run).  Lattice + positions in one call (the position kernel's
    2-levels-per-thread slab form), then the lattice alone (the launch with a LevelPlan) with needles."""
    N = 600_001
    s = Setup(dev, P, F, T, L=4)
    plan = queue_plan(P, F, N, s.L, T)
    assert (plan["np"] if plan else None) == PARTITIONS[(F, T)]
    assert workspace_bytes(s, N) == (plan["bytes"] if plan else 0)
    pts = s.points("hard", N)
    ev = s.evaluator(pts)
    g = s.grad(N)
    gl, gp = torch.zeros_like(s.lat), torch.zeros_like(pts)
    assert backward(s, pts, g, gl, gp) == (2 if plan else 1)
    check(tag_of(s, N, "lattice (dense)"), gl, ev.lattice_grad(g), R_LAT)
    check(tag_of(s, N, "position (dense)"), gp, ev.position_grad(g), R_POS)
    g = s.grad(N, "needle")
    gl = torch.zeros_like(s.lat)
    assert backward(s, pts, g, gl, None) == (2 if plan else 1)
    check(tag_of(s, N, "lattice alone (needles)"), gl, ev.lattice_grad(g), R_LAT)


@pytest.mark.parametrize("P,F", INST)
def test_lattice_gradient_under_a_level_plan_deal(dev, P, F):
    """From 2^18 points on, lattice-only launches deal one resident round of workgroups over the levels from the durations of the
    previous call: three calls, float64 check on the last."""
    N = 300_001
    s = Setup(dev, P, F, 2 ** 18 if (P, F) == (3, 2) else 2 ** 16 + 4099, L=6, window="c2f", concat=False)
    pts = s.points("rays", N)
    ev = s.evaluator(pts)
    for call in range(3):
        g = s.grad(N, "needle" if call == 2 else "dense")
        gl = torch.zeros_like(s.lat)
        assert backward(s, pts, g, gl, None) == 2
    counts = (ctypes.c_int * 64)()
    n = _lib().lib().psdf_encode_backward_level_shares(counts, 64)
    assert n == s.L and all(c >= 1 for c in counts[:n]), list(counts[:n])
    print("    deal over the levels at the last call:", list(counts[:n]))
    check(tag_of(s, N, "lattice under a level plan (needles)"), gl, ev.lattice_grad(g), R_LAT)
    closed = [l for l in range(s.L) if float(s.win[l]) == 0.0]
    assert closed and float(gl[closed].abs().max()) == 0.0
    # the double backward's queue form deals its round the same way (its own state): three calls, check the last
    from permuto_sdf_amd.encoding import encode_double_backward_raw
    u = torch.randn(N, P, generator=s.gen).to(dev)
    g2 = s.grad(N, "needle")
    for call in range(3):
        gl, gg = torch.zeros_like(s.lat), torch.full((s.C, N), float("nan"), device=dev)
        encode_double_backward_raw(s.cfg, pts, s.lat, s.sf, s.sh, s.win, u, fm(g), gl, gg, fm(g2))
    torch.cuda.synchronize()
    check(tag_of(s, N, "dbl scattered + direct under a level plan"), gl, ev.double_backward_scattered(u, g, g2), R_DBL)
    check(tag_of(s, N, "dbl gathered under a level plan"), gg.t(), ev.double_backward_gathered(u), R_DBL)
    assert float(gl[closed].abs().max()) == 0.0 and float(gg[closed[0] * F:].abs().max()) == 0.0


# ========================================================================================== queue-full fallback
@pytest.mark.parametrize("P,F", [(3, 2), (3, 4)])
def test_queue_full_fallback(dev, P, F):
    """The first 2^17 points uniform (every workgroup's first super-tile sees no re-use at the fine levels and votes its cache
    off; one resident round is at most 5 x 256 / L workgroups per level, 512 points each, so every first super-tile lies in this
    part), the rest cycling through three fixed points A, B, C, A, ... (no two neighbours equal: the run combine merges nothing).
    ~1.9 M contributions of a fine level go to at most 12 rows: their partitions' queues (capacity contrib / np * 1.25 + 4096)
    overflow and the remainder takes the float-atomic fallback.  The overflow is PROVED from the tail counters."""
    from permuto_sdf_amd.encoding import _head, _tail
    L = _lib()
    N, T = 600_001, 2 ** 18
    s = Setup(dev, P, F, T, L=8, window="open", concat=False)
    plan = queue_plan(P, F, N, s.L, T)
    assert (plan["np"], plan["cap"]) == {(3, 2): (32, 97846), (3, 4): (64, 50971)}[(P, F)]
    assert workspace_bytes(s, N) == plan["bytes"]
    head = s.points("uniform", 2 ** 17)
    abc = s.points("uniform", 3)
    pts = torch.cat([head, abc.repeat((N - 2 ** 17 + 2) // 3, 1)[:N - 2 ** 17]]).contiguous()
    assert pts.shape[0] == N and not bool((pts[2 ** 17 + 1:] == pts[2 ** 17:-1]).all(1).any())
    ev = s.evaluator(pts)
    g = s.grad(N)
    ws = torch.empty(plan["bytes"], dtype=torch.uint8, device=dev)
    gl = torch.zeros_like(s.lat)
    L.call("psdf_encode_backward_ws", *_head(s.cfg, N), L.ptr(pts), L.ptr(s.lat), L.ptr(s.sf), L.ptr(s.sh), L.ptr(s.win),
           *_tail(s.cfg), L.ptr(fm(g)), L.ptr(gl), None, L.ptr(ws), L.c_l(plan["bytes"]), L.stream())
    torch.cuda.synchronize()
    assert last_path() == 2
    tails = ws[plan["tails_off"]:plan["tails_off"] + s.L * plan["np"] * 4].view(torch.int32).view(s.L, plan["np"]).cpu()
    over = (tails.long() - plan["cap"]).clamp_min(0)
    print("    queue-full fallback: %d contributions of %d (level, partition) queues went past the capacity %d; per level %s"
          % (int(over.sum()), int((over > 0).sum()), plan["cap"], over.sum(1).tolist()))
    assert int(tails.sum()) > 0 and int(over.sum()) > 100_000, "the fallback did not run: this case checks nothing"
    check(tag_of(s, N, "lattice, queue-full fallback"), gl, ev.lattice_grad(g), R_LAT)


# =================================================================================================== running sum
@pytest.mark.parametrize("N", [3001, 20001, 2 ** 17])      # plain / queue + 8-level position kernel / queue + slab form
@pytest.mark.parametrize("P,F", INST)
def test_gradients_add_into_a_running_sum(dev, P, F, N):
    s = Setup(dev, P, F, 2 ** 14 + 4099)
    pts = s.points("hard", N)
    ev = s.evaluator(pts)
    g = s.grad(N, "needle")
    pre_l = torch.randn(s.lat.shape, generator=s.gen).to(dev)
    pre_p = torch.randn(N, P, generator=s.gen).to(dev)
    gl, gp = pre_l.clone(), pre_p.clone()
    assert backward(s, pts, g, gl, gp) == (2 if N >= 2 ** 13 else 1)
    check(tag_of(s, N, "lattice += (with positions)"), gl, ev.lattice_grad(g), R_LAT, prefill=pre_l)
    check(tag_of(s, N, "position += (with lattice)"), gp, ev.position_grad(g), R_POS, prefill=pre_p)
    gl = pre_l.clone()
    backward(s, pts, g, gl, None)
    check(tag_of(s, N, "lattice += (alone)"), gl, ev.lattice_grad(g), R_LAT, prefill=pre_l)
    gp = pre_p.clone()
    assert backward(s, pts, g, None, gp) == 3
    check(tag_of(s, N, "position += (alone)"), gp, ev.position_grad(g), R_POS, prefill=pre_p)


@pytest.mark.parametrize("P,F", INST)
def test_position_running_sum_slab_form_of_the_eight_level_kernel(dev, P, F):
    """3001 points, L + extra = 12 levels: two level groups of the 8-levels-per-thread kernel (the first full -- its eighth level is
    open --, the second partly filled) -> slab form"""
    N = 3001
    s = Setup(dev, P, F, 5000, L=12 - po.nr_extra_levels(P, F, True))
    assert s.Lt == 12 and float(s.win[7]) != 0.0
    pts = s.points("hard", N)
    g = s.grad(N)
    pre = torch.randn(N, P, generator=s.gen).to(dev)
    gp = pre.clone()
    assert backward(s, pts, g, None, gp) == 3
    check(tag_of(s, N, "position += (two groups of 8)"), gp, s.evaluator(pts).position_grad(g), R_POS, prefill=pre)


# ===================================================================================== position gradient alone
@pytest.mark.parametrize("N", [3001, 2 ** 17 + 1])
@pytest.mark.parametrize("P,F", INST)
def test_position_gradient_alone_and_masked(dev, P, F, N):
    from permuto_sdf_amd.encoding import _head, _tail
    L = _lib()
    s = Setup(dev, P, F, 2 ** 14 + 4099, window="c2f")
    pts = s.points("hard", N)
    ev = s.evaluator(pts)
    g = s.grad(N)
    ref = ev.position_grad(g)
    gp = torch.zeros_like(pts)
    assert backward(s, pts, g, None, gp) == 3
    check(tag_of(s, N, "position alone, coarse-to-fine window"), gp, ref, R_POS)
    # masked rows keep their contents bit for bit, the others accumulate
    skip = (torch.rand(N, generator=s.gen) < 0.3).to(torch.uint8).to(dev)
    pre = torch.randn(N, P, generator=s.gen).to(dev)
    gp = pre.clone()
    L.call("psdf_encode_backward_positions_masked", *_head(s.cfg, N), L.ptr(pts), L.ptr(s.lat), L.ptr(s.sf), L.ptr(s.sh),
           L.ptr(s.win), *_tail(s.cfg), L.ptr(fm(g)), L.ptr(skip), L.ptr(gp), L.stream())
    torch.cuda.synchronize()
    keep = skip.bool()
    assert torch.equal(gp[keep].view(torch.int32), pre[keep].view(torch.int32))
    live = ~keep
    check(tag_of(s, N, "position masked"), gp[live], tuple(x[live] for x in ref), R_POS, prefill=pre[live])


def test_position_gradient_two_million_points_float_atomic_form(dev):
    """2^21 points x (24 + 2) levels: 13 level groups x 2^21 x 3 floats = 327 MB of slabs, above the 256-MiB cap of
    launch_bwd_pos_lpb: the float-atomic form of the 2-levels-per-thread kernel."""
    N = 2 ** 21
    s = Setup(dev, 3, 2, 2 ** 18, L=24, window="open")
    pts = s.points("rays", N)
    g = s.grad(N)
    gp = torch.zeros_like(pts)
    assert backward(s, pts, g, None, gp) == 3
    check(tag_of(s, N, "position alone, float-atomic form"), gp, s.evaluator(pts, cache=False).position_grad(g), R_POS)


@pytest.mark.parametrize("P,F", INST)
def test_position_gradient_captured_in_a_graph(dev, P, F):
    """Captured in a single-stream graph and replayed once: 4 levels per thread, float-atomic form (no stream-ordered scratch
    while capturing)."""
    from permuto_sdf_amd.encoding import _head, _tail
    L = _lib()
    N = 5001
    s = Setup(dev, P, F, 5000)
    pts = s.points("hard", N)
    g = s.grad(N)
    g_fm = fm(g)
    gp = torch.zeros_like(pts)

    def launch():
        L.call("psdf_encode_backward", *_head(s.cfg, N), L.ptr(pts), L.ptr(s.lat), L.ptr(s.sf), L.ptr(s.sh), L.ptr(s.win),
               *_tail(s.cfg), L.ptr(g_fm), None, L.ptr(gp), L.stream())

    launch()                                    # outside the capture once (lazy initialisation)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    gp.zero_()
    graph.replay()
    torch.cuda.synchronize()
    check(tag_of(s, N, "position alone, graph replay"), gp, s.evaluator(pts).position_grad(g), R_POS)


# =============================================================================================== double backward
@pytest.mark.parametrize("N", [3001, 2 ** 13 + 1, 40001])          # plain kernels / queue form
@pytest.mark.parametrize("P,F", INST)
def test_double_backward_every_form(dev, P, F, N):
    from permuto_sdf_amd.encoding import _head, _tail, encode_double_backward_raw
    L = _lib()
    s = Setup(dev, P, F, 2 ** 14 + 4099)
    pts = s.points("hard", N)
    ev = s.evaluator(pts)
    u = torch.randn(N, P, generator=s.gen).to(dev)
    g, g2 = s.grad(N, "needle"), s.grad(N, "needle")
    gd = s.grad(N)
    ref_gg = ev.double_backward_gathered(u)
    form = "queue" if N >= 2 ** 13 else "plain"
    # lattice gradient + gathered output (queue form from 2^13 points on)
    gl, gg = torch.zeros_like(s.lat), torch.full((s.C, N), float("nan"), device=dev)
    encode_double_backward_raw(s.cfg, pts, s.lat, s.sf, s.sh, s.win, u, fm(g), gl, gg)
    check(tag_of(s, N, "dbl scattered (%s, needles)" % form), gl, ev.double_backward_scattered(u, g), R_DBL)
    check(tag_of(s, N, "dbl gathered (%s)" % form), gg.t(), ref_gg, R_DBL)
    assert float(gg[2 * F:3 * F].abs().max()) == 0.0                     # the closed level: written as 0
    # the plain kernel (no workspace), dense; its gathered output is bit-identical to the queue form's
    gl_a, gg_a = torch.zeros_like(s.lat), torch.full((s.C, N), float("nan"), device=dev)
    L.call("psdf_encode_double_backward", *_head(s.cfg, N), L.ptr(pts), L.ptr(s.lat), L.ptr(s.sf), L.ptr(s.sh), L.ptr(s.win),
           *_tail(s.cfg), L.ptr(u), L.ptr(fm(gd)), L.ptr(gl_a), L.ptr(gg_a), L.stream())
    torch.cuda.synchronize()
    check(tag_of(s, N, "dbl scattered (plain, dense)"), gl_a, ev.double_backward_scattered(u, gd), R_DBL)
    assert torch.equal(gg_a, gg)
    # without a lattice gradient
    gg_n = torch.full((s.C, N), float("nan"), device=dev)
    encode_double_backward_raw(s.cfg, pts, s.lat, s.sf, s.sh, s.win, u, fm(g), None, gg_n)
    assert torch.equal(gg_n, gg)
    # without the gathered output; then with a direct gradient riding along (prefilled: the scatter adds)
    gl = torch.zeros_like(s.lat)
    encode_double_backward_raw(s.cfg, pts, s.lat, s.sf, s.sh, s.win, u, fm(gd), gl, None)
    check(tag_of(s, N, "dbl scattered (%s, no gathered output)" % form), gl, ev.double_backward_scattered(u, gd), R_DBL)
    pre = torch.randn(s.lat.shape, generator=s.gen).to(dev)
    gl = pre.clone()
    encode_double_backward_raw(s.cfg, pts, s.lat, s.sf, s.sh, s.win, u, fm(g), gl, None, fm(g2))
    check(tag_of(s, N, "dbl scattered + direct (%s, needles)" % form), gl, ev.double_backward_scattered(u, g, g2), R_DBL,
          prefill=pre)
