"""GPU: the way OUT of the binning kernel's LDS scatter cache in queue mode (csrc/encode.hip, cache_drain_once).

A workgroup of encode_bwd_kernel<.., QUEUE = true> that keeps its cache to the end of its walk hands the live entries to the
queues of its level in one reservation round (count, reserve, write); one that votes the cache off after its first super-tile
drains it at once (cache_drain_to_queue).  The library is asked how the workgroups left (psdf_encode_backward_cache_votes, read
from the workspace the test supplies) next to psdf_last_path = 2: the one-round drain must run in every case, and both ways must
be met wherever the shape allows it (see both_ways_out).

Shapes: the smallest at which the drain can go wrong.  The queue path starts at 2^13 points and a super-tile is 512 points: 8192
(16 full super-tiles), 8193 (a super-tile of one point), 8703 (a last super-tile one point short); 4 levels with scales 2^0,
2^-4, 2^-8, 2^-12 -- the coarsest level sends the whole batch to a handful of rows (cache kept), at the finest no two samples share
a row (cache voted off); tables of 2^12 rows (one partition: every drained entry in one queue) and 2^18 rows (32 partitions).

Reference and bars: oracle/encode_float64.py through tests/float64_check.py, every entry of the gradient table against float64 with
the bar test_gpu_encode_float64.py derives, (m + r) u sum|t| + m 2^-126 with its r (R_LAT, R_DBL) -- nothing wider.  A cache
entry that the drain loses or writes twice is the partial sum of up to 512 x (P + 1) contributions of a row: far outside.

The queue-full fallback inside the drain is not met here: the plan (csrc/encode_plan.h) gives every queue room for 1.25 x its
share of ALL contributions and has no switch that makes it smaller; that branch is the same three lines as in queue_push.
"""
import ctypes

import pytest
import torch

from oracle import encode_float64 as e64
from tests.float64_check import check, show
from tests.test_gpu_encode_float64 import R_DBL, R_LAT, Setup, fm, last_path, queue_plan

pytestmark = pytest.mark.gpu

LEVELS = 4


def _lib():
    from permuto_sdf_amd import _lib as L
    return L


def make_points(s, kind, N):
    g, P = s.gen, s.P
    if kind == "one_simplex":        # a cube of side 0.02: inside one simplex of the coarsest level (asserted by the caller), some
        c = torch.rand(1, P, generator=g) - 0.5      # 58 cells wide at the finest
        p = c + (torch.rand(N, P, generator=g) - 0.5) * 0.02
    elif kind == "line":             # consecutive samples of one ray at the benchmark's spacing (a chord of <= 1 in 128 samples)
        o = torch.rand(1, P, generator=g) - 0.5
        d = torch.nn.functional.normalize(torch.randn(1, P, generator=g), dim=1)
        t = (torch.arange(N, dtype=torch.float32) - N / 2) / 128.0
        p = o + t[:, None] * d
    elif kind == "ball":
        u = torch.randn(N, P, generator=g)
        p = u / u.norm(dim=1, keepdim=True) * 0.5 * torch.rand(N, 1, generator=g) ** (1.0 / P)
    else:
        raise ValueError(kind)
    return p.contiguous().to(s.dev)


def votes(s, N, ws, nbytes):
    L = _lib()
    kept, off = (ctypes.c_int * 64)(), (ctypes.c_int * 64)()
    fn = L.lib().psdf_encode_backward_cache_votes
    fn.restype = ctypes.c_int
    n = fn(L.c_i(s.P), L.c_i(s.F), L.c_l(N), L.c_i(s.L), L.c_i(s.T), L.ptr(ws), L.c_l(nbytes), kept, off, L.c_i(64), L.stream())
    assert n == s.L, n
    return list(kept[:n]), list(off[:n])


def lattice_backward(s, pts, g, gl):
    """psdf_encode_backward_ws, lattice gradient alone, with a workspace of the test's own -> (kept, voted off) per level"""
    from permuto_sdf_amd.encoding import _head, _tail
    L = _lib()
    N = pts.shape[0]
    plan = queue_plan(s.P, s.F, N, s.L, s.T)
    ws = torch.empty(plan["bytes"], dtype=torch.uint8, device=s.dev)
    L.call("psdf_encode_backward_ws", *_head(s.cfg, N), L.ptr(pts), L.ptr(s.lat), L.ptr(s.sf), L.ptr(s.sh), L.ptr(s.win),
           *_tail(s.cfg), L.ptr(fm(g)), L.ptr(gl), None, L.ptr(ws), L.c_l(plan["bytes"]), L.stream())
    torch.cuda.synchronize()
    assert last_path() == 2
    return votes(s, N, ws, plan["bytes"])


def double_backward(s, pts, u, g, gl, gg):
    from permuto_sdf_amd.encoding import _head, _tail
    L = _lib()
    N = pts.shape[0]
    plan = queue_plan(s.P, s.F, N, s.L, s.T)
    ws = torch.empty(plan["bytes"], dtype=torch.uint8, device=s.dev)
    L.call("psdf_encode_double_backward_ws", *_head(s.cfg, N), L.ptr(pts), L.ptr(s.lat), L.ptr(s.sf), L.ptr(s.sh), L.ptr(s.win),
           *_tail(s.cfg), L.ptr(u), L.ptr(fm(g)), L.ptr(gl), L.ptr(gg), None, L.ptr(ws), L.c_l(plan["bytes"]), L.stream())
    torch.cuda.synchronize()
    return votes(s, N, ws, plan["bytes"])


def both_ways_out(s, kept, off):
    """The coarsest level keeps its cache (one-round drain) in every case.  That a level votes its cache off is asserted for the
    table of 2^18 rows.  With 2^12 rows no choice of scales can make a full super-tile do so: its 2048 contributions fall on at
    most 4096 rows, and even spread evenly over them by the hash (the finest levels here) about 0.14 - 0.18 of them meet an entry
    of their own row -- above the vote's 1/8; there only a last super-tile of a few points votes off (N = 8193)."""
    print("    caches kept per level %s, voted off %s" % (kept, off))
    closed = [l for l in range(s.L) if float(s.win[l]) == 0.0]
    assert all(kept[l] == 0 and off[l] == 0 for l in closed), (kept, off)
    assert kept[0] > 0, "the coarsest level did not keep its cache: the one-round drain did not run (%r, %r)" % (kept, off)
    if s.T >= 2 ** 18:
        assert sum(off) > 0, "no workgroup voted its cache off (%r, %r)" % (kept, off)


def against_float64(out, name, got, ref, r, prefill=None):
    val, mag, cnt = ref
    if prefill is not None:                                   # a running sum: what was there is one more term
        val, mag, cnt = val + prefill.double(), mag + prefill.double().abs(), cnt + 1
    bar = e64.error_bar(mag, cnt, r)
    check(out, name, got, val.cpu(), bar.expand_as(val).cpu())


@pytest.mark.parametrize("kind", ["one_simplex", "line", "ball"])
@pytest.mark.parametrize("T", [2 ** 12, 2 ** 18])
@pytest.mark.parametrize("N", [8192, 8193, 8703])
def test_drained_cache_against_float64(dev, N, T, kind):
    s = Setup(dev, 3, 2, T, L=LEVELS, window="open", concat=False)
    pts = make_points(s, kind, N)
    ev = s.evaluator(pts)
    if kind == "one_simplex":
        rows = ev.level(0)[0]
        assert bool((rows == rows[:1]).all()), "the cloud crosses a simplex border of the coarsest level"
    g = s.grad(N)
    gl = torch.zeros_like(s.lat)
    kept, off = lattice_backward(s, pts, g, gl)
    both_ways_out(s, kept, off)
    out = []
    against_float64(out, "lattice", gl, ev.lattice_grad(g), R_LAT)
    show("(3,2) T %d N %d %s" % (T, N, kind), out)


def test_closed_level_stays_exactly_zero(dev):
    N, T = 8703, 2 ** 18
    s = Setup(dev, 3, 2, T, L=LEVELS, window="mixed", concat=False)
    assert float(s.win[2]) == 0.0 and float(s.win[0]) != 0.0 and float(s.win[3]) != 0.0
    pts = make_points(s, "line", N)
    g = s.grad(N)
    gl = torch.zeros_like(s.lat)
    kept, off = lattice_backward(s, pts, g, gl)
    both_ways_out(s, kept, off)
    assert float(gl[2].abs().max()) == 0.0
    out = []
    against_float64(out, "lattice", gl, s.evaluator(pts).lattice_grad(g), R_LAT)
    show("closed level", out)


@pytest.mark.parametrize("P,F", [(3, 4), (4, 2)])
def test_other_instantiations(dev, P, F):
    N, T = 8192, 2 ** 18
    s = Setup(dev, P, F, T, L=LEVELS, window="open", concat=False)
    pts = make_points(s, "ball", N)
    g = s.grad(N)
    gl = torch.zeros_like(s.lat)
    kept, off = lattice_backward(s, pts, g, gl)
    both_ways_out(s, kept, off)
    out = []
    against_float64(out, "lattice", gl, s.evaluator(pts).lattice_grad(g), R_LAT)
    show("(%d,%d)" % (P, F), out)


def test_double_backward(dev):
    N, T = 8192, 2 ** 18
    s = Setup(dev, 3, 2, T, L=LEVELS, window="open", concat=False)
    pts = make_points(s, "line", N)
    ev = s.evaluator(pts)
    u = torch.randn(N, 3, generator=s.gen).to(dev)
    g = s.grad(N)
    gl, gg = torch.zeros_like(s.lat), torch.full((s.C, N), float("nan"), device=dev)
    kept, off = double_backward(s, pts, u, g, gl, gg)
    both_ways_out(s, kept, off)
    out = []
    against_float64(out, "scattered", gl, ev.double_backward_scattered(u, g), R_DBL)
    against_float64(out, "gathered", gg.t(), ev.double_backward_gathered(u), R_DBL)
    show("double backward", out)


def test_adds_into_a_table_that_is_not_zero(dev):
    N, T = 8193, 2 ** 18
    s = Setup(dev, 3, 2, T, L=LEVELS, window="open", concat=False)
    pts = make_points(s, "ball", N)
    g = s.grad(N)
    pre = torch.randn(s.lat.shape, generator=s.gen).to(dev)
    gl = pre.clone()
    kept, off = lattice_backward(s, pts, g, gl)
    both_ways_out(s, kept, off)
    out = []
    against_float64(out, "lattice +=", gl, s.evaluator(pts).lattice_grad(g), R_LAT, prefill=pre)
    show("running sum", out)
