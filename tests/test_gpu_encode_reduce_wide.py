"""GPU: the fold loop of encode_bwd_reduce_kernel (csrc/encode.hip) -- four consecutive queue entries per thread, one 8-byte
load of their rows and 16-byte loads of their values, the next group's loads in flight during the adds, every workgroup
starting at another place of its queue -- at the smallest shapes at which it can go wrong.

What the loop adds over its predecessor, and so what can break:
  * groups are 4-entry aligned in the WORKSPACE, while a queue starts at (level * partitions + partition) * capacity entries,
    which need not be a multiple of 4, and holds any number of entries: up to three entries at each end of a queue take a
    scalar form.  Batches of 8192, 8193, 8195 and 12 289 points give queue capacities with every residue mod 4, and fully hashed
    levels give queue lengths with every residue (counted from the tail counters of a workspace the test owns and printed by
    the last test of this file);
  * the walk wraps round the end of the queue, and threads past the last group load it again without adding it: queues shorter
    than one step of the workgroup (2^18 rows: a few hundred entries per queue) and longer than two (2^14 rows) are both met;
  * a thread holds several entries of one row at once, and a row that many threads hit at once falls back to the LDS float
    atomic.  All points equal is the plain form of that case; at these batch sizes the binning kernel's LDS cache absorbs such
    a batch before it reaches a queue (the queued count is printed), so a second case alternates two points chosen so that a
    row of one is kept OUT of the cache by a row of the other (same cache slot): half the batch's contributions to that row
    then sit in one queue, one after the other.  The case asserts that they did.

Reference and bar: oracle/encode_float64.py entry by entry with the bar of tests/test_gpu_encode_float64.py (its `check`, R_LAT),
no other tolerance.  Second reference: the plain path (LDS cache + float atomics) of the same library, computed once for all
cases by ONE child process with PSDF_ENC_QUEUE_MIN_N raised (the switch is read once per process).  Both paths add the SAME
fp32 terms, in different orders; two fp32 sums of m terms in any two orders differ by at most

    2 gamma_(m-1) sum|t^|,   gamma_k = k u / (1 - k u),  u = 2^-24

(Higham, Accuracy and Stability of Numerical Algorithms, eq. 4.4, once per order), t^ the rounded terms: sum|t^| <= (1 + u)^2
sum|t| for R_LAT = 2 roundings per term, plus m 2^-126 per order for terms that underflow.  m = 1: the two paths agree bit for bit.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from oracle import encode_float64 as e64
from tests.test_gpu_encode_float64 import R_LAT, Setup, _lib, check, fm, last_path, queue_plan, tag_of, workspace_bytes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (8192, 8193, 8195, 12289)
TABLES = (2 ** 14, 2 ** 15 + 8, 2 ** 18)       # F = 2: 2, 5 (the last one 8 rows) and 32 partitions; F = 4: 4, 9 and 64
# (name, F, T, L, N, points, window).  L = 3: scales 1, 2^-6, 2^-12; L = 2: 1, 2^-13 -- the last level is fully hashed
CASES = [("uniform", F, T, 3 if (i + j) % 2 else 2, N, "uniform", "open")
         for F in (2, 4) for i, T in enumerate(TABLES) for j, N in enumerate(SIZES)]
CASES += [("identical", 2, 2 ** 14, 3, 8195, "identical", "open"), ("identical", 4, 2 ** 15 + 8, 3, 8193, "identical", "open"),
          ("collide", 2, 2 ** 14, 2, 8195, "collide", "open"), ("collide", 4, 2 ** 15 + 8, 2, 12289, "collide", "open"),
          ("closed", 2, 2 ** 15 + 8, 3, 12289, "uniform", "closed"), ("closed", 4, 2 ** 18, 3, 8193, "uniform", "closed")]
IDS = ["%s-F%d-T%d-L%d-N%d" % c[:5] for c in CASES]


def cache_slot(row, F):
    """slot of a table row in the binning kernel's LDS cache (ScatterCache<F, 4096>::add in csrc/encode.hip)"""
    return (row ^ (row >> 12)) & (4096 // F - 1)


def build_case(dev, case):
    """-> (setup, points, upstream gradient): seeded, the same in this process and in the child"""
    name, F, T, L, N, kind, window = case
    s = Setup(dev, 3, F, T, L=L, window="open", seed=len(name) + N % 7, concat=False)
    if window == "closed":
        w = torch.ones(L)
        w[1] = 0.0
        s.win = w.to(dev)
    if kind == "collide":
        # A, B, A, B, ...: no two neighbours equal (the run combine merges nothing); a row of B shares its cache slot with
        # another row of A at the finest level, so one of the two never gets into the cache
        cand = s.points("uniform", 8192)
        rows = s.evaluator(cand, cache=False).level(L - 1)[0].cpu()          # [8192, 4]
        slots = cache_slot(rows, F)
        hit = ((slots[1:, :, None] == slots[0][None, None, :]) & (rows[1:, :, None] != rows[0][None, None, :])).any(2).any(1)
        assert bool(hit.any()), "no candidate shares a cache slot with the first point: this case checks nothing"
        b = 1 + int(torch.nonzero(hit)[0])
        pts = cand[[0, b]].repeat((N + 1) // 2, 1)[:N].contiguous()
    else:
        pts = s.points(kind, N)
    return s, pts, s.grad(N)


def run_case(case, plain):
    """the lattice gradient of one case -> (gradient, setup, points, upstream gradient, tail counters or None)"""
    from permuto_sdf_amd.encoding import _head, _tail
    Lb = _lib()
    dev = torch.device("cuda")
    s, pts, g = build_case(dev, case)
    N = pts.shape[0]
    plan = queue_plan(s.P, s.F, N, s.L, s.T)
    assert plan is not None and workspace_bytes(s, N) == (0 if plain else plan["bytes"])
    ws = torch.zeros(plan["bytes"], dtype=torch.uint8, device=dev)
    gl = torch.zeros_like(s.lat)
    Lb.call("psdf_encode_backward_ws", *_head(s.cfg, N), Lb.ptr(pts), Lb.ptr(s.lat), Lb.ptr(s.sf), Lb.ptr(s.sh), Lb.ptr(s.win),
            *_tail(s.cfg), Lb.ptr(fm(g)), Lb.ptr(gl), None, Lb.ptr(ws), Lb.c_l(plan["bytes"]), Lb.stream())
    torch.cuda.synchronize()
    assert last_path() == (1 if plain else 2)
    tails = ws[plan["tails_off"]:plan["tails_off"] + s.L * plan["np"] * 4].view(torch.int32).view(s.L, plan["np"]).cpu()
    return gl, s, pts, g, (None if plain else (tails, plan))


@pytest.fixture(scope="module")
def plain_path():
    """{case id: lattice gradient of the plain path}: one child process for every case"""
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "plain.npz")
        env = dict(os.environ, PSDF_ENC_QUEUE_MIN_N=str(2 ** 40), PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
        r = subprocess.run([sys.executable, "-m", "tests.test_gpu_encode_reduce_wide", out], cwd=ROOT, env=env,
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        return dict(np.load(out))


SEEN = {"length": [0, 0, 0, 0], "offset": [0, 0, 0, 0], "ragged": 0, "queues": 0}


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_binned_lattice_gradient(dev, plain_path, case):
    name, F, T, L, N = case[:5]
    gl, s, pts, g, (tails, plan) = run_case(case, plain=False)
    n = tails.clamp(max=plan["cap"])
    assert int((tails > plan["cap"]).sum()) == 0                      # no queue overflowed: every entry went through the fold loop
    first = (torch.arange(L * plan["np"]).view(L, plan["np"]) * plan["cap"]) % 4      # a queue's first entry inside its group of 4
    for k in range(4):
        SEEN["length"][k] += int(((n % 4 == k) & (n > 0)).sum())
        SEEN["offset"][k] += int(((first == k) & (n > 0)).sum())
    SEEN["queues"] += int((n > 0).sum())
    SEEN["ragged"] += int(((n > 0) & ((first != 0) | (n % 4 != 0))).sum())
    queued = n.sum(1).tolist()
    print("    %s: capacity %d (mod 4: %d), %d partitions, queued per level %s of %d contributions"
          % (IDS[CASES.index(case)], plan["cap"], plan["cap"] % 4, plan["np"], queued, 4 * N))
    if name != "identical":         # (all points equal: the cache absorbs the batch at these sizes, see the head of this file)
        assert queued[-1] > 0, "nothing reached the finest level's queues: this case checks nothing"
    if name == "uniform":
        # (a super-tile's 2048 contributions first fill the empty slots of its workgroup's LDS cache: about a third to a half
        # of a fully hashed level's contributions are queued at these sizes, the rest leaves the cache as float atomics)
        assert queued[-1] >= N, "the finest level is not fully hashed: this case checks nothing"
    if name == "collide":
        assert queued[-1] >= N // 2 - 512, "the colliding row was not queued: this case checks nothing"
    ev = s.evaluator(pts)
    val, mag, cnt = ev.lattice_grad(g)
    check(tag_of(s, N, "lattice, %s (binned)" % name), gl, (val, mag, cnt), R_LAT)
    if name == "closed":
        assert float(gl[1].abs().max()) == 0.0 and int(n[1].sum()) == 0
    # against the plain path: the same terms in another order
    other = torch.from_numpy(plain_path[IDS[CASES.index(case)]]).to(gl.device)
    m = cnt.double().expand_as(val)
    k = (m - 1).clamp_min(0)
    bar = 2 * (k * e64.U / (1 - k * e64.U)) * mag * (1 + e64.U) ** 2 + 2 * m * e64.TINY * (m > 1)
    err = (gl.double() - other.double()).abs()
    worst = float(torch.where(bar > 0, err / bar.clamp_min(1e-300),
                              torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err))).max())
    print("    [err/bar] binned against plain path: %.3f   (entries with one term: %d, bit-equal)" % (worst, int((m == 1).sum())))
    assert worst <= 1.0, "binned and plain path differ by more than two orders of one sum can: %.4g" % worst


def test_every_residue_was_exercised(dev):
    """runs after the cases above (file order): queues per length residue and per start residue mod 4"""
    print("    queues folded: %d, with a ragged end: %d; by length mod 4: %s; by first entry mod 4: %s"
          % (SEEN["queues"], SEEN["ragged"], SEEN["length"], SEEN["offset"]))
    assert SEEN["queues"] > 0, "run the whole file: this test reads what the cases before it counted"
    assert all(c > 0 for c in SEEN["length"]) and all(c > 0 for c in SEEN["offset"]), SEEN


if __name__ == "__main__":      # the child of plain_path(): every case on the plain path, gradients to an .npz
    assert int(os.environ["PSDF_ENC_QUEUE_MIN_N"]) > max(SIZES)
    np.savez(sys.argv[1], **{i: run_case(c, plain=True)[0].cpu().numpy() for i, c in zip(IDS, CASES)})
