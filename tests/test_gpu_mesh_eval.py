"""GPU: the three stages of the DTU Chamfer protocol (permuto_sdf_amd/mesh_eval.py, csrc/mesh_eval.hip) and the protocol end to
end, against the float64 restatement tests/mesh_eval_reference.py (pinned to sklearn by tests/test_mesh_eval_host.py).

u = 2^-24.  Bars:
  * sampling: per-triangle counts equal (every input triangle keeps l / s further than 1e-9 relative from an integer: asserted),
    order identical, positions within 2 u max|coordinate of the point| of the helper's rounded to fp32, vertices first;
  * thinning: the mask equals the sequential loop's exactly; before comparing, no pair of the cloud lies within 16 u radius of
    the radius (the fp32 difference form errs by ~3.5 u: a closer pair is a coin toss for any implementation): asserted;
  * nearest neighbour: |d - d64| <= 4 u d64 -- one rounding per component difference (2 u on the squares), the squares (1 u), two
    sums (2 u), halved by the root plus its own rounding: 3.5 u, half a u of headroom; d = 0 exact for duplicates; the index is
    checked through its distance, ||q - ref[idx]||64 <= d64 (1 + 4 u); (max_dist, -1) exactly where d64 >= max_dist, and no query
    has d64 within 8 u max_dist of the cut-off: asserted.
Run with -s for the largest observed error / bar per stage, the sweep counts and the share of queries the ring search finished."""
import ctypes

import numpy as np
import pytest
import torch

from tests import mesh_eval_reference as ref

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


def noisy_sphere(seed, n):
    r = np.random.default_rng(seed)
    v = r.standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return (v * 0.4 + r.standard_normal((n, 3)) * 0.002).astype(np.float32)


def planned_edge(points, n, min_edge=0.0):
    """the cell edge and dims the library plans for a cloud (its box from the finite points)"""
    from permuto_sdf_amd import _lib as L
    p = np.asarray(points, dtype=np.float32)
    p = p[np.isfinite(p).all(1)].astype(np.float64)
    oe, dims, cells = (ctypes.c_float * 4)(), (ctypes.c_int * 3)(), ctypes.c_int64(0)
    L.call("psdf_mesh_eval_grid_plan", (ctypes.c_double * 3)(*p.min(0)), (ctypes.c_double * 3)(*p.max(0)), ctypes.c_int64(n),
           ctypes.c_double(min_edge), ctypes.c_int64(0), oe, dims, ctypes.byref(cells), None)
    return float(oe[3]), list(dims)


# ------------------------------------------------------------------------------------------------------------- sampling
DENSITY = 0.2


def sampling_mesh():
    r = np.random.default_rng(11)
    V, F = [], []

    def tri(p0, p1, p2):
        F.append([len(V), len(V) + 1, len(V) + 2])
        V.extend([p0, p1, p2])

    def unit(k):
        v = r.standard_normal((k, 3))
        return v / np.linalg.norm(v, axis=1, keepdims=True)

    p0 = r.uniform(-10, 10, (500, 3))
    l = r.uniform(0.5, 20.0, (500, 2)) * DENSITY
    d1, d2 = unit(500), unit(500)
    for k in range(500):
        tri(p0[k], p0[k] + l[k, 0] * d1[k], p0[k] + l[k, 1] * d2[k])
    tri([1, 2, 3], [1, 2, 3], [2, 2, 3])                                     # two equal corners
    tri([0, 0, 0], [1, 1, 1], [2, 2, 2])                                     # three collinear corners (exactly, in fp32)
    tri([5, 5, 5], [5 + 0.3 * DENSITY, 5, 5], [5, 5 + 0.3 * DENSITY, 5])     # smaller than the density: n1 = n2 = 0
    for n in (3, 4, 5, 7):                                                   # right isosceles: the a + b = 1 knife edge
        leg = (n + 0.5) * DENSITY
        tri([0, 0, 0], [leg, 0, 0], [0, leg, 0])
        tri([-3, 1, 2], [-3, 1 + leg, 2], [-3, 1, 2 + leg])
    return np.asarray(V, dtype=np.float32), np.asarray(F, dtype=np.int32)


def test_sampling_counts_order_and_positions(dev):
    from permuto_sdf_amd import mesh_eval as me
    V, F = sampling_mesh()
    want, counts, margin = ref.sample_surface(V, F, DENSITY)
    assert margin.min() > 1e-9, "an input triangle has l / s within 1e-9 of an integer: its count is a coin toss"
    _, _, _, n1, n2, _ = ref.triangle_lattice(V, F, DENSITY)
    assert n1[500] == -1 and n1[501] == -1 and (n1[502], n2[502]) == (0, 0) and counts[500:503].tolist() == [0, 0, 0]
    assert [(n1[503 + k], n2[503 + k]) for k in range(8)] == [(n, n) for n in (3, 4, 5, 7) for _ in range(2)]
    assert counts[:500].max() > 150 and counts[:500].min() == 0
    got = me.sample_surface(torch.from_numpy(V).to(dev), torch.from_numpy(F).to(dev), DENSITY)
    assert got.dtype == torch.float32 and got.shape == (len(V) + counts.sum(), 3), (got.shape, len(V) + counts.sum())
    got = got.cpu().numpy()
    assert np.array_equal(got[:len(V)], V)                                   # vertices first
    # the counts, triangle by triangle, through the library's own count pass
    from permuto_sdf_amd import _lib as L
    c = torch.empty(len(F), dtype=torch.int32, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    L.call("psdf_mesh_sample_count", L.ptr(torch.from_numpy(V).to(dev)), L.c_l(len(V)), L.ptr(torch.from_numpy(F).to(dev)),
           L.c_l(len(F)), ctypes.c_double(DENSITY), L.ptr(c), L.ptr(flag), L.stream())
    assert np.array_equal(c.cpu().numpy(), counts) and int(flag) == 0
    want32 = want.astype(np.float32)
    bar = 2 * U * np.abs(want32).max(1, keepdims=True).astype(np.float64)
    err = np.abs(got.astype(np.float64) - want32.astype(np.float64))
    ratio = float((err[len(V):] / bar[len(V):]).max())
    print("\nsampling: %d triangles, %d samples, largest position error / bar = %.3f" % (len(F), counts.sum(), ratio))
    assert ratio <= 1.0                                                      # same order: row k is sample k
    # no faces: the vertices alone; a face that names a vertex outside the mesh is refused
    assert me.sample_surface(torch.from_numpy(V).to(dev), torch.zeros((0, 3), dtype=torch.int32, device=dev), DENSITY).shape == (len(V), 3)
    with pytest.raises(ValueError):
        me.sample_surface(torch.from_numpy(V[:3]).to(dev), torch.tensor([[0, 1, 3]], dtype=torch.int32, device=dev), DENSITY)


# ------------------------------------------------------------------------------------------------------------- thinning
def thinning_cases():
    """name -> (points fp32, radius, order, the mask known by hand or None)"""
    cases = {}
    for seed, radius in ((0, 0.02), (2, 0.05), (0, 0.05), (2, 0.02)):
        p = noisy_sphere(seed, 3000)
        cases["sphere seed %d r %.2f" % (seed, radius)] = (p, radius, np.random.default_rng(seed + 100).permutation(len(p)), None)
    for n in (1, 2, 63, 64, 65, 257):
        p = noisy_sphere(7, 3000)[:n] * np.float32(0.25)               # a dense patch: most points have neighbours
        cases["n = %d" % n] = (p, 0.02, np.random.default_rng(n).permutation(n), None)
    # radii whose fp32 value lies above the double, on clouds dense enough that the radius decides the cell edge: the grid must
    # be planned with the radius the sweeps compare against
    for radius in (0.008, 0.064):
        p = noisy_sphere(12, 3000) * np.float32(10 * radius)
        cases["radius %.3f decides the edge" % radius] = (p, radius, np.random.default_rng(12).permutation(len(p)), None)
    same = np.tile(np.array([[0.25, -1.5, 3.0]], dtype=np.float32), (257, 1))
    order = np.random.default_rng(3).permutation(257)
    first = np.zeros(257, dtype=bool)
    first[order[0]] = True
    cases["identical points"] = (same, 0.02, order, first)
    radius = 0.02
    line = np.zeros((300, 3), dtype=np.float32)
    line[:, 0] = np.arange(300, dtype=np.float32) * np.float32(0.6 * radius)
    cases["sorted line"] = (line, radius, np.arange(300), np.arange(300) % 2 == 0)
    # points exactly on cell boundaries: the radius decides the edge (asserted in the test), coordinates = origin + k edge
    radius = 0.125
    edge = np.float32(radius * (1 + 1 / 512))
    r = np.random.default_rng(5)
    k = np.stack(np.meshgrid(*[np.arange(4)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    corner = np.array([0.3, -1.7, 2.1], dtype=np.float32) + k * edge
    jit = r.standard_normal((4, 64, 3))
    jit = (jit / np.linalg.norm(jit, axis=2, keepdims=True) * r.uniform(0.1, 0.45, (4, 64, 1)) * radius).astype(np.float32)
    inner = (corner[None] + jit).reshape(-1, 3)
    inner = np.clip(inner, corner.min(0), corner.max(0))                # the lattice's extremes stay the box
    p = np.concatenate([corner, inner]).astype(np.float32)
    cases["cell boundaries"] = (p, radius, r.permutation(len(p)), None)
    return cases


THIN = thinning_cases()


@pytest.mark.parametrize("name", list(THIN))
def test_thinning_equals_the_sequential_loop(dev, name):
    from permuto_sdf_amd import mesh_eval as me
    p, radius, order, by_hand = THIN[name]
    if len(p) > 1:
        gap = ref.pair_distances_min_gap(p, np.float64(np.float32(radius)))
        assert gap > 16 * U * radius, "a pair lies within 16 u radius of the radius (%.3g): a coin toss" % gap
    want = ref.radius_thin(p, np.float64(np.float32(radius)), order)
    if by_hand is not None:
        assert np.array_equal(want, by_hand)
    if name.endswith("decides the edge"):
        assert np.float64(np.float32(radius)) > radius
        floor = np.float64(np.float32(radius)) * (1 + 1 / 512)
        assert floor <= planned_edge(p, len(p), float(np.float32(radius)))[0] <= floor * (1 + 2 * U)     # the radius decides
    if name == "cell boundaries":
        edge, dims = planned_edge(p, len(p), radius)
        assert edge == np.float32(radius * (1 + 1 / 512)) and dims == [4, 4, 4]
        assert 1 < want.sum() < len(p)
    mask, sweeps = me.radius_thin(torch.from_numpy(p).to(dev), radius, order=torch.from_numpy(order), return_sweeps=True)
    assert mask.dtype == torch.bool and mask.shape == (len(p),)
    print("\nthinning %s: %d of %d kept, %d sweeps" % (name, int(mask.sum()), len(p), sweeps))
    assert np.array_equal(mask.cpu().numpy(), want)
    if name == "sorted line":
        assert sweeps >= 100            # about N / 2: a loop with a sweep cap would have stopped with a wrong answer


def test_thinning_of_an_empty_cloud_and_default_order(dev):
    from permuto_sdf_amd import mesh_eval as me
    mask = me.radius_thin(torch.zeros((0, 3), device=dev), 0.1)
    assert mask.shape == (0,) and mask.dtype == torch.bool
    # default order: torch.randperm from the generator -- the same generator state gives the same mask, and it is a maximal
    # independent set whatever the order: no two kept points within the radius, every dropped point within it of a kept one
    p = noisy_sphere(0, 3000)
    pt = torch.from_numpy(p).to(dev)
    a = me.radius_thin(pt, 0.05, generator=torch.Generator().manual_seed(4))
    b = me.radius_thin(pt, 0.05, generator=torch.Generator().manual_seed(4))
    assert torch.equal(a, b)
    order = torch.randperm(3000, generator=torch.Generator().manual_seed(4))
    assert np.array_equal(a.cpu().numpy(), ref.radius_thin(p, np.float64(np.float32(0.05)), order.numpy()))
    # an order that is no permutation is refused, not answered
    twice = order.clone()
    twice[5] = twice[6]
    for bad in (twice, order - 1, order[:-1]):
        with pytest.raises(ValueError):
            me.radius_thin(pt, 0.05, order=bad)


# ------------------------------------------------------------------------------------------------------------- nearest
def check_nearest(dev, q, r, max_dist, label, cell_budget=None):
    """runs nearest() and checks it against brute-force float64; -> (largest error / bar, share of queries left to the ring)"""
    from permuto_sdf_amd import mesh_eval as me
    q, r = np.asarray(q, dtype=np.float32).reshape(-1, 3), np.asarray(r, dtype=np.float32).reshape(-1, 3)
    fin_r = np.isfinite(r).all(1)
    fin_q = np.isfinite(q).all(1)
    d64, i64 = ref.nearest(np.where(fin_q[:, None], q, 0).astype(np.float64), r[fin_r].astype(np.float64))
    d64[~fin_q] = np.inf
    assert not (np.abs(d64 - max_dist) <= 8 * U * max_dist).any(), "a query lies within 8 u max_dist of the cut-off"
    d, idx, nr_open = me.nearest(torch.from_numpy(q).to(dev), torch.from_numpy(r).to(dev), max_dist, cell_budget=cell_budget,
                                 return_stats=True)
    assert d.dtype == torch.float32 and idx.dtype == torch.int64 and d.shape == idx.shape == (len(q),)
    d, idx = d.cpu().numpy(), idx.cpu().numpy()
    far = d64 >= max_dist
    assert np.array_equal(idx < 0, far), (label, int((idx < 0).sum()), int(far.sum()))
    assert (d[far] == np.float32(max_dist)).all() and (idx[far] == -1).all()
    near = ~far
    ratio = 0.0
    if near.any():
        assert fin_r[idx[near]].all(), "a non-finite reference was returned"
        err = np.abs(d[near].astype(np.float64) - d64[near])
        bar = 4 * U * d64[near]
        assert (err <= bar).all(), (label, float(err.max()), float((err / np.maximum(bar, 1e-300)).max()))
        assert (d[near][d64[near] == 0] == 0).all()
        through = np.sqrt(((q[near].astype(np.float64) - r[idx[near]].astype(np.float64)) ** 2).sum(1))
        assert (through <= d64[near] * (1 + 4 * U)).all(), label
        nz = bar > 0
        ratio = float((err[nz] / bar[nz]).max()) if nz.any() else 0.0
    share = float(int(nr_open)) / max(len(q), 1)
    print("\nnearest %s: %d x %d, %d beyond the cut-off, largest error / bar = %.3f, left to the ring search %.1f %%"
          % (label, len(q), len(r), int(far.sum()), ratio, 100 * share))
    return ratio, share


def test_nearest_on_noisy_spheres_at_scan_scale(dev):
    r = noisy_sphere(5, 4096) * np.float32(500)
    q = noisy_sphere(6, 4096) * np.float32(500) + np.float32(0.3)
    check_nearest(dev, q, r, 20.0, "spheres x 500")
    check_nearest(dev, q, r, 2.0, "spheres x 500, cut-off 2")          # many queries beyond the cut-off
    check_nearest(dev, q, np.concatenate([r, q[:100]]), 20.0, "with duplicates")      # d = 0 exactly


@pytest.mark.parametrize("nq, nr", [(0, 5), (5, 0), (0, 0), (1, 1), (63, 65), (64, 64), (65, 63), (1, 65), (65, 1)])
def test_nearest_small_and_empty(dev, nq, nr):
    q, r = noisy_sphere(8, 65)[:nq], noisy_sphere(9, 65)[:nr]
    if nr == 0:
        from permuto_sdf_amd import mesh_eval as me
        d, idx = me.nearest(torch.from_numpy(q).to(dev), torch.from_numpy(r).to(dev), 0.5)
        assert d.shape == idx.shape == (nq,) and (d == 0.5).all() and (idx == -1).all()
        return
    check_nearest(dev, q, r, 0.5, "%d x %d" % (nq, nr))
    check_nearest(dev, q, r, 0.03, "%d x %d, tight cut-off" % (nq, nr))


def test_nearest_one_cell_with_more_references_than_two_tiles(dev):
    from permuto_sdf_amd import mesh_eval as me
    cap = me.tile_capacity()
    g = np.random.default_rng(21)
    corners = np.array([[x, y, z] for x in (0, 10) for y in (0, 10) for z in (0, 10)], dtype=np.float32)
    cluster = (5.5 + g.uniform(-1e-3, 1e-3, (2 * cap + 100, 3))).astype(np.float32)
    r = np.concatenate([corners, cluster])
    edge, dims = planned_edge(r, len(r))
    cell = np.floor(cluster.astype(np.float64) / edge)
    assert (cell == cell[0]).all() and min(dims) >= 4                   # one cell holds the whole cluster
    q = np.concatenate([(5.5 + g.uniform(-1e-2, 1e-2, (300, 3))), g.uniform(0, 10, (300, 3))]).astype(np.float32)
    _, share = check_nearest(dev, q, r, 20.0, "heavy cell")
    assert share < 1.0


def test_nearest_across_a_cell_corner_and_a_block_boundary(dev):
    g = np.random.default_rng(22)
    corners = np.array([[x, y, z] for x in (0, 8) for y in (0, 8) for z in (0, 8)], dtype=np.float32)
    filler = np.concatenate([g.uniform(0, 8, (990, 2)), np.full((990, 1), 8.0)], 1).astype(np.float32)      # far from the query
    base = np.concatenate([corners, filler])
    edge, dims = planned_edge(base, len(base) + 2)
    assert min(dims) >= 6
    q = (np.full(3, 4 * edge) + 0.05 * edge).astype(np.float32)[None]        # just inside cell (4, 4, 4): the first of a block
    same_cell = q + np.array([[0.9 * edge, 0, 0]], dtype=np.float32)
    diagonal = q - np.float32(0.2 * edge / np.sqrt(3))
    assert (np.floor(same_cell / edge) == 4).all() and (np.floor(diagonal / edge) == 3).all()
    r = np.concatenate([base, same_cell, diagonal]).astype(np.float32)
    assert planned_edge(r, len(r))[0] == edge
    from permuto_sdf_amd import mesh_eval as me
    check_nearest(dev, q, r, 20.0, "cell corner")
    _, idx = me.nearest(torch.from_numpy(q).to(dev), torch.from_numpy(r).to(dev), 20.0)
    assert int(idx[0]) == len(r) - 1


def test_nearest_several_shells_out_and_outside_the_box(dev):
    # a 4^3 lattice of spacing s, and enough duplicates of one corner that the planned edge is s / 5
    g = np.random.default_rng(23)
    s = 2.0
    lattice = (np.stack(np.meshgrid(*[np.arange(4)] * 3, indexing="ij"), -1).reshape(-1, 3) * s).astype(np.float32)
    r = np.concatenate([lattice, np.zeros((5336, 3), dtype=np.float32)])
    edge, dims = planned_edge(r, len(r))
    assert abs(edge - s / 5) < 1e-6 * s and min(dims) >= 15
    q = g.uniform(0, 3 * s, (500, 3)).astype(np.float32)
    _, share = check_nearest(dev, q, r, 10 * s, "lattice 5 edges apart")
    assert share > 0.5                                                   # the answers lie several shells out
    check_nearest(dev, q, r, 0.5 * s, "lattice, cut-off below the far answers")
    # outside the box by less and by more than max_dist, on every side
    out = []
    for axis in range(3):
        for sign in (-1, 1):
            for by in (0.3, 0.9, 1.1, 4.0):
                p = g.uniform(0, 3 * s, (20, 3))
                p[:, axis] = (3 * s + by) if sign > 0 else -by
                out.append(p)
    check_nearest(dev, np.concatenate(out).astype(np.float32), r, 1.0, "outside the box")
    check_nearest(dev, np.array([[1e6, -1e6, 3.0], [-40.0, 2.0, 2.0]], dtype=np.float32), r, 20.0, "far outside")


def test_nearest_points_on_cell_boundaries(dev):
    g = np.random.default_rng(24)
    base = g.uniform(0, 10, (4000, 3)).astype(np.float32)
    base[:8] = np.array([[x, y, z] for x in (0, 10) for y in (0, 10) for z in (0, 10)], dtype=np.float32)
    edge, dims = planned_edge(base, len(base))
    k = g.integers(0, min(dims), (4000, 3))
    on = (k * np.float32(edge)).astype(np.float32)
    r = np.where(g.random((4000, 1)) < 0.5, on, base).astype(np.float32)
    r[:8] = base[:8]
    assert planned_edge(r, len(r))[0] == edge
    q = np.concatenate([(g.integers(0, min(dims), (500, 3)) * np.float32(edge)), g.uniform(0, 10, (500, 3))]).astype(np.float32)
    check_nearest(dev, q, r, 20.0, "cell boundaries")


def test_nearest_with_non_finite_points(dev):
    from permuto_sdf_amd import mesh_eval as me
    r = noisy_sphere(5, 1000) * np.float32(500)
    q = noisy_sphere(6, 1000) * np.float32(500) + np.float32(0.3)
    inner = np.argsort(np.abs(r).max(1))[:2]                               # two references that do not span the box
    clean = np.delete(r, inner, 0)
    d0, i0 = me.nearest(torch.from_numpy(q).to(dev), torch.from_numpy(clean).to(dev), 20.0)
    r2, q2 = r.copy(), q.copy()
    r2[inner[0], 1] = np.nan
    r2[inner[1], 2] = np.inf
    q2[10, 0] = np.nan
    q2[20, 2] = -np.inf
    check_nearest(dev, q2, r2, 20.0, "non-finite")
    d, idx = me.nearest(torch.from_numpy(q2).to(dev), torch.from_numpy(r2).to(dev), 20.0)
    assert d[10] == 20.0 and idx[10] == -1 and d[20] == 20.0 and idx[20] == -1
    others = np.ones(1000, dtype=bool)
    others[[10, 20]] = False
    rows = np.delete(np.arange(1000), inner)                               # row of `clean` -> row of r
    assert torch.equal(d[others], d0[others])                              # all other answers are unaffected
    assert np.array_equal(idx.cpu().numpy()[others], np.where(i0.cpu().numpy() >= 0, rows[i0.cpu().numpy().clip(0)], -1)[others])
    # every reference non-finite: nothing to return
    d, idx = me.nearest(torch.from_numpy(q[:5]).to(dev), torch.full((3, 3), float("nan"), device=dev), 20.0)
    assert (d == 20.0).all() and (idx == -1).all()


# ------------------------------------------------------------------------------------------------------------- end to end
E2E_DENSITY, E2E_MAX_DIST, E2E_N = 0.01, 0.1, 48


@pytest.fixture(scope="module")
def sphere_case(dev):
    """the sphere mesh, the scan, the shuffle, the helper's cloud -- computed once and left unchanged"""
    from permuto_sdf_amd.mesh import marching_tetrahedra
    axis = torch.linspace(-0.5, 0.5, E2E_N, device=dev)
    x, y, z = torch.meshgrid(axis, axis, axis, indexing="ij")
    h = 1.0 / (E2E_N - 1)
    V, F, _, _ = marching_tetrahedra(torch.sqrt(x * x + y * y + z * z) - 0.4, 0.0, spacing=(h, h, h), normals=False)
    V = V - 0.5
    g = np.random.default_rng(31)
    gt = g.standard_normal((20000, 3))
    gt = (gt / np.linalg.norm(gt, axis=1, keepdims=True) * 0.4).astype(np.float32)
    from permuto_sdf_amd import mesh_eval as me
    cloud = me.sample_surface(V, F, E2E_DENSITY).cpu().numpy()
    # the helper's cloud, rounded to fp32: same length, same order, within 2 u max|coordinate|; the later stages of both sides
    # start from the cloud the device sampled
    cloud64, counts, margin = ref.sample_surface(V.cpu().numpy(), F.cpu().numpy(), E2E_DENSITY)
    assert margin.min() > 1e-9 and cloud.shape == cloud64.shape
    want32 = cloud64.astype(np.float32)
    err = np.abs(cloud.astype(np.float64) - want32.astype(np.float64))
    assert (err <= 2 * U * np.abs(want32).max(1, keepdims=True)).all()
    print("\nend to end: %d triangles, %d points sampled, %d rows differ from the helper's in the last bit"
          % (len(F), len(cloud), int((err > 0).any(1).sum())))
    order = g.permutation(len(cloud))
    # no pair of the cloud within 16 u radius of the radius (KD-tree pair counts on both sides of the band)
    from scipy.spatial import cKDTree
    tree, rad = cKDTree(cloud.astype(np.float64)), np.float64(np.float32(E2E_DENSITY))
    assert tree.count_neighbors(tree, rad * (1 + 32 * U)) == tree.count_neighbors(tree, rad * (1 - 32 * U))
    return {"V": V, "F": F, "gt": gt, "cloud": cloud, "order": order, "h": h}


def _means_close(got, want, n, label):
    bar = 4 * U * abs(want) + n * 2.0 ** -53 * abs(want)
    print("\nend to end %s: %.9g against %.9g, error / bar = %.3f" % (label, got, want, abs(got - want) / bar))
    assert abs(got - want) <= bar, (label, got, want)


def test_chamfer_end_to_end_equals_the_helpers_pipeline(dev, sphere_case):
    from permuto_sdf_amd import mesh_eval as me
    c = sphere_case
    res = me.chamfer_dtu((c["V"], c["F"]), torch.from_numpy(c["gt"]).to(dev), density=E2E_DENSITY, max_dist=E2E_MAX_DIST,
                         order=torch.from_numpy(c["order"]))
    cloud = c["cloud"]
    want = ref.chamfer_dtu(c["cloud"], c["gt"], c["order"], np.float64(np.float32(E2E_DENSITY)), E2E_MAX_DIST, tree=True)
    for v in (want["d2s"], want["s2d"]):
        assert not (np.abs(v - E2E_MAX_DIST) <= 8 * U * E2E_MAX_DIST).any()
    assert np.array_equal(np.nonzero(res.kept_mask.cpu().numpy())[0], want["kept"])      # the kept set is identical
    assert np.array_equal(res.kept.cpu().numpy(), c["cloud"][want["kept"]])
    assert res.data_in.shape == res.kept.shape and res.data_in_obs.shape == res.kept.shape   # no filter given
    print("\nend to end: %d points sampled, %d kept in %d sweeps, %d of %d queries left to the ring search"
          % (len(cloud), len(want["kept"]), res.sweeps, res.nr_open, len(want["d2s"]) + len(want["s2d"])))
    _means_close(res.mean_d2s, want["mean_d2s"], len(want["d2s"]), "data -> scan")
    _means_close(res.mean_s2d, want["mean_s2d"], len(want["s2d"]), "scan -> data")
    assert res.overall == (res.mean_d2s + res.mean_s2d) / 2
    assert res.mean_d2s < c["h"] and res.mean_s2d < c["h"]                    # both below the grid spacing
    for got, w in ((res.dist_d2s, want["d2s"]), (res.dist_s2d, want["s2d"])):
        assert (np.abs(got.cpu().numpy().astype(np.float64) - w) <= 4 * U * w).all()
    # an ExtractedMesh is accepted as well, and the default order comes from the generator
    from permuto_sdf_amd.mesh import ExtractedMesh
    again = me.chamfer_dtu(ExtractedMesh(c["V"], c["F"]), torch.from_numpy(c["gt"]).to(dev), density=E2E_DENSITY,
                           max_dist=E2E_MAX_DIST, generator=torch.Generator().manual_seed(1))
    assert abs(again.overall - res.overall) < 0.05 * res.overall and again.kept.shape[0] != 0


def test_chamfer_filters_select_the_helpers_index_sets(dev, sphere_case):
    from permuto_sdf_amd import mesh_eval as me
    c = sphere_case
    g = np.random.default_rng(32)
    bb = np.array([[-0.3, -0.3, -0.3], [0.1, 0.2, 0.3]], dtype=np.float32)
    obs = g.random((16, 12, 16)) < 0.6
    patch, res_, plane = 0.05, 0.05, np.array([0.0, 0.0, 1.0, 0.1])
    res = me.chamfer_dtu((c["V"], c["F"]), torch.from_numpy(c["gt"]).to(dev), density=E2E_DENSITY, max_dist=E2E_MAX_DIST,
                         patch=patch, obs_mask=torch.from_numpy(obs), bb=torch.from_numpy(bb), res=res_,
                         plane=torch.from_numpy(plane), order=torch.from_numpy(c["order"]))
    want = ref.chamfer_dtu(c["cloud"], c["gt"], c["order"], np.float64(np.float32(E2E_DENSITY)), E2E_MAX_DIST, patch=patch,
                           obs_mask=obs, bb=bb, res=res_, plane=plane, tree=True)
    # no coordinate on a knife edge of the rounding to grid indices
    frac = (c["cloud"][want["data_in"]].astype(np.float64) - bb[0].astype(np.float64)) / res_
    assert np.abs(np.abs(frac - np.floor(frac)) - 0.5).min() > 1e-9
    assert 0 < len(want["data_in_obs"]) < len(want["data_in"]) < len(want["kept"]) and 0 < len(want["gt_above"]) < len(c["gt"])
    assert np.array_equal(res.data_in.cpu().numpy(), c["cloud"][want["data_in"]])
    assert np.array_equal(res.data_in_obs.cpu().numpy(), c["cloud"][want["data_in_obs"]])
    assert res.dist_s2d.shape[0] == len(want["gt_above"]) and res.dist_d2s.shape[0] == len(want["data_in_obs"])
    # the selected scan rows, query by query: row k of dist_s2d answers scan point gt_above[k]
    for v in (want["d2s"], want["s2d"]):
        assert not (np.abs(v - E2E_MAX_DIST) <= 8 * U * E2E_MAX_DIST).any()
    for got, w in ((res.dist_d2s, want["d2s"]), (res.dist_s2d, want["s2d"])):
        got, cut = got.cpu().numpy().astype(np.float64), np.minimum(w, np.float64(np.float32(E2E_MAX_DIST)))
        assert (np.abs(got - cut) <= 4 * U * cut).all()
    _means_close(res.mean_d2s, want["mean_d2s"], len(want["d2s"]), "data -> scan, filtered")
    _means_close(res.mean_s2d, want["mean_s2d"], len(want["s2d"]), "scan -> data, filtered")
    # an empty selection gives NaN, as numpy's mean does
    empty = me.chamfer_dtu(torch.from_numpy(c["cloud"][:500]).to(dev), torch.from_numpy(c["gt"]).to(dev), density=E2E_DENSITY,
                           max_dist=E2E_MAX_DIST, bb=torch.tensor([[5.0, 5.0, 5.0], [6.0, 6.0, 6.0]]), patch=0.0)
    assert empty.data_in.shape[0] == 0 and np.isnan(empty.mean_d2s) and np.isnan(empty.mean_s2d) and np.isnan(empty.overall)
