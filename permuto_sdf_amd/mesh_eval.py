"""Mesh evaluation on the device: the DTU-protocol Chamfer distance (csrc/mesh_eval.hip).

The reference scores an extracted mesh with permuto_sdf_py/experiments/evaluation/evaluate_chamfer_distance.py, which runs
DTUeval-python/eval.py: sample the mesh's triangles, shuffle and thin the cloud to one point per `density`, filter it with the
scan's box and observation mask, and average the nearest-neighbour distances below `max_dist` in both directions.  Here the
three data-parallel stages are kernels over tensors `MeshExtractor` leaves on the device:

  * `sample_surface(V, F, density)`        lattice sampling of every triangle (count -> scan -> emit);
  * `radius_thin(points, radius, order)`   the order-dependent thinning, as sweeps of its parallel form;
  * `nearest(query, ref, max_dist)`        exact nearest neighbour with a cut-off, over a uniform grid;
  * `chamfer_dtu(mesh, gt_points, ...)`    the protocol end to end (the filters are plain torch: they are not hot).

Loading `.mat` / `.ply` files stays the caller's business.  Host reads: one per grid (the cloud's bounding box and its
number of finite points -- the grid's size decides allocations -- and, in the thinning, the check that `order` is a permutation,
all in one transfer), the sample total, and the undecided counter of the thinning (at most one read per sweep).
"""
import ctypes

import torch

from . import _lib as L

_SWEEPS_PER_READ = 4        # sweeps enqueued between two reads of the undecided counters (each sweep has a counter of its own)
_BLOCK_LOG2 = 2             # cells per axis of a query block = 1 << _BLOCK_LOG2 (csrc/mesh_eval_plan.h: QUERY_BLOCK_LOG2)


def tile_capacity():
    """reference points per LDS tile of the cooperative nearest-neighbour kernel"""
    fn = L.lib().psdf_mesh_eval_tile_capacity
    fn.restype = ctypes.c_int
    return int(fn())


def fp32(value):
    """a Python float rounded to fp32 once: the value the kernels receive, and therefore the value every plan is made with"""
    return ctypes.c_float(value).value


class _Grid:
    """the uniform grid of a cloud's finite points: host arrays for the C ABI (csrc/mesh_eval_plan.h decides them).  One host
    read: the box, the number of finite points and the caller's `extra` device scalars in one transfer.  `cells` is 0 when no
    point is finite: there is no grid."""

    def __init__(self, points, min_edge, cell_budget, extra=()):
        inf = float("inf")
        m = torch.isfinite(points).all(1, keepdim=True)
        read = [torch.where(m, points, inf).amin(0).double(), torch.where(m, points, -inf).amax(0).double(), m.sum().double().view(1)]
        box = torch.cat(read + [e.double().view(1) for e in extra]).tolist()            # the host read
        self.n_finite, self.extra = int(box[6]), box[7:]
        self.origin_edge, self.dims = (L.c_f * 4)(), (L.c_i * 3)()
        self.cells = self.blocks = 0
        if self.n_finite == 0:
            return
        cells, blocks = ctypes.c_int64(0), ctypes.c_int64(0)
        L.call("psdf_mesh_eval_grid_plan", (ctypes.c_double * 3)(*box[:3]), (ctypes.c_double * 3)(*box[3:6]), L.c_l(self.n_finite),
               ctypes.c_double(min_edge), L.c_l(cell_budget or 0), self.origin_edge, self.dims, ctypes.byref(cells),
               ctypes.byref(blocks))
        self.cells, self.blocks = cells.value, blocks.value

    def sort(self, points, block_log2=0):
        """-> (points sorted by cell / block, their keys, the permutation, start [cells + 1])"""
        n, dev = points.shape[0], points.device
        keys = torch.empty(n, dtype=torch.int32, device=dev)
        L.call("psdf_mesh_eval_cell_keys", L.ptr(points), L.c_l(n), self.origin_edge, self.dims, L.c_i(block_log2), L.ptr(keys),
               L.stream())
        keys, perm = torch.sort(keys, stable=True)
        count = self.blocks if block_log2 else self.cells
        start = torch.empty(count + 1, dtype=torch.int32, device=dev)
        L.call("psdf_mesh_eval_cell_ranges", L.ptr(keys), L.c_l(n), L.c_l(count), L.ptr(start), L.stream())
        return points[perm].contiguous(), keys, perm, start


def _cloud(points, name):
    L.require_cuda(points)
    if points.ndim != 2 or points.shape[1] != 3:
        raise ValueError("%s must be [N, 3], got %s" % (name, tuple(points.shape)))
    if points.shape[0] > 2 ** 31 - 1:
        raise L.PsdfError("%s: more than 2^31 - 1 points" % name)
    return points.detach().to(torch.float32).contiguous()


@torch.no_grad()
def sample_surface(V, F, density):
    """-> [V + S, 3] fp32: the mesh's vertices followed by the lattice samples of its triangles, in face order"""
    V = _cloud(V, "V")
    L.require_cuda(F)
    if F.ndim != 2 or F.shape[1] != 3:
        raise ValueError("F must be [F, 3], got %s" % (tuple(F.shape),))
    density = float(density)
    if not density > 0.0:
        raise ValueError("density must be positive")
    F = F.detach().to(torch.int32).contiguous()
    nV, nF, dev = V.shape[0], F.shape[0], V.device
    if nF == 0:
        return V.clone()
    counts = torch.empty(nF, dtype=torch.int32, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    L.call("psdf_mesh_sample_count", L.ptr(V), L.c_l(nV), L.ptr(F), L.c_l(nF), ctypes.c_double(density), L.ptr(counts),
           L.ptr(flag), L.stream())
    incl = torch.cumsum(counts, 0, dtype=torch.int64)
    total, bad = torch.cat([incl[-1:], flag.to(torch.int64)]).tolist()                # the host read
    if bad & 2:
        raise ValueError("sample_surface: a face names a vertex outside [0, %d)" % nV)
    if bad & 1:
        raise L.PsdfError("sample_surface: a triangle is more than 30 000 x density long; subdivide it")
    if nV + total > 2 ** 31 - 1:
        raise L.PsdfError("sample_surface: %d points exceed the int32 point numbers of the later stages" % (nV + total))
    out = torch.empty((nV + total, 3), dtype=torch.float32, device=dev)
    out[:nV] = V
    if total:
        L.call("psdf_mesh_sample_emit", L.ptr(V), L.c_l(nV), L.ptr(F), L.c_l(nF), ctypes.c_double(density), L.ptr(incl),
               L.ptr(out[nV:]), L.stream())
    return out


@torch.no_grad()
def radius_thin(points, radius, order=None, generator=None, cell_budget=None, return_sweeps=False):
    """-> bool mask [N] in input order: the points the protocol's loop keeps when it walks the cloud in `order` (a permutation of
    0 .. N - 1: order[k] is the k-th point visited; default torch.randperm(N, generator=generator)) and every point still alive
    kills its neighbours within `radius`, inclusive.  With return_sweeps: (mask, sweeps)."""
    points = _cloud(points, "points")
    radius = fp32(float(radius))        # rounded once: the grid is planned with the radius the sweeps compare against
    if not radius >= 0.0:
        raise ValueError("radius must be >= 0")
    n, dev = points.shape[0], points.device
    if order is None:
        order = torch.randperm(n, generator=generator, device=generator.device if generator is not None else "cpu")
    order = torch.as_tensor(order).to(device=dev, dtype=torch.int64)
    if order.shape != (n,):
        raise ValueError("order must be a permutation of the %d points" % n)
    if n == 0:
        mask = torch.zeros(0, dtype=torch.bool, device=dev)
        return (mask, 0) if return_sweeps else mask
    in_range = (order >= 0) & (order < n)
    visits = torch.bincount(torch.where(in_range, order, 0), minlength=n)
    not_a_permutation = (visits != 1).sum() + (~in_range).sum()
    rank = torch.zeros(n, dtype=torch.int32, device=dev)
    rank[torch.where(in_range, order, 0)] = torch.arange(n, dtype=torch.int32, device=dev)
    grid = _Grid(points, radius, cell_budget, extra=(not_a_permutation,))
    if grid.extra[0] != 0:
        raise ValueError("order is not a permutation of 0 .. %d" % (n - 1))
    if grid.n_finite == 0:     # no point has a neighbour
        mask = torch.ones(n, dtype=torch.bool, device=dev)
        return (mask, 0) if return_sweeps else mask
    pts, keys, perm, start = grid.sort(points)
    rank_sorted = rank[perm].contiguous()
    state = torch.zeros(n, dtype=torch.uint8, device=dev)
    sweeps, before = 0, n + 1
    while True:
        undecided = torch.zeros(_SWEEPS_PER_READ, dtype=torch.int32, device=dev)
        for k in range(_SWEEPS_PER_READ):
            L.call("psdf_mesh_thin_sweep", L.ptr(pts), L.ptr(rank_sorted), L.ptr(keys), L.c_l(n), L.ptr(start), grid.origin_edge,
                   grid.dims, L.c_f(radius), L.ptr(state), L.ptr(undecided[k:k + 1]), L.stream())
        left = undecided.tolist()                                                       # the stage's host read
        done = [k for k, v in enumerate(left) if v == 0]
        if done:
            sweeps += done[0] + 1
            break
        # the undecided point of lowest rank decides in every sweep: a count that does not fall is a fault, not a slow case
        if left[-1] >= before:
            raise L.PsdfError("radius_thin: %d points stayed undecided over %d sweeps" % (left[-1], _SWEEPS_PER_READ))
        sweeps, before = sweeps + _SWEEPS_PER_READ, left[-1]
    mask = torch.empty(n, dtype=torch.bool, device=dev)
    mask[perm] = state == 1
    return (mask, sweeps) if return_sweeps else mask


@torch.no_grad()
def nearest(query, ref, max_dist, cell_budget=None, return_stats=False):
    """-> (dist [Q] fp32, idx [Q] int64): distance to the nearest point of `ref` and its row, or (max_dist, -1) where nothing is
    closer than max_dist, strictly.  A reference with a non-finite coordinate is never returned; such a query yields
    (max_dist, -1).  With return_stats: (dist, idx, nr_open): a [1] int32 device tensor, the queries the cooperative pass left to
    the ring search."""
    query, ref = _cloud(query, "query"), _cloud(ref, "ref")
    if query.device != ref.device:
        raise ValueError("query and ref live on different devices")
    max_dist = fp32(float(max_dist))
    if not max_dist >= 0.0:
        raise ValueError("max_dist must be >= 0")
    nq, nr, dev = query.shape[0], ref.shape[0], query.device
    dist = torch.full((nq,), max_dist, dtype=torch.float32, device=dev)
    idx = torch.full((nq,), -1, dtype=torch.int64, device=dev)
    nr_open = torch.zeros(1, dtype=torch.int32, device=dev)
    grid = _Grid(ref, 0.0, cell_budget) if nq and nr else None
    if grid is not None and grid.n_finite:
        refs, _, rperm, start = grid.sort(ref)
        qs, _, qperm, qstart = grid.sort(query, _BLOCK_LOG2)
        d = torch.full((nq,), max_dist, dtype=torch.float32, device=dev)
        at = torch.full((nq,), -1, dtype=torch.int32, device=dev)
        still = torch.zeros(nq, dtype=torch.uint8, device=dev)
        L.call("psdf_mesh_nn_cooperative", L.ptr(qs), L.c_l(nq), L.ptr(qstart), L.ptr(refs), L.c_l(nr), L.ptr(start),
               grid.origin_edge, grid.dims, L.c_f(max_dist), L.ptr(d), L.ptr(at), L.ptr(still), L.ptr(nr_open), L.stream())
        L.call("psdf_mesh_nn_ring", L.ptr(qs), L.c_l(nq), L.ptr(refs), L.c_l(nr), L.ptr(start), grid.origin_edge, grid.dims,
               L.c_f(max_dist), L.ptr(d), L.ptr(at), L.ptr(still), L.stream())
        dist[qperm] = d
        idx[qperm] = torch.where(at >= 0, rperm[at.clamp_min(0).to(torch.int64)], -1)
    return (dist, idx, nr_open) if return_stats else (dist, idx)


class ChamferResult:
    """mean_d2s (data -> scan), mean_s2d (scan -> data), overall = their average (Python floats; NaN for an empty selection);
    dist_d2s / dist_s2d: the distance vectors of the two queries (max_dist where nothing is closer); kept: the thinned cloud;
    data_in / data_in_obs: what the box and the observation mask leave of it; sweeps: thinning sweeps; nr_open: queries of both
    directions finished by the ring search"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return "ChamferResult(mean_d2s=%.6g, mean_s2d=%.6g, overall=%.6g)" % (self.mean_d2s, self.mean_s2d, self.overall)


def _mean_below(d, max_dist):
    return float(d[d < max_dist].double().mean()) if d.numel() else float("nan")


@torch.no_grad()
def chamfer_dtu(mesh_or_points, gt_points, density=0.2, max_dist=20.0, patch=60.0, obs_mask=None, bb=None, res=None, plane=None,
                generator=None, order=None):
    """The DTU protocol (eval.py:42-157) end to end.  `mesh_or_points`: an ExtractedMesh, a (V, F) pair, or a point cloud [N, 3].
    `bb` [2, 3]: the scan's box (filter p >= bb[0] - patch and p < bb[1] + 2 patch: the reference's asymmetry); `obs_mask`
    [X, Y, Z] bool with `res`: the observation mask at grid index round-half-even((p - bb[0]) / res), indices outside it dropped;
    `plane` [4]: scan points with plane . (x, 1) > 0 take part in scan -> data.  Each filter is skipped when its tensor is None.
    `order`: the shuffle (default torch.randperm from `generator`)."""
    if hasattr(mesh_or_points, "V") and hasattr(mesh_or_points, "F"):
        cloud = sample_surface(mesh_or_points.V, mesh_or_points.F, density)
    elif isinstance(mesh_or_points, (tuple, list)):
        cloud = sample_surface(mesh_or_points[0], mesh_or_points[1], density)
    else:
        cloud = _cloud(mesh_or_points, "points")
    gt = _cloud(gt_points, "gt_points")
    dev = cloud.device
    mask, sweeps = radius_thin(cloud, density, order=order, generator=generator, return_sweeps=True)
    kept = cloud[mask]
    data_in = kept
    if bb is not None:
        bb64 = torch.as_tensor(bb).to(device=dev, dtype=torch.float64).view(2, 3)
        p = kept.double()
        data_in = kept[((p >= bb64[0] - float(patch)) & (p < bb64[1] + 2.0 * float(patch))).all(1)]
    data_in_obs = data_in
    if obs_mask is not None:
        if bb is None or res is None:
            raise ValueError("obs_mask needs bb and res")
        obs = torch.as_tensor(obs_mask).to(device=dev, dtype=torch.bool)
        g = torch.round((data_in.double() - bb64[0]) / float(res)).to(torch.int64)
        shape = torch.tensor(obs.shape, dtype=torch.int64, device=dev)
        inside = ((g >= 0) & (g < shape)).all(1)
        g = g[inside]
        data_in_obs = data_in[inside][obs[g[:, 0], g[:, 1], g[:, 2]]]
    d2s, _, open_a = nearest(data_in_obs, gt, max_dist, return_stats=True)
    gt_above = gt
    if plane is not None:
        pl = torch.as_tensor(plane).to(device=dev, dtype=torch.float64).view(4)
        gt_above = gt[(gt.double() * pl[:3]).sum(1) + pl[3] > 0]
    s2d, _, open_b = nearest(gt_above, data_in, max_dist, return_stats=True)
    mean_d2s, mean_s2d = _mean_below(d2s, max_dist), _mean_below(s2d, max_dist)
    return ChamferResult(mean_d2s=mean_d2s, mean_s2d=mean_s2d, overall=(mean_d2s + mean_s2d) / 2, dist_d2s=d2s, dist_s2d=s2d,
                         kept=kept, kept_mask=mask, data_in=data_in, data_in_obs=data_in_obs, sweeps=sweeps,
                         nr_open=int(open_a) + int(open_b))
