"""Float64 restatement of the three stages of the DTU Chamfer protocol (numpy only, no torch): the yardstick of
tests/test_gpu_mesh_eval.py, itself pinned to sklearn's NearestNeighbors -- the library the protocol uses -- by
tests/test_mesh_eval_host.py.

  * sample_surface: the lattice of every triangle, decisions and positions in float64 from the fp32 corners;
  * radius_thin: the sequential loop (a point still alive kills every neighbour with d <= radius), in the given order;
  * nearest: brute force in row chunks.
Large clouds (the end-to-end case) may take the pair list / the nearest neighbour from scipy's KD-tree instead of the O(N^2)
loops (`tree=True`); test_mesh_eval_host.py checks that both routes give the same answer."""
import numpy as np

U = 2.0 ** -24


def triangle_lattice(V, F, density):
    """per triangle: n1, n2 (float64; -1 where the triangle emits nothing) and the relative distance of l1 / s, l2 / s from the
    nearest integer (inf where there is no lattice)"""
    V = np.asarray(V, dtype=np.float32).astype(np.float64)
    F = np.asarray(F).astype(np.int64)
    p0, e1, e2 = V[F[:, 0]], V[F[:, 1]] - V[F[:, 0]], V[F[:, 2]] - V[F[:, 0]]
    l1 = np.sqrt(e1[:, 0] * e1[:, 0] + e1[:, 1] * e1[:, 1] + e1[:, 2] * e1[:, 2])
    l2 = np.sqrt(e2[:, 0] * e2[:, 0] + e2[:, 1] * e2[:, 1] + e2[:, 2] * e2[:, 2])
    c = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                  e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
    A2 = np.sqrt(c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1] + c[:, 2] * c[:, 2])
    ok = A2 > 0
    n1, n2 = np.full(len(F), -1.0), np.full(len(F), -1.0)
    margin = np.full(len(F), np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = float(density) * np.sqrt(l1 * l2 / A2)
        r1, r2 = l1 / s, l2 / s
    n1[ok], n2[ok] = np.floor(r1[ok]), np.floor(r2[ok])
    for r in (r1, r2):
        margin[ok] = np.minimum(margin[ok], np.abs(r[ok] - np.round(r[ok])) / np.maximum(np.abs(r[ok]), 1.0))
    return p0, e1, e2, n1, n2, margin


def sample_surface(V, F, density):
    """-> (cloud [V + S, 3] float64: the vertices, then the samples triangle by triangle, i-major, j-minor; counts [F]; margin [F])"""
    V32 = np.asarray(V, dtype=np.float32)
    p0, e1, e2, n1, n2, margin = triangle_lattice(V32, F, density)
    out, counts = [V32.astype(np.float64).reshape(-1, 3)], np.zeros(len(n1), dtype=np.int64)
    for f in range(len(n1)):
        if n1[f] < 0:
            continue
        a = (np.arange(int(n1[f]) + 1, dtype=np.float64) + 0.5) / max(n1[f], 1e-7)
        b = (np.arange(int(n2[f]) + 1, dtype=np.float64) + 0.5) / max(n2[f], 1e-7)
        A, B = np.meshgrid(a, b, indexing="ij")
        keep = (A + B) < 1
        A, B = A[keep][:, None], B[keep][:, None]           # boolean indexing walks row-major: i-major, j-minor
        out.append((e1[f][None] * A + e2[f][None] * B) + p0[f][None])
        counts[f] = len(A)
    return np.concatenate(out, 0), counts, margin


def pair_distances_min_gap(points, radius, chunk=1024):
    """min over pairs of |d - radius| (float64): how far the cloud is from a coin toss at this radius"""
    p = np.asarray(points, dtype=np.float64)
    gap = np.inf
    for a in range(0, len(p), chunk):
        d = np.sqrt(((p[a:a + chunk, None, :] - p[None, :, :]) ** 2).sum(2))
        rows = np.arange(a, min(a + chunk, len(p)))
        d[rows - a, rows] = np.inf
        gap = min(gap, float(np.abs(d - radius).min())) if d.size else gap
    return gap


def _neighbour_lists(p, radius, tree, chunk=1024):
    n = len(p)
    if tree:
        from scipy.spatial import cKDTree
        pairs = cKDTree(p).query_pairs(radius * (1 + 1e-9), output_type="ndarray")
        d = np.sqrt(((p[pairs[:, 0]] - p[pairs[:, 1]]) ** 2).sum(1))
        pairs = pairs[d <= radius]
        src = np.concatenate([pairs[:, 0], pairs[:, 1]])
        dst = np.concatenate([pairs[:, 1], pairs[:, 0]])
        o = np.argsort(src, kind="stable")
        src, dst = src[o], dst[o]
        first = np.searchsorted(src, np.arange(n + 1))
        return [dst[first[i]:first[i + 1]] for i in range(n)]
    lists = []
    for a in range(0, n, chunk):
        d = np.sqrt(((p[a:a + chunk, None, :] - p[None, :, :]) ** 2).sum(2))
        lists.extend(np.nonzero(row <= radius)[0] for row in d)
    return lists


def radius_thin(points, radius, order, tree=False):
    """-> bool mask in input order: eval.py's loop over the cloud visited in `order` (order[k] = k-th point visited)"""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    order = np.asarray(order, dtype=np.int64)
    lists = _neighbour_lists(p, float(radius), tree)
    mask = np.ones(len(p), dtype=bool)
    for cur in order:
        if mask[cur]:
            mask[lists[cur]] = False
            mask[cur] = True
    return mask


def nearest(query, ref, chunk=512, tree=False):
    """-> (d [Q] float64, idx [Q]) without a cut-off; (inf, -1) for no references"""
    q = np.asarray(query, dtype=np.float64).reshape(-1, 3)
    r = np.asarray(ref, dtype=np.float64).reshape(-1, 3)
    if len(r) == 0:
        return np.full(len(q), np.inf), np.full(len(q), -1, dtype=np.int64)
    if tree:
        from scipy.spatial import cKDTree
        d, i = cKDTree(r).query(q, k=1)
        return np.sqrt(((q - r[i]) ** 2).sum(1)), i.astype(np.int64)
    d, i = np.empty(len(q)), np.empty(len(q), dtype=np.int64)
    for a in range(0, len(q), chunk):
        D = ((q[a:a + chunk, None, :] - r[None, :, :]) ** 2).sum(2)
        i[a:a + chunk] = D.argmin(1)
        d[a:a + chunk] = np.sqrt(D[np.arange(D.shape[0]), i[a:a + chunk]])
    return d, i


def chamfer_dtu(cloud, gt, order, density, max_dist, patch=60.0, obs_mask=None, bb=None, res=None, plane=None, tree=True):
    """the protocol from the sampled cloud on; -> dict with the index sets (into `cloud` / `gt`) and the two means"""
    cloud, gt = np.asarray(cloud, dtype=np.float64), np.asarray(gt, dtype=np.float64)
    keep = radius_thin(cloud, density, order, tree=tree)
    kept = np.nonzero(keep)[0]
    inb = kept
    if bb is not None:
        bb = np.asarray(bb, dtype=np.float64).reshape(2, 3)
        p = cloud[kept]
        inb = kept[((p >= bb[0] - patch) & (p < bb[1] + 2 * patch)).all(1)]
    obs = inb
    if obs_mask is not None:
        g = np.around((cloud[inb] - bb[0]) / res).astype(np.int64)        # numpy rounds half to even
        inside = ((g >= 0) & (g < np.array(obs_mask.shape)[None])).all(1)
        g = g[inside]
        obs = inb[inside][np.asarray(obs_mask, dtype=bool)[g[:, 0], g[:, 1], g[:, 2]]]
    above = np.arange(len(gt))
    if plane is not None:
        pl = np.asarray(plane, dtype=np.float64).reshape(4)
        above = np.nonzero((gt * pl[None, :3]).sum(1) + pl[3] > 0)[0]
    d2s, _ = nearest(cloud[obs], gt, tree=tree)
    s2d, _ = nearest(gt[above], cloud[inb], tree=tree)
    with np.errstate(invalid="ignore"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            m1 = d2s[d2s < max_dist].mean() if len(d2s) else np.nan
            m2 = s2d[s2d < max_dist].mean() if len(s2d) else np.nan
    return {"kept": kept, "data_in": inb, "data_in_obs": obs, "gt_above": above, "d2s": d2s, "s2d": s2d, "mean_d2s": float(m1),
            "mean_s2d": float(m2)}
