"""The yardstick of the mesh-cleaning tests: numpy restatements, written out explicitly, of the lines of the reference that
permuto_sdf_amd/mesh_clean.py replaces -- permuto_sdf_py/experiments/evaluation/evaluate_chamfer_distance.py:110-167
(clean_points_by_mask, clean_mesh), create_my_meshes.py:72-75 and aabb.py:28-42.  OpenCV and trimesh are not available: the
ellipse and the face-adjacency rule are restated, and tests/test_mesh_clean_host.py pins the dilation and the components to
scipy.  Everything here is an integer or a boolean: the GPU tests compare exactly."""
import numpy as np


def ellipse_half_widths(ksize):
    """cv.getStructuringElement(cv.MORPH_ELLIPSE, (ksize, ksize)) as the half-width of every row (restated, unpinned)"""
    r = c = ksize // 2
    out = []
    for i in range(ksize):
        dy = i - r
        if r == 0 or abs(dy) > r:
            out.append(0)
            continue
        out.append(int(np.rint(c * np.sqrt((r * r - dy * dy) / (r * r)))))      # np.rint: half to even
    return out


def element_matrix(half_widths):
    """the structuring element as a 0 / 1 matrix with its anchor at the centre: row k covers the columns c - hw[k] .. c + hw[k]
    (len(hw) columns for an ellipse, whose half-widths never exceed len(hw) // 2; wider when a half-width does)"""
    k = len(half_widths)
    width = max(k, 2 * max(half_widths) + 1)
    m = np.zeros((k, width), dtype=bool)
    c = width // 2
    for i, h in enumerate(half_widths):
        m[i, c - h:c + h + 1] = True
    return m


def dilate(masks, half_widths):
    """masks [n, H, W] bool -> bool: out[y, x] iff some dy in -r .. r with y + dy inside the image and some |dx| <= hw[dy + r]
    with x + dx inside the image has masks[y + dy, x + dx] (cv.dilate with an anchor at the centre and nothing set outside)"""
    masks = np.asarray(masks, dtype=bool)
    n, H, W = masks.shape
    r = len(half_widths) // 2
    out = np.zeros_like(masks)
    cs = np.concatenate([np.zeros((n, H, 1), dtype=np.int32), np.cumsum(masks, axis=2, dtype=np.int32)], axis=2)   # cs[x] = sum [0, x)
    x = np.arange(W)
    for k, h in enumerate(half_widths):
        dy = k - r
        lo, hi = np.clip(x - h, 0, W), np.clip(x + h + 1, 0, W)
        row_hit = (cs[:, :, hi] - cs[:, :, lo]) > 0          # [n, H, W]: row y has a set pixel within h of column x
        # out[y] |= row_hit[y + dy]
        y0, y1 = max(0, -dy), min(H, H - dy)
        if y0 < y1:
            out[:, y0:y1] |= row_hit[:, y0 + dy:y1 + dy]
    return out


def threshold(masks, thr=128):
    masks = np.asarray(masks)
    return masks.copy() if masks.dtype == bool else masks > thr


def pack(bits):
    """[n, H, W] bool -> [n, H, ceil(W / 32)] int32: pixel x at bit x & 31 of word x >> 5"""
    n, H, W = bits.shape
    ww = (W + 31) // 32
    padded = np.zeros((n, H, ww * 32), dtype=np.uint64)
    padded[:, :, :W] = bits
    words = (padded.reshape(n, H, ww, 32) << np.arange(32, dtype=np.uint64)).sum(-1)
    return words.astype(np.uint32).view(np.int32)


def project(V, world_mats):
    """-> (u, v) [n, nV] float64, before rounding: p = ((P0 x + P1 y) + P2 z) + P3 per row, u = p0 / p2, v = p1 / p2"""
    V = np.asarray(V, dtype=np.float32).astype(np.float64)
    P = np.asarray(world_mats, dtype=np.float64)[:, :3, :]
    x, y, z = V[None, :, 0], V[None, :, 1], V[None, :, 2]
    with np.errstate(all="ignore"):
        p = [((P[:, k, 0, None] * x + P[:, k, 1, None] * y) + P[:, k, 2, None] * z) + P[:, k, 3, None] for k in range(3)]
        return p[0] / p[2], p[1] / p[2]


def inside_masks(V, world_mats, dilated):
    """clean_points_by_mask (evaluate_chamfer_distance.py:110-143) on masks already dilated and thresholded, [n, H, W] bool.  The
    reference adds 1 to the rounded pixel, pads the image with a border of ones and clips the index into the padded image: a
    vertex that projects outside the image reads a one.  A non-finite u or v is outside the image -- said here, not left to
    what a float-to-int cast makes of it."""
    dilated = np.asarray(dilated, dtype=bool)
    n, H, W = dilated.shape
    u, v = project(V, world_mats)
    keep = np.ones(u.shape[1], dtype=bool)
    for i in range(n):
        finite = np.isfinite(u[i]) & np.isfinite(v[i])
        ru = np.rint(np.where(finite, u[i], -1.0))
        rv = np.rint(np.where(finite, v[i], -1.0))
        inside = finite & (ru >= 0) & (ru < W) & (rv >= 0) & (rv < H)
        xi = np.where(inside, ru, 0).astype(np.int64)
        yi = np.where(inside, rv, 0).astype(np.int64)
        keep &= np.where(inside, dilated[i, yi, xi], True)
    return keep


def inside_box(V, lo, hi):
    V = np.asarray(V, dtype=np.float32)
    return ((V < np.asarray(hi, dtype=np.float32)) & (V > np.asarray(lo, dtype=np.float32))).all(1)


def filter_vertices(V, F, keep, NV=None):
    """evaluate_chamfer_distance.py:146-156 -> (V, F, vertex_map, face_keep[, NV])"""
    V, F, keep = np.asarray(V), np.asarray(F).reshape(-1, 3), np.asarray(keep, dtype=bool)
    vertex_map = np.full(len(V), -1, dtype=np.int32)
    vertex_map[keep] = np.arange(keep.sum(), dtype=np.int32)
    face_keep = keep[F[:, 0]] & keep[F[:, 1]] & keep[F[:, 2]] if len(F) else np.zeros(0, dtype=bool)
    out = (V[keep], vertex_map[F[face_keep]].astype(np.int32).reshape(-1, 3), vertex_map, face_keep)
    return out + (np.asarray(NV)[keep],) if NV is not None else out


def _components(n, pairs):
    """labels [n]: the smallest member of every node's component under the links `pairs`"""
    parent = list(range(n))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    for a, b in pairs:
        a, b = find(int(a)), find(int(b))
        if a != b:
            parent[max(a, b)] = min(a, b)
    return np.array([find(i) for i in range(n)], dtype=np.int32)


def edge_adjacency(F):
    """trimesh's face_adjacency, restated: the pairs of faces that own the two half-edges of an undirected edge which occurs
    exactly twice in the whole mesh; an edge with equal endpoints links nothing"""
    F = np.asarray(F, dtype=np.int64).reshape(-1, 3)
    nF = len(F)
    if nF == 0:
        return np.zeros((0, 2), dtype=np.int64)
    e = np.stack([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]], axis=1).reshape(-1, 2)       # slot 3 f + k
    e.sort(axis=1)
    owner = np.arange(3 * nF) // 3
    order = np.lexsort((e[:, 1], e[:, 0]))
    e, owner = e[order], owner[order]
    new = np.ones(len(e), dtype=bool)
    new[1:] = (e[1:] != e[:-1]).any(1)
    start = np.flatnonzero(new)
    length = np.diff(np.append(start, len(e)))
    twice = start[(length == 2) & (e[start, 0] != e[start, 1])]
    return np.stack([owner[twice], owner[twice + 1]], axis=1)


def face_components(F, nV, connectivity="edge"):
    """-> (labels [nF] int32: the smallest face of the component, sizes [nF] int32: faces per label, 0 elsewhere)"""
    F = np.asarray(F, dtype=np.int64).reshape(-1, 3)
    nF = len(F)
    if connectivity == "edge":
        labels = _components(nF, edge_adjacency(F))
    else:
        vertex_label = _components(nV, np.concatenate([F[:, [0, 1]], F[:, [0, 2]]]) if nF else [])
        first = np.full(nV, nF, dtype=np.int64)
        np.minimum.at(first, vertex_label[F[:, 0]], np.arange(nF))
        labels = first[vertex_label[F[:, 0]]].astype(np.int32)
    sizes = np.bincount(labels, minlength=nF).astype(np.int32) if nF else np.zeros(0, dtype=np.int32)
    return labels, sizes


def largest_component(V, F, connectivity="edge"):
    """Trimesh.split(only_watertight=False) and np.argmax over the face counts -> (V, F); the first of equal maxima is the one
    with the smallest label"""
    V, F = np.asarray(V), np.asarray(F).reshape(-1, 3)
    if len(F) == 0:
        return V[:0], F[:0].astype(np.int32)
    labels, sizes = face_components(F, len(V), connectivity)
    face_mask = labels == int(np.argmax(sizes))
    used = np.zeros(len(V), dtype=bool)
    used[F[face_mask].reshape(-1)] = True
    vertex_map = np.full(len(V), -1, dtype=np.int32)
    vertex_map[used] = np.arange(used.sum(), dtype=np.int32)
    return V[used], vertex_map[F[face_mask]].astype(np.int32)


def clean_mesh_dtu(V, F, world_mats, masks, ksize=101, thr=128, box=None, connectivity="edge"):
    """the chain -> (V, F, stats)"""
    V, F = np.asarray(V, dtype=np.float32), np.asarray(F).reshape(-1, 3)
    n0 = len(V)
    if box is not None:
        V, F = filter_vertices(V, F, inside_box(V, box[0], box[1]))[:2]
    n1 = len(V)
    dilated = dilate(threshold(masks, thr), ellipse_half_widths(ksize))
    V, F = filter_vertices(V, F, inside_masks(V, world_mats, dilated))[:2]
    n2 = len(V)
    _, sizes = face_components(F, len(V), connectivity)
    V, F = largest_component(V, F, connectivity)
    return V, F, {"removed_by_box": n0 - n1, "removed_by_masks": n1 - n2, "components": int((sizes > 0).sum()), "faces": len(F)}
