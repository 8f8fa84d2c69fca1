"""GPU: the mesh cleaning between extraction and scoring (permuto_sdf_amd/mesh_clean.py, csrc/mesh_clean.hip) against the numpy
restatement tests/mesh_clean_reference.py (pinned to scipy by tests/test_mesh_clean_host.py).  Every result is an integer or a
boolean: every comparison is exact.  The one place where floating point decides is the rounding of a projected coordinate; the
vertex test first asserts, from the yardstick alone, that no coordinate lies within 1e-8 px of k + 1/2."""
import numpy as np
import pytest
import torch

from tests import mesh_clean_reference as ref

pytestmark = pytest.mark.gpu
H, W = 150, 200


def gpu(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ------------------------------------------------------------------------------------------------------------- dilation
def sparse_masks(seed, n, h, w, share):
    r = np.random.default_rng(seed)
    m = r.random((n, h, w)) < share
    m[:, 0, 0] = m[:, 0, -1] = m[:, -1, 0] = m[:, -1, -1] = True              # the four corners
    m[:, 0, w // 2] = m[:, -1, w // 3] = m[:, h // 2, 0] = m[:, h // 3, -1] = True    # every border
    return m


def check_dilation(dev, masks_u8, half_widths, threshold=128):
    from permuto_sdf_amd import mesh_clean as mc
    want = ref.dilate(ref.threshold(masks_u8, threshold), half_widths)
    packed = mc.dilate_masks(gpu(masks_u8, dev), half_widths, threshold)
    n, h, w = masks_u8.shape
    assert (packed.H, packed.W) == (h, w) and packed.words.dtype == torch.int32
    assert tuple(packed.words.shape) == (n, h, (w + 31) // 32)
    assert np.array_equal(packed.words.cpu().numpy(), ref.pack(want))          # the padding bits included: zero
    assert np.array_equal(packed.unpack().cpu().numpy(), want)
    return want


@pytest.mark.parametrize("ksize", [1, 3, 21, 101])
def test_dilation_of_sparse_masks(dev, ksize):
    """101 rows are taller than the halo a 150-row image can supply: the clipping case"""
    m = sparse_masks(0, 3, H, W, 0.002)
    want = check_dilation(dev, np.where(m, 255, 0).astype(np.uint8), ref.ellipse_half_widths(ksize))
    assert want.any() and (ksize == 1) == np.array_equal(want, m)


@pytest.mark.parametrize("shape", [(1, 1), (1, 65), (7, 31), (7, 32), (7, 33), (70, 64)])
@pytest.mark.parametrize("ksize", [5, 21])
def test_dilation_shapes(dev, shape, ksize):
    r = np.random.default_rng(shape[0] * 100 + shape[1])
    m = r.random((2,) + shape) < 0.03
    m[:, 0, 0] = m[:, -1, -1] = True
    check_dilation(dev, np.where(m, 200, 17).astype(np.uint8), ref.ellipse_half_widths(ksize))


def test_dilation_all_clear_all_set_threshold_and_bool(dev):
    from permuto_sdf_amd import mesh_clean as mc
    hw = ref.ellipse_half_widths(7)
    clear = check_dilation(dev, np.zeros((1, 9, 70), dtype=np.uint8), hw)
    full = check_dilation(dev, np.full((2, 9, 70), 255, dtype=np.uint8), hw)
    assert not clear.any() and full.all()
    # 128 is clear and 129 is set under the default threshold
    m = sparse_masks(5, 2, 40, 70, 0.004)
    u8 = np.where(m, 129, 128).astype(np.uint8)
    want = check_dilation(dev, u8, hw)
    assert want.any() and not want.all()
    assert not mc.dilate_masks(gpu(np.full((1, 9, 70), 128, dtype=np.uint8), dev), hw).words.any()
    # a bool tensor: set when true, whatever the threshold argument
    packed = mc.dilate_masks(gpu(m, dev), hw, threshold=200)
    assert np.array_equal(packed.unpack().cpu().numpy(), want)
    # an element wider than tall, and a row distance beyond the byte's range
    wide = np.zeros((1, 5, 600), dtype=np.uint8)
    wide[0, 2, 10] = wide[0, 4, 599] = 255
    check_dilation(dev, wide, [254, 3, 100])
    with pytest.raises(ValueError):
        mc.dilate_masks(gpu(wide, dev), [0, 255, 0])
    with pytest.raises(ValueError):
        mc.dilate_masks(gpu(wide, dev), [0, 1])


# ----------------------------------------------------------------------------------------------------------- vertex test
def look_at(c):
    """world -> camera rotation and translation of a camera at c looking at the origin"""
    c = np.asarray(c, dtype=np.float64)
    z = -c / np.linalg.norm(c)
    up = np.array([0.0, 1.0, 0.0]) if abs(z[1]) < 0.9 else np.array([1.0, 0.0, 0.0])
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    return R, -R @ c


def pinhole_views(centres, focal, h, w):
    """world_mat [n, 4, 4] = K [R | t], as in cameras_sphere.npz"""
    P = np.zeros((len(centres), 4, 4))
    K = np.array([[focal, 0, w / 2], [0, focal, h / 2], [0, 0, 1.0]])
    for i, c in enumerate(centres):
        R, t = look_at(c)
        P[i, :3, :3], P[i, :3, 3], P[i, 3, 3] = K @ R, K @ t, 1.0
    return P


def view_centres(n, distance, seed):
    r = np.random.default_rng(seed)
    d = r.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[0] = [0, 0, -1]                     # view 0 on the axis: its matrix is exact, p2 = z + distance
    return d * distance


FOCAL = 250.0


@pytest.fixture(scope="module")
def vertex_case():
    P = pinhole_views(view_centres(8, 2.5, 1), FOCAL, H, W)
    assert np.array_equal(P[0, 2], [0, 0, 1, 2.5])
    r = np.random.default_rng(0)
    V = r.uniform(-0.5, 0.5, (20000, 3)).astype(np.float32)
    at = lambda u, v: [(u - W / 2) * 2.5 / FOCAL, (v - H / 2) * 2.5 / FOCAL, 0.0]      # noqa: E731  (view 0, z = 0)
    extra = np.array([
        [0.0, 0.0, -5.0],                      # behind camera 0
        [0.1, 0.2, -2.5],                      # p2 == 0 exactly in view 0
        [np.nan, 0.0, 0.0], [0.0, np.inf, 0.0],
        [1e30, -1e30, 1e30],
        at(-0.6, 70), at(-0.4, 70), at(W - 0.4, 70), at(W - 0.6, 70),      # just outside / inside the left and right edges
        at(90, -0.6), at(90, -0.4), at(90, H - 0.4), at(90, H - 0.6),      # ... the top and bottom edges
    ], dtype=np.float32)
    V = np.concatenate([V, extra])
    blobs = ref.dilate(np.random.default_rng(2).random((8, H, W)) < 0.0004, ref.ellipse_half_widths(41))
    masks = np.where(blobs, 255, 0).astype(np.uint8)
    dilated = ref.dilate(blobs, ref.ellipse_half_widths(21))
    return {"P": P, "V": V, "masks": masks, "dilated": dilated, "want": ref.inside_masks(V, P, dilated), "extra": len(extra)}


def test_vertex_case_is_decidable_and_exercises_both_outcomes(vertex_case):
    """from the yardstick alone: no projected coordinate within 1e-8 px of k + 1/2 (a closer one is a coin toss for any summation
    order), and every view both keeps and culls"""
    c = vertex_case
    u, v = ref.project(c["V"], c["P"])
    closest = np.inf
    for t in (u, v):
        t = t[np.isfinite(t)]
        closest = min(closest, np.abs(t - np.floor(t) - 0.5).min())
    print("closest projected coordinate to a half pixel: %.3g px" % closest)
    assert closest >= 1e-8
    nr = 20000
    for i in range(8):
        one = ref.inside_masks(c["V"][:nr], c["P"][i:i + 1], c["dilated"][i:i + 1])
        assert 0 < one.sum() < nr, i
    assert 0 < c["want"][:nr].sum() < nr
    # the edge vertices land where they were aimed in view 0
    e = len(c["V"]) - 8
    assert np.rint(u[0, e:e + 4]).tolist() == [-1, 0, W, W - 1] and np.rint(v[0, e + 4:]).tolist() == [-1, 0, H, H - 1]


def test_vertex_test_equals_the_yardstick(dev, vertex_case):
    from permuto_sdf_amd import mesh_clean as mc
    c = vertex_case
    packed = mc.dilate_masks(gpu(c["masks"], dev), mc.ellipse_half_widths(21))
    assert np.array_equal(packed.unpack().cpu().numpy(), c["dilated"])
    V, P = gpu(c["V"], dev), gpu(c["P"], dev)
    got = mc.inside_masks(V, P, packed)
    assert got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), c["want"])
    assert np.array_equal(mc.inside_masks(V, P[:, :3].contiguous(), packed).cpu().numpy(), c["want"])
    assert np.array_equal(mc.inside_masks(V, c["P"], packed).cpu().numpy(), c["want"])      # a numpy array of matrices
    for i in range(8):      # every view by itself: the AND hides no view's decision (the vertices aimed at view 0's edges among them)
        one = mc.inside_masks(V, P[i:i + 1], mc.PackedMasks(packed.words[i:i + 1].contiguous(), H, W))
        assert np.array_equal(one.cpu().numpy(), ref.inside_masks(c["V"], c["P"][i:i + 1], c["dilated"][i:i + 1])), i
    tail = c["V"][-c["extra"]:]
    for nV in (0, 1, 63, 64, 65):
        part = np.concatenate([tail, c["V"]])[:nV]
        assert np.array_equal(mc.inside_masks(gpu(part, dev), P, packed).cpu().numpy(), ref.inside_masks(part, c["P"], c["dilated"]))
    with pytest.raises(ValueError):
        mc.inside_masks(V, P[:5], packed)


def test_inside_box_is_strict(dev):
    from permuto_sdf_amd import mesh_clean as mc
    V = np.array([[0, 0, 0], [0.5, 0, 0], [-0.5, 0, 0], [0.49999, 0.49999, -0.49999], [0, 0.6, 0], [np.nan, 0, 0]], dtype=np.float32)
    lo, hi = [-0.5] * 3, [0.5] * 3
    want = ref.inside_box(V, lo, hi)
    assert want.tolist() == [True, False, False, True, False, False]
    assert np.array_equal(mc.inside_box(gpu(V, dev), lo, hi).cpu().numpy(), want)


# ----------------------------------------------------------------------------------------------------------------- filter
def test_filter_equals_the_yardstick(dev):
    from permuto_sdf_amd import mesh_clean as mc
    from permuto_sdf_amd.mesh import ExtractedMesh
    r = np.random.default_rng(4)
    nV, nF = 5000, 10000
    V = r.standard_normal((nV, 3)).astype(np.float32)
    NV = r.standard_normal((nV, 3)).astype(np.float32)
    edges = r.integers(0, 2 ** 40, (nV, 2))
    F = r.integers(0, nV, (nF, 3)).astype(np.int32)
    keep = r.random(nV) < 0.9
    Vw, Fw, map_w, face_w, NVw = ref.filter_vertices(V, F, keep, NV)
    assert 0 < len(Fw) < nF
    mesh = ExtractedMesh(gpu(V, dev), gpu(F, dev), gpu(NV, dev), edges=gpu(edges, dev), nr_evaluated=7)
    out = mc.filter_vertices(mesh, gpu(keep, dev))
    assert np.array_equal(out.V.cpu().numpy(), Vw) and np.array_equal(out.F.cpu().numpy(), Fw)
    assert out.F.dtype == torch.int32 and out.vertex_map.dtype == torch.int32 and out.face_keep.dtype == torch.bool
    assert np.array_equal(out.vertex_map.cpu().numpy(), map_w) and np.array_equal(out.face_keep.cpu().numpy(), face_w)
    assert np.array_equal(out.NV.cpu().numpy(), NVw) and np.array_equal(out.edges.cpu().numpy(), edges[keep])
    assert out.nr_evaluated == 7
    # a (V, F) pair; keep-all is the identity; keep-none is empty
    same = mc.filter_vertices((gpu(V, dev), gpu(F, dev)), torch.ones(nV, dtype=torch.bool, device=dev))
    assert np.array_equal(same.V.cpu().numpy(), V) and np.array_equal(same.F.cpu().numpy(), F) and same.NV is None
    assert np.array_equal(same.vertex_map.cpu().numpy(), np.arange(nV)) and bool(same.face_keep.all())
    none = mc.filter_vertices(mesh, torch.zeros(nV, dtype=torch.bool, device=dev))
    assert tuple(none.V.shape) == (0, 3) and tuple(none.F.shape) == (0, 3) and tuple(none.NV.shape) == (0, 3)
    assert bool((none.vertex_map == -1).all()) and not bool(none.face_keep.any())
    empty = mc.filter_vertices((gpu(V[:0], dev), gpu(F[:0], dev)), torch.zeros(0, dtype=torch.bool, device=dev))
    assert tuple(empty.V.shape) == (0, 3) and tuple(empty.F.shape) == (0, 3)
    bad = F.copy()
    bad[77, 1] = nV
    with pytest.raises(ValueError):
        mc.filter_vertices((gpu(V, dev), gpu(bad, dev)), gpu(keep, dev))
    with pytest.raises(ValueError):
        mc.filter_vertices(mesh, gpu(keep[:-1], dev))


# ------------------------------------------------------------------------------------------------------------- components
def strip(n, seed=None):
    order = np.arange(n) if seed is None else np.random.default_rng(seed).permutation(n)
    return np.stack([order, order + 1, order + 2], 1).astype(np.int32)


def soup(seed, nF):
    return np.random.default_rng(seed).integers(0, nF // 2 + 3, (nF, 3)).astype(np.int32)


COMPONENT_CASES = {
    "strip": (strip(20000, 3), 20002),                                                       # deep chains
    "fan": (np.stack([np.zeros(300, dtype=np.int64), np.arange(300) + 1, np.arange(300) + 2], 1).astype(np.int32), 302),
    "bow-tie": (np.array([[0, 1, 2], [2, 3, 4]], dtype=np.int32), 5),
    "three-on-an-edge": (np.array([[0, 1, 2], [0, 1, 3], [1, 0, 4]], dtype=np.int32), 5),
    "identical": (np.array([[0, 1, 2], [0, 1, 2], [4, 5, 6]], dtype=np.int32), 7),
    "equal-indices": (np.array([[0, 0, 1], [0, 1, 2], [3, 3, 3], [1, 2, 4]], dtype=np.int32), 5),
    "disjoint": (np.arange(1500, dtype=np.int32).reshape(500, 3), 1500),
    "empty": (np.zeros((0, 3), dtype=np.int32), 4),
}
COMPONENT_CASES.update({"soup%d" % n: (soup(n, n), n // 2 + 3) for n in (1, 63, 64, 65, 257)})
_component_reference = {}


def component_reference(name, connectivity):
    key = (name, connectivity)
    if key not in _component_reference:
        F, nV = COMPONENT_CASES[name]
        _component_reference[key] = ref.face_components(F, nV, connectivity)
    return _component_reference[key]


@pytest.mark.parametrize("connectivity", ["edge", "vertex"])
@pytest.mark.parametrize("name", sorted(COMPONENT_CASES))
def test_components_equal_the_yardstick(dev, name, connectivity):
    from permuto_sdf_amd import mesh_clean as mc
    F, nV = COMPONENT_CASES[name]
    labels_w, sizes_w = component_reference(name, connectivity)
    labels, sizes, flag = mc.face_components(gpu(F, dev), nV, connectivity, return_flag=True)
    assert flag == 0                                                          # no loop met its cap, every face in range
    assert labels.dtype == torch.int32 and sizes.dtype == torch.int32
    assert np.array_equal(labels.cpu().numpy(), labels_w) and np.array_equal(sizes.cpu().numpy(), sizes_w)
    by_hand = {("bow-tie", "edge"): 2, ("bow-tie", "vertex"): 1, ("three-on-an-edge", "edge"): 3, ("identical", "edge"): 2,
               ("strip", "edge"): 1, ("strip", "vertex"): 1, ("fan", "edge"): 1, ("disjoint", "edge"): 500, ("disjoint", "vertex"): 500,
               ("equal-indices", "edge"): 3, ("equal-indices", "vertex"): 2}
    if (name, connectivity) in by_hand:
        assert int((sizes_w > 0).sum()) == by_hand[(name, connectivity)]


def test_components_refuse_a_face_out_of_range_and_an_unknown_connectivity(dev):
    from permuto_sdf_amd import mesh_clean as mc
    F = gpu(np.array([[0, 1, 2], [1, 2, 5]], dtype=np.int32), dev)
    for connectivity in ("edge", "vertex"):
        with pytest.raises(ValueError):
            mc.face_components(F, 5, connectivity)
    with pytest.raises(ValueError):
        mc.face_components(F, 6, "corner")


def test_largest_component_order_ties_and_unreferenced_vertices(dev):
    from permuto_sdf_amd import mesh_clean as mc
    r = np.random.default_rng(9)
    # a strip of 40 faces and one of 25 interleaved face by face, two stray vertices, a lone triangle
    a, b = strip(40), strip(25) + 50
    F = np.concatenate([np.stack([a[:25], b], 1).reshape(-1, 3), a[25:], [[90, 91, 92]]]).astype(np.int32)
    V = r.standard_normal((95, 3)).astype(np.float32)
    for connectivity in ("edge", "vertex"):
        Vw, Fw = ref.largest_component(V, F, connectivity)
        out = mc.largest_component((gpu(V, dev), gpu(F, dev)), connectivity)
        assert np.array_equal(out.V.cpu().numpy(), Vw) and np.array_equal(out.F.cpu().numpy(), Fw)
        assert len(Vw) == 42 and np.array_equal(Fw, a)
    # a tie between the two largest goes to the smaller label: faces 1 and 2 form one pair, faces 0 and 3 the other
    T = np.array([[0, 1, 2], [10, 11, 12], [11, 12, 13], [1, 2, 3]], dtype=np.int32)
    Vt = r.standard_normal((14, 3)).astype(np.float32)
    out = mc.largest_component((gpu(Vt, dev), gpu(T, dev)))
    Vw, Fw = ref.largest_component(Vt, T)
    assert np.array_equal(out.V.cpu().numpy(), Vw) and np.array_equal(out.F.cpu().numpy(), Fw)
    assert np.array_equal(Vw, Vt[:4]) and Fw.tolist() == [[0, 1, 2], [1, 2, 3]]
    # faces of another component whose vertices all belong to the largest do not come along: a cone around vertex 0 and its
    # base twice over -- the base's edges occur three times and link nothing under "edge"
    X = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 1], [1, 2, 3], [1, 2, 3]], dtype=np.int32)
    Vx = r.standard_normal((5, 3)).astype(np.float32)
    out = mc.largest_component((gpu(Vx, dev), gpu(X, dev)))
    Vw, Fw = ref.largest_component(Vx, X)
    assert np.array_equal(out.V.cpu().numpy(), Vw) and np.array_equal(out.F.cpu().numpy(), Fw)
    assert np.array_equal(Fw, X[:3]) and len(Vw) == 4
    empty = mc.largest_component((gpu(Vx, dev), gpu(X[:0], dev)))
    assert tuple(empty.V.shape) == (0, 3) and tuple(empty.F.shape) == (0, 3)


# -------------------------------------------------------------------------------------------------------------- end to end
BIG, SMALL, BLOB = ((0.0, 0.0, 0.0), 0.5), ((0.0, 0.78, 0.0), 0.12), ((-0.72, -0.7, 0.66), 0.1)
E2E_FOCAL, E2E_KSIZE = 150.0, 11


def silhouettes(P_centres, spheres, focal, h, w):
    """[n, h, w] uint8: 255 where the pixel's ray meets one of the spheres"""
    out = np.zeros((len(P_centres), h, w), dtype=np.uint8)
    vv, uu = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    for i, c in enumerate(P_centres):
        R, _ = look_at(c)
        d = np.stack([(uu - w / 2) / focal, (vv - h / 2) / focal, np.ones_like(uu, dtype=np.float64)], -1) @ R     # camera -> world
        d /= np.linalg.norm(d, axis=-1, keepdims=True)
        for centre, radius in spheres:
            oc = np.asarray(centre) - c
            along = d @ oc
            out[i][(along > 0) & ((oc @ oc) - along ** 2 <= radius ** 2)] = 255
    return out


@pytest.fixture(scope="module")
def e2e_case(dev):
    from permuto_sdf_amd.mesh import marching_tetrahedra
    n = 48
    h = 2.0 / (n - 1)
    g = torch.linspace(-1.0, 1.0, n, device=dev)
    x, y, z = torch.meshgrid(g, g, g, indexing="ij")
    sdf = None
    for (cx, cy, cz), radius in (BIG, SMALL, BLOB):
        s = torch.sqrt((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2) - radius
        sdf = s if sdf is None else torch.minimum(sdf, s)
    verts, F, normals, _ = marching_tetrahedra(sdf, 0.0, spacing=(h, h, h))
    V = (verts - 1.0).contiguous()
    centres = view_centres(6, 2.5, 7)
    P = pinhole_views(centres, E2E_FOCAL, H, W)
    masks = silhouettes(centres, (BIG, SMALL), E2E_FOCAL, H, W)
    return {"V": V, "F": F, "NV": -normals, "P": P, "masks": masks, "Vn": V.cpu().numpy(), "Fn": F.cpu().numpy()}


@pytest.mark.parametrize("box", [None, ([-0.6] * 3, [0.6] * 3)], ids=["masks", "box-and-masks"])
def test_clean_mesh_dtu_end_to_end(dev, e2e_case, box, tmp_path):
    from permuto_sdf_amd import mesh_clean as mc
    from permuto_sdf_amd import mesh_eval as me
    from permuto_sdf_amd.mesh import ExtractedMesh
    c = e2e_case
    Vw, Fw, stats_w = ref.clean_mesh_dtu(c["Vn"], c["Fn"], c["P"], c["masks"], ksize=E2E_KSIZE, box=box)
    # the scene is what it is meant to be: three pieces, the masks remove (at least part of) the blob and spare the spheres
    _, sizes0 = ref.face_components(c["Fn"], len(c["Vn"]))
    assert (sizes0 > 0).sum() == 3
    if box is None:
        assert stats_w["removed_by_box"] == 0 and stats_w["removed_by_masks"] > 0 and stats_w["components"] >= 2
    else:
        assert stats_w["removed_by_box"] > 0 and stats_w["components"] == 1
    radius = np.linalg.norm(Vw, axis=1)
    assert len(Fw) == sizes0.max() and np.abs(radius - 0.5).max() < 0.02          # the large sphere alone, whole
    mesh = ExtractedMesh(c["V"], c["F"], c["NV"])
    out = mc.clean_mesh_dtu(mesh, gpu(c["P"], dev), gpu(c["masks"], dev), ksize=E2E_KSIZE, box=box)
    assert np.array_equal(out.V.cpu().numpy(), Vw) and np.array_equal(out.F.cpu().numpy(), Fw)
    assert out.stats == stats_w
    assert out.NV is not None and tuple(out.NV.shape) == tuple(out.V.shape)
    # the result feeds the scorer and the writer unchanged
    gt = np.random.default_rng(0).standard_normal((4000, 3))
    gt = (0.5 * gt / np.linalg.norm(gt, axis=1, keepdims=True)).astype(np.float32)
    score = me.chamfer_dtu(out, gpu(gt, dev), density=0.05, max_dist=1.0, generator=torch.Generator().manual_seed(0))
    assert 0.0 < score.overall < 0.05
    path = str(tmp_path / "clean.ply")
    out.save_ply(path)
    with open(path, "rb") as f:
        head = f.read(200).decode("ascii", "replace")
    assert "element vertex %d" % len(Vw) in head and "element face %d" % len(Fw) in head
