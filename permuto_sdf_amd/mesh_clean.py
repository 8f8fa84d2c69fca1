"""Mesh cleaning on the device: mask culling and the largest component (csrc/mesh_clean.hip).

Between extraction and scoring the reference cleans its meshes.  permuto_sdf_py/experiments/evaluation/create_my_meshes.py:72-75
removes the vertices outside the scene's box; for scenes trained without masks, evaluate_chamfer_distance.py:110-167
(clean_points_by_mask, clean_mesh: NeuS's published protocol) projects every vertex into every training view, drops a vertex that
falls outside any view's mask dilated by a 101 x 101 ellipse, drops the faces that lost a vertex, renumbers, and keeps the largest
connected component.  Here, on tensors `MeshExtractor` leaves on the device:

  * `ellipse_half_widths(ksize)`                   the row spans of OpenCV's MORPH_ELLIPSE (restated, unpinned against cv2);
  * `dilate_masks(masks, half_widths, threshold)`  threshold and dilate -> bit-packed masks (row distance, span dilation);
  * `inside_masks(V, world_mats, packed)`          clean_points_by_mask: the AND over the views of the projected lookups;
  * `inside_box(V, lo, hi)`                        aabb.py:28-42, strict on both sides (plain torch: it is not hot);
  * `filter_vertices(mesh, keep)`                  remove vertices, the faces that lost one, renumber (count -> scan -> emit);
  * `face_components(F, nV, connectivity)`         labels and sizes of the face components (sort + union-find);
  * `largest_component(mesh, connectivity)`        Trimesh.split(only_watertight=False) and the argmax over the face counts;
  * `clean_mesh_dtu(mesh, world_mats, masks, ..)`  the chain; its result feeds `chamfer_dtu` and `save_ply` unchanged.

Out of scope: reading `.npz`, `.png` or `.ply` files; trimesh's `process=True` vertex merge (the extractor's meshes are already
welded); the DTU frame transform.  Two rules are restated from the libraries' published behaviour because neither library is
available to the tests: OpenCV's ellipse and trimesh's face adjacency -- an edge links two faces iff it occurs in exactly two
half-edges of the whole mesh (`group_rows(..., require_count=2)`).  Both are unpinned.

Host reads: `dilate_masks` and `inside_masks` none; `filter_vertices` one (the two totals and the error flag);
`face_components` one (the error flag); `largest_component` two (face_components' and filter's); `clean_mesh_dtu` one per
filter it runs, face_components' and one for the statistics.
"""
import math

import torch

from . import _lib as L
from .mesh import ExtractedMesh

_PLAN_FIELDS = 9            # include/psdf.h: PSDF_MESH_CLEAN_PLAN_FIELDS
_FLAG_BAD_INDEX, _FLAG_NO_END = 2, 4
_INT32_MAX = 2 ** 31 - 1


def ellipse_half_widths(ksize):
    """-> list of `ksize` ints: the half-width dx of every row of cv.getStructuringElement(cv.MORPH_ELLIPSE, (ksize, ksize)).
    With r = c = ksize // 2, row i covers the columns [max(c - dx, 0), min(c + dx + 1, ksize)) where
    dx = round_half_even(c sqrt((r r - (i - r)^2) / (r r))), and dx = 0 for r = 0.  OpenCV is not available to the tests: this
    restates its formula and is unpinned against cv2."""
    ksize = int(ksize)
    if ksize < 1:
        raise ValueError("ksize must be >= 1")
    r = c = ksize // 2
    if r == 0:
        return [0] * ksize
    out = []
    for i in range(ksize):
        dy = i - r
        out.append(int(round(c * math.sqrt((r * r - dy * dy) / (r * r)))) if abs(dy) <= r else 0)     # round(): half to even
    return out


class PackedMasks:
    """words [n, H, ceil(W / 32)] int32: pixel (y, x) at bit x & 31 of word x >> 5, padding bits zero; H, W"""

    def __init__(self, words, H, W):
        self.words, self.H, self.W = words, int(H), int(W)

    def unpack(self):
        """-> [n, H, W] bool"""
        shifts = torch.arange(32, dtype=torch.int32, device=self.words.device)
        bits = (self.words.unsqueeze(-1) >> shifts) & 1
        return bits.reshape(self.words.shape[0], self.H, -1)[:, :, :self.W].to(torch.bool)


def _half_width_array(half_widths):
    hw = [int(h) for h in half_widths]
    if len(hw) < 1 or len(hw) % 2 == 0:
        raise ValueError("half_widths must have an odd number of rows, got %d" % len(hw))
    if min(hw) < 0 or max(hw) > 254:
        raise ValueError("every half-width must lie in [0, 254]")
    return (L.c_i * len(hw))(*hw), len(hw)


def dilate_plan(n, H, W, half_widths):
    """the launch plan of the dilation (csrc/mesh_clean_plan.h) as a dict"""
    arr, count = _half_width_array(half_widths)
    out = (L.c_l * _PLAN_FIELDS)()
    L.call("psdf_mesh_clean_dilate_plan", L.c_l(n), L.c_l(H), L.c_l(W), arr, L.c_l(count), out)
    names = ("radius", "tile_rows", "staged_rows", "tiles_x", "tiles_y", "words_per_row", "workgroups", "row_groups", "lds_bytes")
    return dict(zip(names, (int(v) for v in out)))


@torch.no_grad()
def row_distance(masks, threshold=128):
    """-> hd [n, H, W] uint8: the distance along the row to the nearest set pixel, saturated at 255 (the first of the two
    dilation kernels, exposed for the tests and the stage timings)"""
    L.require_cuda(masks)
    if masks.ndim != 3:
        raise ValueError("masks must be [n, H, W], got %s" % (tuple(masks.shape),))
    if masks.dtype == torch.bool:
        src, threshold = masks.contiguous().view(torch.uint8), 0
    elif masks.dtype == torch.uint8:
        src, threshold = masks.contiguous(), int(threshold)
    else:
        raise ValueError("masks must be uint8 or bool, got %s" % masks.dtype)
    if not 0 <= threshold <= 255:
        raise ValueError("threshold must lie in [0, 255]")
    n, H, W = src.shape
    if H < 1 or W < 1:
        raise ValueError("masks of %d x %d pixels" % (H, W))
    hd = torch.empty((n, H, W), dtype=torch.uint8, device=src.device)
    L.call("psdf_mesh_clean_row_distance", L.ptr(src), L.c_l(n), L.c_i(H), L.c_i(W), L.c_i(threshold), L.ptr(hd), L.stream())
    return hd


@torch.no_grad()
def dilate_masks(masks, half_widths, threshold=128):
    """-> PackedMasks: `masks` [n, H, W] uint8 (a pixel is set when its value is > threshold) or bool, dilated by the symmetric
    row-span element `half_widths` (odd length, every entry <= 254) anchored at its centre; outside the image nothing is set
    (cv.dilate's default border).  No host read."""
    arr, count = _half_width_array(half_widths)
    hd = row_distance(masks, threshold)
    n, H, W = hd.shape
    words = torch.empty((n, H, (W + 31) // 32), dtype=torch.int32, device=hd.device)
    L.call("psdf_mesh_clean_dilate", L.ptr(hd), L.c_l(n), L.c_i(H), L.c_i(W), arr, L.c_i(count), L.ptr(words), L.stream())
    return PackedMasks(words, H, W)


def _vertices(V):
    L.require_cuda(V)
    if V.ndim != 2 or V.shape[1] != 3:
        raise ValueError("V must be [N, 3], got %s" % (tuple(V.shape),))
    if V.shape[0] > _INT32_MAX:
        raise L.PsdfError("V: more than 2^31 - 1 vertices")
    return V.detach().to(torch.float32).contiguous()


def _faces(F):
    L.require_cuda(F)
    if F.ndim != 2 or F.shape[1] != 3:
        raise ValueError("F must be [F, 3], got %s" % (tuple(F.shape),))
    if F.shape[0] > _INT32_MAX // 3:
        raise L.PsdfError("F: more than (2^31 - 1) / 3 faces")
    return F.detach().to(torch.int32).contiguous()


@torch.no_grad()
def inside_masks(V, world_mats, packed):
    """-> [nV] bool: clean_points_by_mask.  `world_mats` [n, 4, 4] or [n, 3, 4] float64: the world_mat_i of cameras_sphere.npz;
    `packed`: the dilated masks of the same n views.  Per view, in float64: p = ((P00 x + P01 y) + P02 z) + P03 row by row,
    u = p0 / p2, v = p1 / p2, each rounded half to even; with 0 <= u < W and 0 <= v < H the view keeps the vertex iff the dilated
    bit (v, u) is set, otherwise it keeps it (the reference's `+ 1` into a ones-padded image); a non-finite u or v counts as
    outside the image; the sign of p2 is not tested.  The result is the AND over the views.  No host read."""
    V = _vertices(V)
    dev = V.device
    P = torch.as_tensor(world_mats).to(device=dev, dtype=torch.float64)
    if P.ndim != 3 or P.shape[1] not in (3, 4) or P.shape[2] != 4:
        raise ValueError("world_mats must be [n, 4, 4] or [n, 3, 4], got %s" % (tuple(P.shape),))
    words = packed.words
    L.require_cuda(words)
    if words.device != dev or words.dtype != torch.int32 or tuple(words.shape) != (P.shape[0], packed.H, (packed.W + 31) // 32):
        raise ValueError("packed masks do not match the %d views" % P.shape[0])
    P = P[:, :3, :].contiguous()
    nV = V.shape[0]
    keep = torch.empty(nV, dtype=torch.uint8, device=dev)
    L.call("psdf_mesh_clean_inside_masks", L.ptr(V), L.c_l(nV), L.ptr(P), L.c_i(P.shape[0]), L.ptr(words.contiguous()),
           L.c_i(packed.H), L.c_i(packed.W), L.ptr(keep), L.stream())
    return keep.to(torch.bool)


@torch.no_grad()
def inside_box(V, lo, hi):
    """-> [nV] bool: lo < p < hi in every coordinate (aabb.py:28-42: strict on both sides), compared in fp32 as the reference does"""
    lo = torch.as_tensor(lo, dtype=torch.float32).to(V.device).view(3)
    hi = torch.as_tensor(hi, dtype=torch.float32).to(V.device).view(3)
    p = V.detach().to(torch.float32)
    return ((p < hi) & (p > lo)).all(1)


def _mesh_of(mesh_or_VF):
    if hasattr(mesh_or_VF, "V") and hasattr(mesh_or_VF, "F"):
        return mesh_or_VF
    V, F = mesh_or_VF
    return ExtractedMesh(V, F)


def _raise_on(flag_bits, who, nV):
    if flag_bits & _FLAG_BAD_INDEX:
        raise ValueError("%s: a face names a vertex outside [0, %d)" % (who, nV))
    if flag_bits & _FLAG_NO_END:
        raise L.PsdfError("%s: a union-find loop exceeded its iteration cap" % who)


def _filter(mesh, keep, face_mask, who):
    V, F = _vertices(mesh.V), _faces(mesh.F)
    nV, nF, dev = V.shape[0], F.shape[0], V.device
    keep = torch.as_tensor(keep).to(device=dev)
    if keep.shape != (nV,):
        raise ValueError("keep must be [%d], got %s" % (nV, tuple(keep.shape)))
    keep = (keep != 0).to(torch.uint8).contiguous()
    NV = mesh.NV.detach().to(torch.float32).contiguous() if mesh.NV is not None and len(mesh.NV) == nV else None
    edges = getattr(mesh, "edges", None)
    edges = edges.detach().to(torch.int64).contiguous() if edges is not None and len(edges) == nV else None
    if face_mask is not None:
        face_mask = (face_mask != 0).to(torch.uint8).contiguous()
    face_keep = torch.zeros(nF, dtype=torch.uint8, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    L.call("psdf_mesh_clean_face_keep", L.ptr(F), L.c_l(nF), L.ptr(keep), L.c_l(nV), L.ptr(face_mask), L.ptr(face_keep),
           L.ptr(flag), L.stream())
    vincl = torch.cumsum(keep, 0, dtype=torch.int32)
    fincl = torch.cumsum(face_keep, 0, dtype=torch.int32)
    zero = torch.zeros(1, dtype=torch.int32, device=dev)
    kept_v, kept_f, bad = torch.cat([vincl[-1:] if nV else zero, fincl[-1:] if nF else zero, flag]).tolist()     # the host read
    _raise_on(bad, who, nV)
    V_out = torch.empty((kept_v, 3), dtype=torch.float32, device=dev)
    NV_out = torch.empty((kept_v, 3), dtype=torch.float32, device=dev) if NV is not None else None
    edges_out = torch.empty((kept_v, 2), dtype=torch.int64, device=dev) if edges is not None else None
    F_out = torch.empty((kept_f, 3), dtype=torch.int32, device=dev)
    vertex_map = torch.full((nV,), -1, dtype=torch.int32, device=dev)
    if kept_v:      # (an empty output has no address to hand over)
        L.call("psdf_mesh_clean_emit_vertices", L.c_l(nV), L.ptr(keep), L.ptr(vincl), L.ptr(V), L.ptr(NV), L.ptr(edges),
               L.ptr(V_out), L.ptr(NV_out), L.ptr(edges_out), L.ptr(vertex_map), L.stream())
    if kept_f:
        L.call("psdf_mesh_clean_emit_faces", L.ptr(F), L.c_l(nF), L.ptr(face_keep), L.ptr(fincl), L.ptr(vertex_map), L.ptr(F_out),
               L.stream())
    out = ExtractedMesh(V_out, F_out, NV_out, edges_out, getattr(mesh, "volume", None), getattr(mesh, "nr_evaluated", 0))
    C = getattr(mesh, "C", None)
    if C is not None and len(C) == nV:      # per-vertex colours (mesh_color.py): the kept vertices', in their order
        # a stable sort of the flags lists the kept vertices first, in their order; their number is known: no second host read
        kept = torch.argsort(keep, descending=True, stable=True)[:kept_v]
        out.C = C.to(dev).index_select(0, kept)
    out.vertex_map, out.face_keep = vertex_map, face_keep.to(torch.bool)
    return out


@torch.no_grad()
def filter_vertices(mesh_or_VF, keep):
    """-> ExtractedMesh with `.vertex_map` [nV] int32 (-1 where removed) and `.face_keep` [nF] bool:
    evaluate_chamfer_distance.py:146-155 and remove_marked_vertices(mask, True).  Kept vertices stay in their old order, a face
    survives iff all three of its vertices do, surviving faces stay in their old order and are renumbered; `NV`, `edges` and
    the per-vertex colours `C` are carried along.  A face naming a vertex outside [0, nV) raises ValueError.  One host read."""
    return _filter(_mesh_of(mesh_or_VF), keep, None, "filter_vertices")


@torch.no_grad()
def face_components(F, nV, connectivity="edge", return_flag=False):
    """-> (labels [nF] int32, sizes [nF] int32): labels[f] is the smallest face index of f's component, sizes[l] the number of
    faces of the component with label l (0 where l is not a label).  "edge": two faces are adjacent iff they share an undirected
    edge that occurs in exactly two half-edges of the whole mesh (trimesh's face_adjacency, restated and unpinned); an edge used
    by one face or by three or more, or whose endpoints are equal, links nothing.  "vertex": faces are adjacent iff they share a
    vertex.  One host read (the error flag; with return_flag it is returned as a third value: 0 when every loop ended within
    its cap and every face was in range)."""
    if connectivity not in ("edge", "vertex"):
        raise ValueError("connectivity must be 'edge' or 'vertex'")
    F = _faces(F)
    nV, nF, dev = int(nV), F.shape[0], F.device
    if nV < 0 or nV > _INT32_MAX:
        raise ValueError("nV must lie in [0, 2^31 - 1]")
    labels = torch.empty(nF, dtype=torch.int32, device=dev)
    sizes = torch.zeros(nF, dtype=torch.int32, device=dev)
    if nF == 0:
        return (labels, sizes, 0) if return_flag else (labels, sizes)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    if connectivity == "edge":
        keys = torch.empty(3 * nF, dtype=torch.int64, device=dev)
        L.call("psdf_mesh_clean_edge_keys", L.ptr(F), L.c_l(nF), L.c_l(nV), L.ptr(keys), L.ptr(flag), L.stream())
        keys, slot = torch.sort(keys, stable=True)
        parent = torch.arange(nF, dtype=torch.int32, device=dev)
        L.call("psdf_mesh_clean_link_edges", L.ptr(keys), L.ptr(slot.contiguous()), L.c_l(nF), L.ptr(parent), L.ptr(flag), L.stream())
        L.call("psdf_mesh_clean_flatten", L.ptr(parent), L.c_l(nF), L.ptr(labels), L.ptr(sizes), L.ptr(flag), L.stream())
    else:
        parent = torch.arange(nV, dtype=torch.int32, device=dev)
        L.call("psdf_mesh_clean_link_vertices", L.ptr(F), L.c_l(nF), L.c_l(nV), L.ptr(parent), L.ptr(flag), L.stream())
        vertex_label = torch.empty(nV, dtype=torch.int32, device=dev)
        L.call("psdf_mesh_clean_flatten", L.ptr(parent), L.c_l(nV), L.ptr(vertex_label), None, L.ptr(flag), L.stream())
        first_face = torch.full((nV,), _INT32_MAX, dtype=torch.int32, device=dev)
        L.call("psdf_mesh_clean_face_labels", L.ptr(F), L.c_l(nF), L.c_l(nV), L.ptr(vertex_label), L.ptr(first_face), L.ptr(labels),
               L.ptr(sizes), L.stream())
    bits = int(flag)                                                                                  # the host read
    _raise_on(bits, "face_components", nV)
    return (labels, sizes, bits) if return_flag else (labels, sizes)


def _largest(mesh, connectivity):
    F = _faces(mesh.F)
    nF, dev = F.shape[0], F.device
    labels, sizes = face_components(F, mesh.V.shape[0], connectivity)
    if nF == 0:
        return None, labels, sizes
    at = torch.arange(nF, dtype=torch.int64, device=dev)
    best = torch.where(sizes == sizes.max(), at, nF).min()       # a tie goes to the smallest label
    return labels == best, labels, sizes


def _keep_component(mesh, face_mask, who):
    nV, dev = mesh.V.shape[0], mesh.V.device
    keep = torch.zeros(nV, dtype=torch.uint8, device=dev)
    if face_mask is not None:
        keep[mesh.F[face_mask].reshape(-1).to(torch.int64)] = 1      # the vertices the component references
    return _filter(mesh, keep, face_mask, who)


@torch.no_grad()
def largest_component(mesh_or_VF, connectivity="edge"):
    """-> ExtractedMesh: the component with the most faces (a tie goes to the smallest label) of
    Trimesh.split(only_watertight=False), evaluate_chamfer_distance.py:160-161; unreferenced vertices are removed, the order of
    vertices and faces is preserved.  An empty face list returns an empty mesh.  Two host reads."""
    mesh = _mesh_of(mesh_or_VF)
    face_mask, _, _ = _largest(mesh, connectivity)
    return _keep_component(mesh, face_mask, "largest_component")


@torch.no_grad()
def clean_mesh_dtu(mesh, world_mats, masks, ksize=101, threshold=128, box=None, connectivity="edge"):
    """-> ExtractedMesh: the box cull if `box` = (lo, hi) is given (create_my_meshes.py:72-75), then the mask cull of
    clean_points_by_mask with the `ksize` ellipse, the face filter and the largest component (clean_mesh).  `.stats`:
    removed_by_box, removed_by_masks (vertices), components, faces (of the largest component).  `masks` [n, H, W] uint8 or bool,
    or PackedMasks already dilated."""
    mesh = _mesh_of(mesh)
    nV0 = mesh.V.shape[0]
    if box is not None:
        mesh = _filter(mesh, inside_box(mesh.V, box[0], box[1]), None, "clean_mesh_dtu")
    nV1 = mesh.V.shape[0]
    packed = masks if isinstance(masks, PackedMasks) else dilate_masks(masks, ellipse_half_widths(ksize), threshold)
    mesh = _filter(mesh, inside_masks(mesh.V, world_mats, packed), None, "clean_mesh_dtu")
    nV2 = mesh.V.shape[0]
    face_mask, _, sizes = _largest(mesh, connectivity)
    out = _keep_component(mesh, face_mask, "clean_mesh_dtu")
    components = int((sizes > 0).sum()) if sizes.numel() else 0                                       # the host read
    out.stats = {"removed_by_box": nV0 - nV1, "removed_by_masks": nV1 - nV2, "components": components, "faces": out.F.shape[0]}
    return out
