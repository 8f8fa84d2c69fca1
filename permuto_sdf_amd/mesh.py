"""Mesh extraction on the device: marching tetrahedra (csrc/mesh.hip) over a resident volume, or streamed over an SDF network.

`marching_tetrahedra(volume)` is `skimage.measure.marching_cubes` / compat/skimage/measure.py for a CUDA tensor: same
triangulation, same inside test, vertices welded on grid edges and numbered in the stand-in's order -- only the order of the
faces (cell by cell here) and their winding (combinatorial here: csrc/mesh_tables.h) differ.

`MeshExtractor(encoding, mlp, window).extract(n, min, max)` is the reference's `extract_mesh_from_sdf_model`
(permuto_sdf_py/utils/sdf_utils.py:252-292) without the n^3 volume: the field is evaluated slab by slab of x-planes through
the level-major encode + MLP pair (1-row head, as the sphere tracer does), a slab keeps two planes of overlap, and the vertices
of a slab are welded to those of its neighbours because their numbers come from one running prefix sum.  The result does not
depend on the slab size, bit for bit.  With `occupancy_grid=` only the grid points next to an occupied voxel are evaluated.
"""
import os
import warnings

import torch

from . import _lib as L
from .net_eval import masked_sdf, masked_sdf_gradient, one_row_head

_MSG_SHAPE = "Input volume should be a 3D numpy array with at least 2 samples per axis."
_MSG_LEVEL = "Surface level must be within volume data range."


def _march(vol, valid, level, shape, xbase, nplanes, p0, p1, c0, c1, mask, vincl, v_off, want_edges, normals_of_volume):
    """classify -> scans -> emit for vertex planes [p0, p1) and cell planes [c0, c1) of the buffers (csrc/mesh.hip).
    -> verts [v, 3], edges [v, 2] | None, normals [v, 3] | None, faces [f, 3] (global vertex ids).  One host read (the two totals)."""
    X, Y, Z = shape
    plane, dev = Y * Z, vol.device
    dims = (L.c_i(X), L.c_i(Y), L.c_i(Z), L.c_i(xbase), L.c_i(nplanes))
    c1 = max(c0, c1)
    vcount = torch.empty((p1 - p0) * plane, dtype=torch.int32, device=dev)
    tcount = torch.empty((c1 - c0) * plane, dtype=torch.int32, device=dev)
    L.call("psdf_mesh_classify", L.ptr(vol), L.ptr(valid), L.c_f(level), *dims, L.c_i(p0), L.c_i(p1), L.c_i(c0), L.c_i(c1),
           L.ptr(mask), L.ptr(vcount), L.ptr(tcount), L.stream())
    vin = vincl[(p0 - xbase) * plane:(p1 - xbase) * plane]
    torch.cumsum(vcount, 0, dtype=torch.int32, out=vin)
    if v_off:
        vin += v_off
    tincl = torch.cumsum(tcount, 0, dtype=torch.int32)
    zero = torch.zeros(1, dtype=torch.int32, device=dev)
    nv, nf = torch.cat([vin[-1:] if vin.numel() else zero + v_off, tincl[-1:] if tincl.numel() else zero]).tolist()
    nv -= v_off
    verts = torch.empty((nv, 3), dtype=torch.float32, device=dev)
    edges = torch.empty((nv, 2), dtype=torch.int64, device=dev) if want_edges else None
    normals = torch.empty((nv, 3), dtype=torch.float32, device=dev) if normals_of_volume else None
    faces = torch.empty((nf, 3), dtype=torch.int32, device=dev)
    if nv:
        L.call("psdf_mesh_emit_vertices", L.ptr(vol), L.c_f(level), *dims, L.c_i(p0), L.c_i(p1), L.ptr(mask), L.ptr(vincl),
               L.c_l(v_off), L.ptr(verts), L.ptr(edges), L.ptr(normals), L.stream())
    if nf:
        L.call("psdf_mesh_emit_faces", L.ptr(vol), L.ptr(valid), L.c_f(level), *dims, L.c_i(c0), L.c_i(c1), L.ptr(mask),
               L.ptr(vincl), L.ptr(tincl), L.ptr(faces), L.stream())
    return verts, edges, normals, faces


def marching_tetrahedra(volume, level=0.0, spacing=(1.0, 1.0, 1.0), normals=True, return_edges=False, _check_range=True):
    """-> (verts [V,3] f32 in index coordinates * spacing, faces [F,3] i32, normals [V,3] f32 | None, values [V] f32[, edges [V,2]
    i64: linear indices of the two grid points of every vertex's edge]) as device tensors; the convention of
    skimage.measure.marching_cubes: normals point towards decreasing values.  ValueError under the stand-in's two conditions."""
    L.require_cuda(volume)
    if volume.ndim != 3 or min(volume.shape) < 2:
        raise ValueError(_MSG_SHAPE)
    vol = volume.detach().to(torch.float32).contiguous()
    level = float(level)
    if _check_range:
        lo, hi = torch.stack([vol.min(), vol.max()]).tolist()      # NaN propagates, as in numpy: a volume with a NaN raises
        if not (lo < level < hi):
            raise ValueError(_MSG_LEVEL)
    X, Y, Z = vol.shape
    if vol.numel() >= 2 ** 31 // 7:
        raise ValueError("marching_tetrahedra: %d grid points exceed the int32 vertex ids of one pass; stream the field with "
                         "MeshExtractor" % vol.numel())
    mask = torch.empty(vol.numel(), dtype=torch.uint8, device=vol.device)
    vincl = torch.empty(vol.numel(), dtype=torch.int32, device=vol.device)
    verts, edges, nrm, faces = _march(vol.view(-1), None, level, (X, Y, Z), 0, X, 0, X, 0, X - 1, mask, vincl, 0, return_edges,
                                      normals)
    sp = tuple(float(s) for s in spacing)
    if sp != (1.0, 1.0, 1.0):
        verts = verts * torch.tensor(sp, dtype=torch.float32, device=vol.device)
    values = torch.full((verts.shape[0],), level, dtype=torch.float32, device=vol.device)
    out = (verts, faces, nrm, values)
    return out + (edges,) if return_edges else out


class ExtractedMesh:
    """V [V,3] f32 world positions, F [F,3] i32, NV [V,3] f32 outward unit normals or None (what the reference stores as
    `NV = -normals`, sdf_utils.py:288); `edges` [V,2] i64 and `volume` [n,n,n] when requested; `nr_evaluated` grid points;
    C [V,3] u8 per-vertex colours or None (mesh_color.MeshColorizer.colorize)."""

    def __init__(self, V, F, NV=None, edges=None, volume=None, nr_evaluated=0, C=None):
        self.V, self.F, self.NV, self.edges, self.volume, self.nr_evaluated, self.C = V, F, NV, edges, volume, nr_evaluated, C

    def cpu(self):
        c = lambda t: None if t is None else t.cpu()    # noqa: E731
        return ExtractedMesh(c(self.V), c(self.F), c(self.NV), c(self.edges), c(self.volume), self.nr_evaluated, c(self.C))

    def save_ply(self, path):
        """binary little-endian PLY in the layout of compat/easypbr Mesh.save_to_file: 12 (24 with normals) bytes per vertex,
        13 per face; with colours `C`, `uchar red, green, blue` after them: 15 (27) bytes per vertex"""
        import numpy as np
        V = self.V.detach().cpu().numpy().astype("<f4").reshape(-1, 3)
        F = self.F.detach().cpu().numpy().astype("<i4").reshape(-1, 3)
        has_n = self.NV is not None and len(self.NV) == len(V) and len(V) > 0
        has_c = self.C is not None and len(self.C) == len(V) and len(V) > 0
        props = "property float x\nproperty float y\nproperty float z\n" + (
            "property float nx\nproperty float ny\nproperty float nz\n" if has_n else "") + (
            "property uchar red\nproperty uchar green\nproperty uchar blue\n" if has_c else "")
        header = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\n%selement face %d\nproperty list uchar int "
                  "vertex_indices\nend_header\n" % (len(V), props, len(F)))
        vert = np.concatenate([V, self.NV.detach().cpu().numpy().astype("<f4").reshape(-1, 3)], 1) if has_n else V
        if has_c:       # a packed record per vertex: the floats, then three bytes
            rec = np.empty(len(V), dtype=[("f", "<f4", (vert.shape[1],)), ("c", "u1", (3,))])
            rec["f"], rec["c"] = vert, self.C.detach().cpu().numpy().astype("u1").reshape(-1, 3)
            vert = rec
        face = np.empty(len(F), dtype=[("n", "u1"), ("i", "<i4", (3,))])
        face["n"], face["i"] = 3, F
        os.makedirs(os.path.dirname(os.path.abspath(path)) or ".", exist_ok=True)
        with open(path, "wb") as f:
            f.write(header.encode("ascii"))
            f.write(np.ascontiguousarray(vert).tobytes())
            f.write(face.tobytes())


class MeshExtractor:
    """Streams marching tetrahedra over an SDF.  `MeshExtractor(encoding, mlp, window)`: the SDF is row 0 of the MLP's head
    (evaluated with a 1-row head); `MeshExtractor(fn)`: any callable points [N,3] -> [N,1] (no analytic normals)."""

    DEFAULT_POINT_BUDGET = 1 << 21      # points per encode + MLP launch pair: channels * 4 bytes of features each
    DEFAULT_SLAB_POINTS = 1 << 24       # grid points per slab when slab_planes is not given (22 bytes of tables each)

    def __init__(self, encoding, mlp=None, window=None, device=None):
        self.device = torch.device(device) if device is not None else None      # of a callable's points (default: current GPU)
        if mlp is None:
            if not callable(encoding):
                raise TypeError("MeshExtractor needs (encoding, mlp) or a callable points [N,3] -> [N,1]")
            self.fn, self.enc, self.mlp, self.window = encoding, None, None, None
            return
        self.fn, self.enc, self.mlp = None, encoding, mlp
        dev = encoding.lattice_values.device
        self.window = (window if window is not None else torch.ones(encoding.nr_levels, device=dev)).contiguous()

    @classmethod
    def from_sdf_net(cls, net, iter_nr):
        """from a train_step.SdfNet at training iteration `iter_nr` (its coarse-to-fine window)"""
        return cls(net.encoding, net.mlp_sdf, net.window(iter_nr))

    # ---- the network: forward of a chunk, gradient at arbitrary points --------------------------------------------------
    def _forward(self, pts, skip, feat_flat, out):
        """out [1, N] <- SDF at pts [N,3]; points with skip != 0 keep what `out` holds"""
        C, N = self.enc.cfg.channels, pts.shape[0]
        feat, _ = masked_sdf(self.enc, self.window, self._net.dims, self._net.packed, pts, skip=skip, out=out,
                             feat_buf=feat_flat[:C * N].view(C, N))
        return feat

    @torch.no_grad()
    def sdf_gradient(self, pts, point_budget=None):
        """analytic d sdf / d x at pts [N,3] -> [N,3]: the sphere tracer's launches (masked MLP data gradient of a unit output
        gradient, then the encoding's position gradient), in chunks of `point_budget` points"""
        if self.enc is None:
            raise L.PsdfError("MeshExtractor over a callable has no analytic gradient")
        if not hasattr(self, "_net"):
            self._net = one_row_head(self.mlp, pack=True)
        B = int(point_budget or self.DEFAULT_POINT_BUDGET)
        cfg, dev = self.enc.cfg, pts.device
        grads = torch.zeros((pts.shape[0], 3), dtype=torch.float32, device=dev)
        nb = min(B, max(1, pts.shape[0]))
        feat_flat = torch.empty(cfg.channels * nb, dtype=torch.float32, device=dev)
        d_flat = torch.empty(cfg.channels * nb, dtype=torch.float32, device=dev)
        live = torch.zeros(nb, dtype=torch.bool, device=dev)
        for a in range(0, pts.shape[0], B):
            p = pts[a:a + B].contiguous()
            N = p.shape[0]
            sdf = torch.zeros((1, N), dtype=torch.float32, device=dev)
            feat = self._forward(p, None, feat_flat, sdf)
            masked_sdf_gradient(self.enc, self.window, self._net, p, feat, live[:N], out=grads[a:a + N],
                                d_feat=d_flat[:cfg.channels * N].view(cfg.channels, N))
        return grads

    # ---- extraction ---------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def extract(self, nr_points_per_dim, min_val, max_val, threshold=0.0, slab_planes=None, point_budget=None,
                occupancy_grid=None, normals=True, return_edges=False, return_volume=False):
        n = int(nr_points_per_dim)
        if n < 2:
            raise ValueError(_MSG_SHAPE)
        dev = self.enc.lattice_values.device if self.enc is not None else (
            self.device or (occupancy_grid._dev if occupancy_grid is not None else torch.device("cuda", torch.cuda.current_device())))
        if self.enc is not None:
            self._net = one_row_head(self.mlp, pack=True)      # (every extraction: the net may have been trained on since)
        plane = n * n
        S = int(slab_planes) if slab_planes else max(1, self.DEFAULT_SLAB_POINTS // plane)
        S = max(1, min(S, n))
        B = int(point_budget or self.DEFAULT_POINT_BUDGET)
        level = float(threshold)
        axis = torch.linspace(min_val, max_val, n, device=dev)          # the reference's coordinates, torch's bits
        h = (float(max_val) - float(min_val)) / (n - 1)
        grid = occupancy_grid
        if grid is not None and h > grid.m_grid_extent / grid.m_nr_voxels_per_dim:
            warnings.warn("MeshExtractor: mesh spacing %.4g exceeds the occupancy voxel size %.4g, the sparse mode cannot "
                          "guarantee the dense mesh: extracting densely" % (h, grid.m_grid_extent / grid.m_nr_voxels_per_dim))
            grid = None
        cap = min(S + 2, n)                                                 # planes the slab buffers hold
        val = torch.empty(cap * plane, dtype=torch.float32, device=dev)
        valid = torch.empty(cap * plane, dtype=torch.uint8, device=dev) if grid is not None else None
        mask = torch.empty(cap * plane, dtype=torch.uint8, device=dev)
        vincl = torch.empty(cap * plane, dtype=torch.int32, device=dev)
        nb = min(B, cap * plane)
        pts_buf = torch.empty((nb, 3), dtype=torch.float32, device=dev)
        out_buf = torch.empty(nb, dtype=torch.float32, device=dev)
        skip_buf = torch.empty(nb, dtype=torch.uint8, device=dev) if grid is not None else None
        # (zeros: the columns of skipped points are never written, and the MLP's tiles read them beside the live ones)
        feat_flat = torch.zeros(self.enc.cfg.channels * nb, dtype=torch.float32, device=dev) if self.enc is not None else None
        volume = torch.full((n * plane,), float("nan"), dtype=torch.float32, device=dev) if return_volume else None
        inf = float("inf")
        lo_hi = torch.tensor([inf, -inf], dtype=torch.float32, device=dev)
        nr_eval = torch.zeros((), dtype=torch.int64, device=dev)
        if grid is not None:
            occ, tr = grid._occ(), (L.c_f * 3)(*grid.m_grid_translation)

        def evaluate(xbase, a, b):
            """value planes [a, b) -> their slots of `val` (and `valid`), at most B points per launch pair"""
            nonlocal lo_hi, nr_eval
            first, end = (a - xbase) * plane, (b - xbase) * plane
            for s in range(first, end, B):
                N = min(B, end - s)
                pts, out = pts_buf[:N], out_buf[:N]
                L.call("psdf_mesh_grid_points", L.c_i(n), L.c_i(n), L.c_i(n), L.c_i(xbase), L.c_l(s), L.c_l(N), L.ptr(axis),
                       L.ptr(axis), L.ptr(axis), L.ptr(pts), L.stream())
                skip = None
                if grid is not None:
                    skip, ok = skip_buf[:N], valid[s:s + N]
                    L.call("psdf_mesh_sparse_mask", L.c_l(N), L.c_i(grid.m_nr_voxels_per_dim), L.c_f(grid.m_grid_extent), tr,
                           L.ptr(occ), L.ptr(pts), L.c_f(h), L.ptr(ok), L.ptr(skip), L.stream())
                    out.fill_(float("nan"))        # never read by the marching passes (`valid` gates them); NaN if it ever were
                if self.fn is None:
                    self._forward(pts, skip, feat_flat, out.view(1, N))
                elif skip is None:
                    out.copy_(self.fn(pts).reshape(-1))
                else:
                    sel = ok.nonzero().view(-1)
                    if sel.numel():
                        out[sel] = self.fn(pts[sel]).reshape(-1).to(torch.float32)
                val[s:s + N] = out
                if skip is None:
                    lo_hi = torch.stack([torch.minimum(lo_hi[0], out.min()), torch.maximum(lo_hi[1], out.max())])
                    nr_eval += N
                else:
                    okb = ok.bool()
                    lo_hi = torch.stack([torch.minimum(lo_hi[0], torch.where(okb, out, inf).min()),
                                         torch.maximum(lo_hi[1], torch.where(okb, out, -inf).max())])
                    nr_eval += okb.sum()
                if volume is not None:
                    g0 = xbase * plane + s
                    volume[g0:g0 + N] = out
        Vs, Es, Fs = [], [], []
        p0 = have = v_off = 0
        while p0 < n:
            p1 = min(p0 + S, n)
            xbase = max(p0 - 1, 0)
            need = min(p1, n - 1) + 1               # value planes [xbase, need) must be in the buffer
            evaluate(xbase, have, need)
            have = need
            verts, edges, _, faces = _march(val, valid, level, (n, n, n), xbase, min(cap, n - xbase), p0, p1, xbase, p1 - 1, mask,
                                            vincl, v_off, return_edges, False)
            Vs.append(verts)
            Es.append(edges)
            Fs.append(faces)
            v_off += verts.shape[0]
            if p1 < n:                                # carry planes p1 - 1 and p1 to the front: the next slab's xbase is p1 - 1
                k = (p1 - 1 - xbase) * plane
                for buf, planes in ((val, 2), (valid, 2), (mask, 1), (vincl, 1)):
                    if buf is not None:
                        buf[:planes * plane] = buf[k:k + planes * plane].clone()
            p0 = p1
        lo, hi = lo_hi.tolist()
        if not (lo < level < hi):
            raise ValueError(_MSG_LEVEL)
        V = torch.cat(Vs)
        V = V / (n - 1) * (float(max_val) - float(min_val)) + float(min_val)     # sdf_utils.py:283
        NV = None
        if normals and self.enc is not None:
            NV = torch.nn.functional.normalize(self.sdf_gradient(V, B), dim=1)
        return ExtractedMesh(V, torch.cat(Fs), NV, torch.cat(Es) if return_edges else None,
                             volume.view(n, n, n) if volume is not None else None, int(nr_eval))
