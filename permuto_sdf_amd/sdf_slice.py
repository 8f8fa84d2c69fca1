"""Cross-sections of a fitted SDF on the device: isoline slices, alone or cut into a rendered view (csrc/sdf_slice.hip).

The reference judges a field -- eikonal quality, ghost sheets off the surface, how a 4-D fit moves through time -- with
create_sdf_isolines (permuto_sdf_py/experiments/visualization/visualize_sdf_isolines.py:62-166, again in
render_from_frame.py:71-166): a square layer of points in the camera's axes at a chosen depth, the SDF there in chunks of 6 000
points, a round trip through float64 on the host, a colour map, 15 masked passes for the iso-bands, and a viewer for the depth
test against the surface.  Here

  * `SlicePlane(axes, z, extent_scale)`     the layer: the COLUMNS of `axes` [3, 3] are its axes, `z` its depth along the third,
                                            x and y span [-extent_scale, extent_scale); `SlicePlane.from_frame(frame, z)` takes
                                            the camera's axes (the rotation of tf_world_cam as it is: cam.cam_axes());
  * `IsoStyle(width, distance, nr_lines, base_map, line_map, table)`   the colours: base = table(map_range(sdf, *base_map)), line
                                            i at sdf in (i distance -+ width / 2) takes table(map_range(i distance, *line_map));
                                            defaults of src/NGPGui.cxx:22-25; `PUBU` is the default table;
  * `render_slice(net, plane, box, size)`   -> `SliceImage(rgb [3, S, S], sdf [1, S, S], inside [1, S, S])`.  Per chunk: points
                                            -> `net_eval.masked_sdf` with the 1-row head under the outside-the-box mask ->
                                            colorize.  No host wait, no allocation after the first chunk's buffers;
  * `cut_slice_into(net, plane, box, frame, rgb, depth, weights_sum)`   the layer as `frame` sees it, cut IN PLACE into the
                                            planes of a view the caller has (a `TracedFrame`, a `BoxTracedFrame` with (n + 1) / 2
                                            as vis_4d_sdf.py maps it, a volumetric `RenderedFrame` with a depth of its own): the
                                            slice wins a pixel where there is no surface or the layer is nearer.  -> slice_mask.

Restated and unpinned (easypbr is absent): the summation order of the float64 rotation, the "pubu" table (ColorBrewer's 9-class
PuBu here) and its interpolation; csrc/sdf_slice.hip states all three.  CPU tensors raise PsdfError: there is no CPU path.
"""
import dataclasses
import functools

import numpy as np
import torch

from . import _lib as L
from .bridge import OccupancyGrid
from .frame import FramePlan, frame_device, frame_rays, new_planes, open_window
from .net_eval import masked_sdf, one_row_head

MAX_LINES = 32              # csrc/sdf_slice_plan.h
_MAX_CELLS = 2 ** 31 - 1
_POOL = OccupancyGrid.POOL  # the points the tracers evaluate at once

# ColorBrewer 9-class PuBu, light to dark
PUBU = tuple(tuple(c / 255.0 for c in rgb) for rgb in (
    (255, 247, 251), (236, 231, 242), (208, 209, 230), (166, 189, 219), (116, 169, 207), (54, 144, 192), (5, 112, 176), (4, 90, 141),
    (2, 56, 88)))


def _map_range64(x, in_lo, in_hi, out_lo, out_hi):
    """common_utils.py:162-166 in float64"""
    return out_lo + ((out_hi - out_lo) / (in_hi - in_lo)) * (min(max(x, in_lo), in_hi) - in_lo)


def table_lookup64(table, t):
    """the piecewise-linear map over the control points `table` [K, 3] at t clamped to [0, 1], in float64 -> [3]"""
    tab = np.asarray(table, np.float64)
    K = tab.shape[0]
    u = min(max(float(t), 0.0), 1.0) * (K - 1)
    j = min(int(u), K - 2)
    return tab[j] + (u - j) * (tab[j + 1] - tab[j])


@dataclasses.dataclass(frozen=True)
class IsoStyle:
    """visualize_sdf_isolines.py:111-138 as data.  base_map / line_map: (in_lo, in_hi, out_lo, out_hi) of the two map_range
    calls; table: K >= 2 control points (r, g, b) in [0, 1], held on the device as float32"""
    width: float = 0.005
    distance: float = 0.03
    nr_lines: int = 15
    base_map: tuple = (0.0, 0.3, 0.2, 1.0)
    line_map: tuple = (0.0, 0.2, 0.3, 1.0)
    table: tuple = PUBU

    def __post_init__(self):
        tab = np.asarray(self.table, np.float64)
        if tab.ndim != 2 or tab.shape[1] != 3 or tab.shape[0] < 2:
            raise ValueError("a colour table is K >= 2 control points (r, g, b), got an array of shape %s" % (tab.shape,))
        object.__setattr__(self, "table", tuple(tuple(float(v) for v in row) for row in tab))
        object.__setattr__(self, "base_map", tuple(float(v) for v in self.base_map))
        object.__setattr__(self, "line_map", tuple(float(v) for v in self.line_map))
        object.__setattr__(self, "nr_lines", int(self.nr_lines))
        if not 0 <= self.nr_lines <= MAX_LINES:
            raise ValueError("between 0 and %d iso-lines, got %d" % (MAX_LINES, self.nr_lines))
        for m in (self.base_map, self.line_map):
            if len(m) != 4 or not m[1] > m[0]:
                raise ValueError("a map_range is (in_lo, in_hi, out_lo, out_hi) with in_hi > in_lo, got %r" % (m,))

    def table32(self):
        """[K, 3] float32: the control points as the device holds them"""
        return np.asarray(self.table, np.float32)

    def band_table(self):
        """-> (lo [n], hi [n], rgb [n, 3]) float32: line i spans i distance -+ width / 2, computed in float64 and rounded; its
        colour is the float64 lookup of map_range(i distance, *line_map) in the float32 control points, rounded"""
        n = self.nr_lines
        centre = [i * self.distance for i in range(n)]
        lo = np.asarray([c - self.width / 2 for c in centre], np.float64).astype(np.float32)
        hi = np.asarray([c + self.width / 2 for c in centre], np.float64).astype(np.float32)
        tab = self.table32()
        rgb = np.asarray([table_lookup64(tab, _map_range64(c, *self.line_map)) for c in centre], np.float64).reshape(n, 3)
        return lo, hi, rgb.astype(np.float32)

    def base_map32(self):
        """(in_lo, in_hi, out_lo, scale) float32, the scale from float64"""
        a, b, c, d = self.base_map
        return np.asarray([a, b, c, (d - c) / (b - a)], np.float64).astype(np.float32)


@functools.lru_cache(maxsize=64)
def _colour_args(style, device):
    """the colour arguments of psdf_slice_colorize / psdf_slice_cut_resolve for `style`: the table goes to the device once"""
    tab = torch.from_numpy(style.table32()).to(device).contiguous()
    lo, hi, rgb = style.band_table()
    n = style.nr_lines
    host = ((L.c_f * 4)(*style.base_map32().tolist()), (L.c_f * max(1, n))(*lo.tolist()), (L.c_f * max(1, n))(*hi.tolist()),
            (L.c_f * max(1, 3 * n))(*rgb.reshape(-1).tolist()))
    return tab, (L.ptr(tab), L.c_i(tab.shape[0]), host[0], L.c_i(n), host[1], host[2], host[3])


class SlicePlane:
    """The layer of create_sdf_isolines: the points (x a0 + y a1) + z a2 with a0, a1, a2 the COLUMNS of `axes` [3, 3] and x, y
    in [-extent_scale, extent_scale).  Host values: a plane is a kernel argument."""

    def __init__(self, axes, z, extent_scale=1.0):
        a = axes.detach().cpu().numpy() if isinstance(axes, torch.Tensor) else np.asarray(axes)
        if a.shape != (3, 3):
            raise ValueError("SlicePlane takes axes [3, 3] (its columns are the axes), got %s" % (a.shape,))
        self.axes = np.ascontiguousarray(a, np.float32)
        self.z, self.extent_scale = float(z), float(extent_scale)
        if not self.extent_scale > 0:
            raise ValueError("extent_scale must be positive, got %r" % (extent_scale,))
        self._axes_c = (L.c_f * 9)(*self.axes.reshape(-1).tolist())

    @staticmethod
    def from_frame(frame, z, extent_scale=1.0):
        """the layer in the camera's axes (visualize_sdf_isolines.py:90: the columns of the rotation of tf_world_cam) at depth z"""
        return SlicePlane(frame.tf_world_cam[:3, :3], z, extent_scale)


@dataclasses.dataclass
class SliceImage:
    """float32 planes on the device; cell [row, col] is the layer's point (x, y) = (col, row)"""
    rgb: torch.Tensor       # [3, S, S] the colour map with its iso-bands, 0 outside the box and where the SDF is a NaN
    sdf: torch.Tensor       # [1, S, S] the SDF, 0 outside the box
    inside: torch.Tensor    # [1, S, S] 1 strictly inside the box, else 0 (the points the reference keeps)


@dataclasses.dataclass
class SlicedFrame:
    """a view with a slice cut into it: `base` is the view as rendered, whose depth and weights_sum planes are the ones below
    (cut in place)"""
    base: object
    rgb: torch.Tensor           # [3, H, W]
    depth: torch.Tensor         # [1, H, W]
    weights_sum: torch.Tensor   # [1, H, W]
    slice_mask: torch.Tensor    # [1, H, W] 1 where the slice is what the pixel shows


def _check_time(pos_dim, time_val):
    """BoxTracer._check_time's refusals"""
    if pos_dim not in (3, 4):
        raise ValueError("a slice is taken of a 3-D or a 4-D field, got pos_dim = %d" % pos_dim)
    if pos_dim == 4 and time_val is None:
        raise ValueError("a 4-D field is cut at a time: pass time_val")
    if pos_dim == 3 and time_val is not None:
        raise ValueError("a 3-D field has no time: time_val must be None")


class _Field:
    """what both functions need of a net: the window, the 1-row head, the time on the device and the chunk buffers"""

    def __init__(self, net, it, time_val, n):
        enc = self.enc = net.encoding
        self.P = P = int(enc.cfg.pos_dim)
        _check_time(P, time_val)
        L.require_cuda(enc.lattice_values)
        self.dev = dev = enc.lattice_values.device
        self.window = open_window(net, it).detach().to(device=dev, dtype=torch.float32).contiguous()
        self.head = one_row_head(net.mlp_sdf, pack=True)      # channel 0 of the last layer is the SDF (models.py:190-192)
        self.time = torch.full((1,), float(time_val), dtype=torch.float32, device=dev) if P == 4 else None
        self.C, self.n = int(enc.cfg.channels), n
        # flat, so that a shorter last chunk is a view of the same memory
        self.pts = torch.empty(n * P, dtype=torch.float32, device=dev)
        self.skip = torch.empty(n, dtype=torch.bool, device=dev)
        self.sdf = torch.zeros(n, dtype=torch.float32, device=dev)
        self.feat = torch.zeros(self.C * n, dtype=torch.float32, device=dev)

    def views(self, count):
        return self.pts[:count * self.P].view(count, self.P), self.skip[:count], self.sdf[:count].view(1, count)

    def evaluate(self, pts, skip, sdf):
        count = pts.shape[0]
        masked_sdf(self.enc, self.window, self.head.dims, self.head.packed, pts, skip=skip, out=sdf,
                   feat_buf=self.feat[:self.C * count].view(self.C, count))


def slice_points_raw(plane, box, size, first, count, pts, skip, time=None):
    """csrc/sdf_slice.hip: the cells [first, first + count) of the size x size layer -> pts [count, P], skip [count]"""
    L.require_cuda(pts, skip, time)
    L.call("psdf_slice_points", L.c_i(int(size)), L.c_l(int(first)), L.c_i(int(count)), L.c_i(pts.shape[1]), plane._axes_c,
           L.c_f(plane.z), L.c_f(plane.extent_scale), box._tr_c, box._half_c, L.ptr(time), L.ptr(pts), L.ptr(skip), L.stream())


def slice_colorize_raw(style, size, first, count, sdf, skip, out):
    """csrc/sdf_slice.hip: sdf, skip [count] of the cells [first, first + count) -> the planes of `out` (a SliceImage)"""
    L.require_cuda(sdf, skip, out.rgb, out.sdf, out.inside)
    _, colours = _colour_args(style, sdf.device)
    L.call("psdf_slice_colorize", L.c_i(int(size)), L.c_l(int(first)), L.c_i(int(count)), L.ptr(sdf), L.ptr(skip), *colours,
           L.ptr(out.rgb), L.ptr(out.sdf), L.ptr(out.inside), L.stream())


@torch.no_grad()
def render_slice(net, plane, box, size=500, style=IsoStyle(), it=None, time_val=None, max_points_per_chunk=_POOL):
    """-> SliceImage of the field of `net` (anything with `encoding`, `mlp_sdf` and `window(it)`) on `plane` inside `box` (a
    box_trace.Box), at `time_val` for a 4-D net.  size: cells per side (the reference: 500, 4000 for its full layer).  it: the
    iteration whose coarse-to-fine window is used (None: fully open, frame.IT_WINDOW_OPEN).  Chunks of at most
    max_points_per_chunk cells; per chunk four launches (points, masked encode, masked MLP, colorize) and no host wait; the
    buffers of the first chunk serve all of them."""
    S, chunk = int(size), int(max_points_per_chunk)
    if S < 1 or chunk < 1:
        raise ValueError("a layer has size >= 1 and chunks of >= 1 points, got %d and %d" % (S, chunk))
    cells = S * S
    if cells > _MAX_CELLS:
        raise L.PsdfError("a layer of %d x %d cells does not fit 31-bit cell indices" % (S, S))
    f = _Field(net, it, time_val, min(chunk, cells))
    out = SliceImage(*(torch.empty((c, S, S), dtype=torch.float32, device=f.dev) for c in (3, 1, 1)))    # every cell is written once
    for first in range(0, cells, f.n):
        count = min(f.n, cells - first)
        pts, skip, sdf = f.views(count)
        slice_points_raw(plane, box, S, first, count, pts, skip, f.time)
        f.evaluate(pts, skip, sdf)
        slice_colorize_raw(style, S, first, count, sdf, skip, out)
    return out


def _plane_of(frame, t, c, dev, name):
    H, W = frame.height, frame.width
    if not isinstance(t, torch.Tensor):
        raise ValueError("%s must be a tensor" % name)
    L.require_cuda(t)
    if t.device != dev:
        raise L.PsdfError("%s lives on %s, the net on %s" % (name, t.device, dev))
    if tuple(t.shape) != (c, H, W) or t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError("%s must be a contiguous float32 [%d, %d, %d] plane, got %s %s" % (name, c, H, W, t.dtype, tuple(t.shape)))
    return t


@torch.no_grad()
def cut_slice_into(net, plane, box, frame, rgb, depth, weights_sum, style=IsoStyle(), it=None, time_val=None,
                   max_rays_per_chunk=_POOL):
    """The layer as `frame` sees it, cut in place into rgb [3, H, W], depth [1, H, W] and weights_sum [1, H, W] of a view of the
    same frame: a pixel whose ray meets the layer inside the box, in front of the camera, with no surface (weights_sum == 0) or
    nearer than it (t < depth, the distance along the unit ray), takes the slice's colour, depth <- t and weights_sum <- 1; every
    other pixel keeps its bits.  -> slice_mask [1, H, W].  Per chunk of at most max_rays_per_chunk rays (frame.FramePlan with
    one sample per ray): rays -> begin -> `net_eval.masked_sdf` -> resolve.  No host wait."""
    _check_time(int(net.encoding.cfg.pos_dim), time_val)
    dev = frame_device(frame, net)
    H, W = frame.height, frame.width
    rgb, depth, weights_sum = (_plane_of(frame, t, c, dev, n) for t, c, n in ((rgb, 3, "rgb"), (depth, 1, "depth"),
                                                                              (weights_sum, 1, "weights_sum")))
    fplan = FramePlan(H, W, 1, max_rays_per_chunk)
    f = _Field(net, it, time_val, fplan.rays_per_chunk)
    t_buf = torch.empty(f.n, dtype=torch.float32, device=dev)
    mask = new_planes(frame, 1, dev)
    _, colours = _colour_args(style, dev)
    for first, count in fplan.chunks():
        o, d = frame_rays(frame, first, count)
        pts, skip, sdf = f.views(count)
        L.call("psdf_slice_cut_begin", L.c_i(count), L.c_i(f.P), plane._axes_c, L.c_f(plane.z), L.c_f(plane.extent_scale), box._tr_c,
               box._half_c, L.ptr(o), L.ptr(d), L.ptr(f.time), L.c_i(H), L.c_i(W), L.c_l(first), L.ptr(weights_sum), L.ptr(depth),
               L.ptr(pts), L.ptr(skip), L.ptr(t_buf), L.stream())
        f.evaluate(pts, skip, sdf)
        L.call("psdf_slice_cut_resolve", L.c_i(count), L.ptr(sdf), L.ptr(skip), L.ptr(t_buf), *colours, L.c_i(H), L.c_i(W),
               L.c_l(first), L.ptr(rgb), L.ptr(depth), L.ptr(weights_sum), L.ptr(mask), L.stream())
    return mask
