"""Grid-free sphere tracing inside an axis-aligned box: traced views of fitted 3-D and 4-D SDFs (csrc/box_trace.hip).

The reference looks at the nets of train_sdf_from_mesh.py (:193) and train_4d_sdf.py (:268, and the whole of
experiments/visualization/vis_4d_sdf.py) by sphere-tracing them inside an `AABB` with no occupancy grid, at a `time_val` for a
4-D net (permuto_sdf_py/utils/sdf_utils.py:120-218, the `occupancy_grid=None` branch), and writes (normal + 1) / 2 with the
convergence mask as alpha, once per time step.  Here

  * `Box(sizes_xyz, translation)`           the reference's AABB (permuto_sdf_py/utils/aabb.py): `ray_intersection` through the
                                            kernel, `check_point_inside_primitive` and `rand_points_inside` in plain torch;
  * `BoxTracer(encoding, mlp, box, window)` `SphereTracer`'s launch sequence with the box kernels in place of the grid kernels:
                                            begin -> [masked encode -> masked MLP (1-row head) -> step] x n -> masked final SDF ->
                                            masked MLP data backward of a unit gradient -> masked position backward (its first
                                            three columns are the normal).  One slot per ray, no host wait: `capture` records the
                                            sequence once, `replay(t)` fills ONE float on the device and replays it;
  * `render_box_traced(net, box, frame)`    -> `BoxTracedFrame`: normals, normals_cam, weights_sum, depth as [C, H, W] planes;
  * `BoxPlayer(net, box, frame)`            rays, trace and resolve of a one-chunk frame captured once; `frame_at(t)` is one
                                            fill and one replay: playing a fitted 4-D field.

Two stated deviations from the reference.  Rays that miss the box are reported as `SphereTracer` reports rays that met no
occupancy -- converged, point at the ray origin, sdf = 0, gradient 0, never evaluated (`no_hit` tells them apart) -- where the
reference traces them from the camera centre; rays are independent, so every other ray is unaffected.  And the converged rays
stay in their slots, masked out of the evaluations, instead of being compacted away with boolean masks each iteration; the end
points are the compacting loop's bit for bit (tests/test_gpu_box_trace.py).  CPU tensors raise PsdfError: there is no CPU path.
"""
import dataclasses
import functools
from typing import Optional

import numpy as np
import torch

from . import _lib as L
from .bridge import OccupancyGrid
from .frame import FramePlan, frame_device, frame_rays, new_planes, open_window
from .net_eval import masked_sdf, masked_sdf_gradient, one_row_head


def _triple(v):
    return (L.c_f * 3)(*[float(x) for x in v])


class Box:
    """AABB(bounding_box_sizes_xyz, bounding_box_translation) of permuto_sdf_py/utils/aabb.py.  The bounds are computed in
    float32 in the reference's order: bb_min = -sizes / 2 + translation, bb_max = sizes - sizes / 2 + translation (aabb.py:48-49;
    NOT sizes / 2 + translation) for the intersection; min / max_bounds = -+ sizes / 2 about the translation for the inside test
    (aabb.py:15-25)."""

    def __init__(self, sizes_xyz, translation=(0.0, 0.0, 0.0)):
        sizes = [float(x) for x in (sizes_xyz.tolist() if hasattr(sizes_xyz, "tolist") else sizes_xyz)]
        trans = [float(x) for x in (translation.tolist() if hasattr(translation, "tolist") else translation)]
        if len(sizes) != 3 or len(trans) != 3 or not all(s > 0 for s in sizes):
            raise ValueError("Box takes three positive sizes and three translations, got %r and %r" % (sizes_xyz, translation))
        self.sizes_xyz, self.translation = sizes, trans
        s, t, two = np.asarray(sizes, np.float32), np.asarray(trans, np.float32), np.float32(2.0)
        self.bb_min = -s / two + t
        self.bb_max = s - s / two + t
        self.half = np.asarray([x / 2 for x in sizes], np.float32)      # max_bounds; min_bounds is its negative
        self._min_c, self._max_c, self._tr_c, self._half_c = _triple(self.bb_min), _triple(self.bb_max), _triple(t), _triple(self.half)

    def ray_intersection(self, ray_origins, ray_dirs):
        """-> (entry points [R, 3], t_entry [R, 1], exit points [R, 3], t_exit [R, 1], does_ray_intersect_box [R, 1] bool):
        aabb.py:47-100 in one launch; both depths are 0 for a ray that misses, t_entry is 0 for a camera inside the box"""
        L.require_cuda(ray_origins, ray_dirs)
        o, d = ray_origins.to(torch.float32).contiguous(), ray_dirs.to(torch.float32).contiguous()
        R, dev = o.shape[0], o.device
        te, tx = (torch.empty((R, 1), dtype=torch.float32, device=dev) for _ in range(2))
        pe, px = (torch.empty((R, 3), dtype=torch.float32, device=dev) for _ in range(2))
        hit = torch.empty((R, 1), dtype=torch.bool, device=dev)
        L.call("psdf_box_ray_intersection", L.c_i(R), self._min_c, self._max_c, L.ptr(o), L.ptr(d), L.ptr(te), L.ptr(tx), L.ptr(pe),
               L.ptr(px), L.ptr(hit), L.stream())
        return pe, te, px, tx, hit

    def check_point_inside_primitive(self, points):
        """[N, 1] bool: strictly inside on all three axes (aabb.py:28-42); columns past the third are ignored.  Plain torch."""
        q = points[:, :3] - torch.as_tensor(self.translation, dtype=points.dtype, device=points.device)
        half = torch.as_tensor(self.half, device=points.device).to(points.dtype)
        return torch.logical_and(q < half, q > -half).all(dim=-1, keepdim=True)

    def rand_points_inside(self, nr_points, device=None, generator=None):
        """[n, 3] uniform points of the box (aabb.py:110-114).  Plain torch."""
        s, t = (torch.tensor(v, dtype=torch.float32, device=device) for v in (self.sizes_xyz, self.translation))
        return torch.rand((int(nr_points), 3), device=device, generator=generator) * s - s / 2 + t


class BoxTracer:
    def __init__(self, encoding, mlp, box, window=None):
        self.enc, self.mlp, self.box = encoding, mlp, box
        self.pos_dim = int(encoding.cfg.pos_dim)
        if self.pos_dim not in (3, 4):
            raise ValueError("BoxTracer takes a 3-D or a 4-D encoding, got pos_dim = %d" % self.pos_dim)
        dev = encoding.lattice_values.device
        window = window if window is not None else torch.ones(encoding.nr_levels, device=dev)
        self.window = window.detach().to(device=dev, dtype=torch.float32).contiguous()
        # the ONE float a captured trace reads its time from (column 3 of every point, written by the begin kernel)
        self._time = torch.zeros(1, dtype=torch.float32, device=dev)
        self._graph = None
        self.no_hit = None

    # ---- building blocks -----------------------------------------------------------------------------------
    def _sdf(self, pts, dims, packed, skip=None, out=None, feat_buf=None):
        """SDF channel of the net at `pts` [N, P] -> (feat [C, N], sdf [1, N]): net_eval.masked_sdf (masked points are not
        evaluated and keep their entries of `out`).  A method so that a test can put a field of its own in its place."""
        return masked_sdf(self.enc, self.window, dims, packed, pts, skip=skip, out=out, feat_buf=feat_buf)

    def _check_time(self, time_val):
        if self.pos_dim == 4 and time_val is None:
            raise ValueError("a 4-D field is traced at a time: pass time_val")
        if self.pos_dim == 3 and time_val is not None:
            raise ValueError("a 3-D field has no time: time_val must be None")

    def _launch(self, o, d, nr_sphere_traces, sdf_multiplier, sdf_converged_tresh, return_gradients):
        """the fixed launch list; the time is whatever `self._time` holds when it RUNS"""
        P, box = self.pos_dim, self.box
        R, dev = o.shape[0], o.device
        pts = torch.empty((R, P), dtype=torch.float32, device=dev)
        conv = torch.empty((R, 1), dtype=torch.bool, device=dev)
        no_hit = torch.empty(R, dtype=torch.bool, device=dev)
        L.call("psdf_box_trace_begin", L.c_i(R), L.c_i(P), box._min_c, box._max_c, L.ptr(o), L.ptr(d),
               L.ptr(self._time) if P == 4 else None, L.ptr(pts), L.ptr(conv), L.ptr(no_hit), L.stream())
        self.no_hit = no_hit
        # channel 0 of the last layer is the SDF (models.py:190-192): a 1-row head
        head = one_row_head(self.mlp, pack=True)
        dims, packed = head.dims, head.packed
        sdf = torch.zeros((1, R), dtype=torch.float32, device=dev)
        feat_buf = torch.zeros((self.enc.cfg.channels, R), dtype=torch.float32, device=dev)
        for _ in range(nr_sphere_traces):
            self._sdf(pts, dims, packed, skip=conv.view(-1), out=sdf, feat_buf=feat_buf)      # converged rays are skipped
            L.call("psdf_box_trace_step", L.c_i(R), L.c_i(P), box._tr_c, box._half_c, L.ptr(d), L.ptr(sdf), L.c_f(sdf_multiplier),
                   L.c_f(sdf_converged_tresh), L.ptr(pts), L.ptr(conv), L.stream())
        # final SDF (+ analytic normal) at the end points of the rays that entered the box
        sdf.zero_()
        feat, sdf = self._sdf(pts, dims, packed, skip=no_hit, out=sdf, feat_buf=feat_buf)
        # the masked MLP evaluates a partly masked 32-sample tile in full, and writes all of it: a ray that missed the box would
        # hold the net's value at zero features.  It was never evaluated and reports 0.
        sdf.masked_fill_(no_hit.view(1, -1), 0.0)
        # the level groups of the position backward meet in the call's scratch, in group order: the captured trace's normals are
        # the eager trace's bit for bit
        grads = masked_sdf_gradient(self.enc, self.window, head, pts, feat, no_hit, scratch=True) if return_gradients else None
        # rows of P floats, as the resolve kernel reads them
        self._rows = (pts, sdf, grads)
        return (pts if P == 3 else pts[:, :3], sdf.reshape(-1, 1), None if grads is None else (grads if P == 3 else grads[:, :3]),
                conv)

    def _rays(self, ray_origins, ray_dirs):
        L.require_cuda(ray_origins, ray_dirs)
        o, d = ray_origins.to(torch.float32).contiguous(), ray_dirs.to(torch.float32).contiguous()
        if o.dim() != 2 or o.shape[1] != 3 or d.shape != o.shape:
            raise ValueError("rays are origins [R, 3] and directions [R, 3], got %s and %s" % (tuple(o.shape), tuple(d.shape)))
        return o, d

    @torch.no_grad()
    def trace(self, ray_origins, ray_dirs, nr_sphere_traces=20, sdf_multiplier=0.9, sdf_converged_tresh=2e-4, time_val=None,
              return_gradients=True):
        """-> pts [R, 3], sdf [R, 1], sdf_gradients [R, 3] or None, converged [R, 1] bool (views of rows of 4 floats for a
        4-D field).  Defaults as train_sdf_from_mesh.py:193.  `self.no_hit` [R] bool: the rays that missed the box -- reported
        converged, point at the origin, sdf = 0, gradient = 0, never evaluated."""
        self._check_time(time_val)
        o, d = self._rays(ray_origins, ray_dirs)
        if time_val is not None:
            self._time.fill_(float(time_val))
        return self._launch(o, d, int(nr_sphere_traces), float(sdf_multiplier), float(sdf_converged_tresh), bool(return_gradients))

    # ---- hipGraph ------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def capture(self, ray_origins, ray_dirs, nr_sphere_traces=20, sdf_multiplier=0.9, sdf_converged_tresh=2e-4, time_val=None,
                return_gradients=True):
        """Capture one full trace for rays of this shape: one stream, a linear launch list.  `replay(t)` re-runs it on the
        CURRENT contents of the two ray tensors (`self._o`, `self._d`: update them in place) at time t and returns the same
        output tensors every time."""
        self._check_time(time_val)
        self._o, self._d = self._rays(ray_origins, ray_dirs)
        args = (int(nr_sphere_traces), float(sdf_multiplier), float(sdf_converged_tresh), bool(return_gradients))
        if time_val is not None:
            self._time.fill_(float(time_val))           # outside the capture: the graph READS the time, it never sets it
        self._launch(self._o, self._d, *args)            # warm-up outside capture (allocator, lazy init)
        torch.cuda.synchronize()
        self._graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self._graph):
            self._out = self._launch(self._o, self._d, *args)
        self._graph.replay()                             # (a capture runs nothing: the outputs hold this time's trace from here on)
        return self._out

    def replay(self, time_val=None):
        """one fill of the time (a 4-D field; None keeps the last one) and one replay"""
        if time_val is not None:
            if self.pos_dim == 3:
                raise ValueError("a 3-D field has no time: time_val must be None")
            self._time.fill_(float(time_val))
        self._graph.replay()
        return self._out


# ---------------------------------------------------------------------------------------------------------------- frames
@dataclasses.dataclass
class BoxTracedFrame:
    """float32 planes on the device: what vis_4d_sdf.py:106-118 shows, before its (n + 1) / 2 colour map.  No colour: these nets
    have none."""
    normals: torch.Tensor                   # [3, H, W] normalised SDF gradient at the end point of a covered ray, else 0
    normals_cam: Optional[torch.Tensor]     # [3, H, W] the same in the camera's frame; None unless asked for
    weights_sum: torch.Tensor               # [1, H, W] 1 where the ray entered the box and ended with sdf < coverage_tresh, else 0
    depth: torch.Tensor                     # [1, H, W] dot(p - o, d) of a covered ray, else 0


def box_trace_resolve_raw(tracer, origins, dirs, coverage_tresh, height, width, pixel_first, out, rot_cam_world=None):
    """csrc/box_trace.hip: the rays `tracer` traced last written into the planes of `out` at pixel_first + ray"""
    pts, sdf, grads = tracer._rows
    if grads is None:
        raise ValueError("the planes need the gradients: trace with return_gradients=True")
    L.call("psdf_box_trace_resolve", L.c_i(pts.shape[0]), L.c_i(pts.shape[1]), L.ptr(origins), L.ptr(dirs), L.ptr(pts), L.ptr(sdf),
           L.ptr(grads), L.ptr(tracer.no_hit), L.c_f(float(coverage_tresh)), L.ptr(rot_cam_world), L.c_i(int(height)),
           L.c_i(int(width)), L.c_l(int(pixel_first)), L.ptr(out.normals), L.ptr(out.normals_cam), L.ptr(out.weights_sum),
           L.ptr(out.depth), L.stream())


def _frame_setup(net, frame, it, camera_normals, max_rays_per_chunk):
    dev = frame_device(frame, net)
    plan = FramePlan(frame.height, frame.width, 1, max_rays_per_chunk)
    window = open_window(net, it)
    planes = functools.partial(new_planes, frame, dev=dev)
    out = BoxTracedFrame(normals=planes(3), normals_cam=planes(3) if camera_normals else None, weights_sum=planes(1), depth=planes(1))
    return plan, window, out, (frame.rot_cam_world() if camera_normals else None)


_POOL = OccupancyGrid.POOL      # the rays FrameRenderer.render_traced traces at once


@torch.no_grad()
def render_box_traced(net, box, frame, it=None, time_val=None, nr_sphere_traces=20, sdf_multiplier=0.9, sdf_converged_tresh=2e-4,
                      coverage_tresh=0.01, camera_normals=False, max_rays_per_chunk=_POOL):
    """-> BoxTracedFrame of the field of `net` (anything with `encoding`, `mlp_sdf` and `window(it)`) inside `box`, at
    `time_val` for a 4-D net.  it: the iteration whose coarse-to-fine window is used (None: fully open).  coverage_tresh:
    filter_unconverged_points' (sdf_utils.py:221).  Chunks of at most max_rays_per_chunk rays (frame.FramePlan with one
    sample per ray); per chunk: rays -> trace -> one resolve launch.  No host wait."""
    plan, window, out, rot = _frame_setup(net, frame, it, camera_normals, max_rays_per_chunk)
    tracer = BoxTracer(net.encoding, net.mlp_sdf, box, window)
    for first, count in plan.chunks():
        o, d = frame_rays(frame, first, count)
        tracer.trace(o, d, nr_sphere_traces, sdf_multiplier, sdf_converged_tresh, time_val, True)
        box_trace_resolve_raw(tracer, o, d, coverage_tresh, frame.height, frame.width, first, out, rot)
    return out


class BoxPlayer:
    """Rays, trace and resolve of ONE frame captured once (the frame must fit one chunk); `frame_at(t)` is one fill of the
    time on the device and one replay, and returns the SAME planes every time (clone what must outlive the next call).  The
    weights of the net are read when the graph runs: a player follows a net that is trained on."""

    def __init__(self, net, box, frame, it=None, coverage_tresh=0.01, camera_normals=False, max_rays_per_chunk=_POOL,
                 nr_sphere_traces=20, sdf_multiplier=0.9, sdf_converged_tresh=2e-4):
        plan, window, self._frame_out, rot = _frame_setup(net, frame, it, camera_normals, max_rays_per_chunk)
        if plan.nr_chunks != 1:
            raise ValueError("BoxPlayer plays a frame of one chunk: %d x %d is %d chunks of %d rays (render_box_traced takes any "
                             "frame)" % (frame.height, frame.width, plan.nr_chunks, plan.rays_per_chunk))
        self.tracer = tracer = BoxTracer(net.encoding, net.mlp_sdf, box, window)
        args = (int(nr_sphere_traces), float(sdf_multiplier), float(sdf_converged_tresh), True)

        def run():
            o, d = frame_rays(frame)
            tracer._launch(o, d, *args)
            box_trace_resolve_raw(tracer, o, d, coverage_tresh, frame.height, frame.width, 0, self._frame_out, rot)

        with torch.no_grad():
            run()                               # warm-up outside capture (allocator, lazy init)
            torch.cuda.synchronize()
            self._graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self._graph):
                run()

    def frame_at(self, t=None):
        """-> BoxTracedFrame at time t (a 4-D net; a 3-D net takes no time)"""
        self.tracer._check_time(t)
        if t is not None:
            self.tracer._time.fill_(float(t))
        self._graph.replay()
        return self._frame_out
