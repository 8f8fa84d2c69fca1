"""Frame renderer: a held-out view rendered on the device into planar images, volumetrically (csrc/frame_rays.hip,
csrc/frame_composite.hip, csrc/frame_plan.h) or sphere-traced (csrc/sampling.hip: trace_select_*, csrc/frame_trace.hip).  The
camera, its rays and the chunking are frame.py's; `Frame`, `FramePlan` and `frame_rays` are importable from here as well.

The reference renders its evaluation views with permuto_sdf_py/experiments/evaluation/create_my_images.py: run_net_in_chunks
(train_permuto_sdf.py:172-209) over create_rays_from_frame (nerf_utils.py:459-500), 3 000 rays per chunk, every chunk's
results appended to Python lists, concatenated, and transposed into images (lin2nchw).  Here

  * `FrameRenderer(trainer).render(frame)`    -> `RenderedFrame`: rgb, rgb_bg, normals, normals_cam, weights_sum as [C, H, W]
                                              float32 tensors on the device;
  * `FrameRenderer(trainer).render_traced(frame)` -> `TracedFrame`: rgb, normals, normals_cam, weights_sum, depth of the
                                              surface a sphere trace finds (below);
  * `FrameRenderer.render_views(frames)`      -> [N, 3, H, W], what `image_eval.evaluate_views` takes (`mode="traced"`: the
                                              sphere-traced colours);
  * `FrameRenderer.slice(plane)`              -> `sdf_slice.SliceImage`: the isolines of the SDF net on a layer, inside the cube of
                                              the occupancy grid (sdf_slice.py; `sdf_slice.cut_slice_into` cuts such a layer into
                                              the planes of a traced frame).

A frame is cut into chunks by `psdf_frame_plan`: the largest multiple of 64 rays whose uniform samples cannot overflow the
march's sample pool (32 768 rays at the reference's pool and 64 samples per ray: 59 chunks for 1600 x 1200 instead of 640).
Per chunk: rays -> the trainer's sampling path (sphere intersection, occupancy march, two importance rounds; one host wait for
the march's counts) -> SDF net with its input gradient (first order only) -> colour net -> one compositing launch that writes
radiance, normals and the weight sum at the chunk's pixel offset of the planes -> background net and one more launch that adds
the background.  Evaluation mode throughout (no jitter), no colour calibration (the reference passes None).

A sphere-traced frame is the reference's run_net_sphere_traced (train_permuto_sdf.py:211-242 over sdf_utils.py:120-218, called
by render_from_frame.py:335): the surface render used for inspection and figures.  Chunks come from the same plan with one
sample per ray (1920 x 1080 is one chunk).  Per chunk: rays -> `SphereTracer.trace` (end points, no gradients) -> one select
call that keeps the rays whose end point lies in an occupied voxel strictly inside the bounding sphere and compacts them in ray
order (one host wait, for their number M) -> SDF net with its input gradient and colour net on the M points (neither runs with
M = 0) -> one resolve launch that writes colour, normal, coverage and depth at the chunk's pixel offset, zeros where nothing is
hit.  One sample of weight 1 per ray: the planes hold the networks' outputs bit for bit.

Rendering reads a training run and leaves it as it was: parameters, gradients, iteration and ray counters, `rgb.last_inv_s`
(the occupancy refresh reads it) and the device's random state are not written.  Image files are not handled here.  CPU tensors
raise PsdfError: there is no CPU path.
"""
import dataclasses
import functools
from typing import Optional

import torch

from . import _lib as L
from .box_trace import Box
from .bridge import OccupancyGrid, Sphere
from .encoding import PermutoEncodingFunc
from .frame import (IT_WINDOW_OPEN, Frame, FramePlan, _f32, frame_device, frame_rays, new_planes, sample_pool,  # noqa: F401
                    stack_views)                      # (Frame: for the callers that know it as render.Frame)
from .mesh_color import MeshColorizer
from .sdf_slice import render_slice
from .sphere_trace import SphereTracer


def frame_composite_neus_raw(rs, sdf, gradients, rgb, inv_s, cos_anneal_ratio, height, width, pixel_first, rgb_img, normals_img,
                             weights_sum_img, transmittance, normals_cam_img=None, rot_cam_world=None):
    """csrc/frame_composite.hip, foreground: the container `rs` with its per-sample sdf [N, 1], gradients [N, 3] and rgb [N, 3]
    (all None for a container without samples) rendered into the planes at pixel_first + ray; transmittance [>= R] receives the
    background transmittance of every ray"""
    L.require_cuda(rgb_img, normals_img, weights_sum_img, transmittance, inv_s)
    dirs, dt = (rs.samples_dirs, rs.samples_dt) if sdf is not None else (None, None)
    L.call("psdf_frame_composite_neus", *rs._ri(), L.ptr(sdf), L.ptr(dirs), L.ptr(gradients), L.ptr(dt), L.ptr(rgb), L.ptr(inv_s),
           L.c_f(float(cos_anneal_ratio)), L.ptr(rot_cam_world), L.c_i(int(height)), L.c_i(int(width)), L.c_l(int(pixel_first)),
           L.ptr(rgb_img), L.ptr(normals_img), L.ptr(normals_cam_img), L.ptr(weights_sum_img), L.ptr(transmittance), L.stream())


def frame_composite_nerf_raw(rs, raw_density, rgb, transmittance, height, width, pixel_first, rgb_img, rgb_bg_img):
    """csrc/frame_composite.hip, background: rgb_bg_img <- transmittance * render(background container), rgb_img += that"""
    L.require_cuda(rgb_img, rgb_bg_img, transmittance)
    L.call("psdf_frame_composite_nerf", *rs._ri(), L.ptr(raw_density), L.ptr(rs.samples_dt), L.ptr(rgb), L.ptr(transmittance),
           L.c_i(int(height)), L.c_i(int(width)), L.c_l(int(pixel_first)), L.ptr(rgb_img), L.ptr(rgb_bg_img), L.stream())


def trace_frame_select_raw(grid, sphere, pts, dirs, no_hit, scratch, slot, pos, dirs_out, count):
    """csrc/sampling.hip, trace_select_*: the rays whose end point `pts` is a valid surface point (not `no_hit`, in an occupied
    voxel of `grid`, strictly inside `sphere`), compacted in ray order -> slot [R] int32 (dense row or -1), pos / dirs_out
    [>= M, 3], count [1] int32 = M; scratch: 2 * ceil(R / 256) int32"""
    L.require_cuda(pts, dirs, no_hit, scratch, slot, pos, dirs_out, count)
    L.call("psdf_trace_frame_select", L.c_i(pts.shape[0]), *grid._grid_args(), L.ptr(grid._occ()), L.c_f(sphere.m_radius),
           (L.c_f * 3)(*sphere.m_center), L.ptr(pts), L.ptr(dirs), L.ptr(no_hit), L.ptr(scratch), L.ptr(slot), L.ptr(pos),
           L.ptr(dirs_out), L.ptr(count), L.stream())


def trace_frame_resolve_raw(slot, nr_valid, origins, dirs, pos, gradients, rgb, height, width, pixel_first, rgb_img, normals_img,
                            weights_sum_img, depth_img, normals_cam_img=None, rot_cam_world=None):
    """csrc/frame_trace.hip: the chunk's rays written into the planes at pixel_first + ray: colour, normalised gradient, 1 and
    the depth along the ray for the rays with a slot (rows of the dense pos / gradients / rgb [nr_valid, 3], None with
    nr_valid = 0), zeros for the others"""
    L.require_cuda(slot, origins, dirs, rgb_img, normals_img, weights_sum_img, depth_img)
    L.call("psdf_trace_frame_resolve", L.c_i(slot.shape[0]), L.c_i(int(nr_valid)), L.ptr(slot), L.ptr(origins), L.ptr(dirs),
           L.ptr(pos), L.ptr(gradients), L.ptr(rgb), L.ptr(rot_cam_world), L.c_i(int(height)), L.c_i(int(width)),
           L.c_l(int(pixel_first)), L.ptr(rgb_img), L.ptr(normals_img), L.ptr(normals_cam_img), L.ptr(weights_sum_img),
           L.ptr(depth_img), L.stream())


@dataclasses.dataclass
class RenderedFrame:
    """float32 planes on the device: what run_net_in_chunks returns (train_permuto_sdf.py:204-209), plus the camera-frame
    normals of rotate_normals_to_cam_frame when asked for"""
    rgb: torch.Tensor                       # [3, H, W] foreground + transmittance * background (foreground alone with a mask)
    rgb_bg: Optional[torch.Tensor]          # [3, H, W] transmittance * background; None in with_mask mode
    normals: torch.Tensor                   # [3, H, W] normalised integral of the SDF gradient, world frame
    normals_cam: Optional[torch.Tensor]     # [3, H, W] the same in the camera's frame; None unless asked for
    weights_sum: torch.Tensor               # [1, H, W]


@dataclasses.dataclass
class TracedFrame:
    """float32 planes on the device: what run_net_sphere_traced returns (train_permuto_sdf.py:237-242) as images, plus the
    camera-frame normals when asked for and the depth"""
    rgb: torch.Tensor                       # [3, H, W] the colour net at the surface point, 0 where nothing is hit (no background)
    normals: torch.Tensor                   # [3, H, W] normalised SDF gradient at the surface point, world frame, 0 elsewhere
    normals_cam: Optional[torch.Tensor]     # [3, H, W] the same in the camera's frame; None unless asked for
    weights_sum: torch.Tensor               # [1, H, W] 1 where the ray ends on a valid surface point, else 0
    depth: torch.Tensor                     # [1, H, W] dot(p - o, d): distance from the camera centre along the unit ray, else 0


@functools.lru_cache(maxsize=None)
def _models_holder():
    from .train_step import Trainer      # (not at import time: train_step pulls in the optimiser and the collectives)

    class _Models(Trainer):
        """what rendering reads of a Trainer -- networks, occupancy grid, bounding sphere, hyper-parameters -- with the trainer's
        sampling path (Trainer._samples) and without an optimiser.  Trainer.__init__ is not run (it builds the optimiser and its
        moments): the fields below are what Trainer._samples, _samples_begin, _pinned and _params_ready read, and
        tests/test_frame_host.py holds this list to their source."""

        def __init__(self, sdf, rgb, bg, grid, sphere, hp, with_mask, device):
            self.sdf, self.rgb, self.bg, self.grid, self.sphere, self.hp = sdf, rgb, bg, grid, sphere, hp
            self.with_mask, self.dev = bool(with_mask), torch.device(device)
            self._pinned_counts, self._pinned_flip, self.iter = None, 0, 0
            self._pending_gather = {}       # (no collective is ever in flight here)

        def _param_key(self):
            return None        # nothing here knows when the parameters change: the packed weights are never shared

    return _Models


class FrameRenderer:
    def __init__(self, trainer):
        """trainer: a train_step.Trainer, or anything with `sdf`, `rgb`, `bg`, `grid`, `sphere`, `hp` and `with_mask`"""
        if not hasattr(trainer, "_samples"):
            dev = next(trainer.sdf.parameters()).device
            trainer = _models_holder()(trainer.sdf, trainer.rgb, trainer.bg, trainer.grid, trainer.sphere, trainer.hp,
                                       trainer.with_mask, dev)
        self.trainer = trainer

    @staticmethod
    def from_checkpoint(folder, device, hp=None, with_mask=False):
        """the networks and the occupancy grid of train_step.py, loaded from the reference's file set in `folder`
        (checkpoint.load)"""
        from . import checkpoint
        from .train_step import BgNet, HyperParams, RgbNet, SdfNet
        hp = hp or HyperParams()
        dev = torch.device(device)
        L.require_cuda(torch.empty(0, device=dev))
        sdf, rgb, bg = SdfNet(hp).to(dev), RgbNet(hp).to(dev), BgNet().to(dev)
        grid = OccupancyGrid(256, 1.0, [0, 0, 0], device=dev)
        checkpoint.load(folder, sdf=sdf, rgb=rgb, bg=bg, grid=grid, map_location=dev)
        return FrameRenderer(_models_holder()(sdf, rgb, bg, grid, Sphere(0.5, [0, 0, 0]), hp, with_mask, dev))

    def _sdf_and_gradient(self, points, it):
        """SdfNet.sdf_and_gradient (models.py:236-251) without the second-order graph: the same forward and the same
        input-gradient kernels, create_graph=False, and a lattice that is read as a constant (no touched-row marks, no lattice
        gradient) -> (sdf [N, 1], gradient [N, 3], geometry features [N, g]), all detached"""
        net = self.trainer.sdf
        e = net.encoding
        with torch.enable_grad():
            points = points.detach().requires_grad_(True)
            enc = PermutoEncodingFunc.apply(e.cfg, e.scale_factor, e.random_shift_per_level.detach(), e.lattice_values.detach(),
                                            points, net.window(it), False)
            y = net.mlp_sdf(enc)
            sdf, feat = y[:, 0:1], y[:, 1:]
            with net.mlp_sdf.input_gradient_only():
                (grad,) = torch.autograd.grad(sdf, points, torch.ones_like(sdf), create_graph=False, retain_graph=False)
        return sdf.detach(), grad.detach(), feat.detach()

    def _inv_s(self, forced_variance):
        """RgbNet.neus_weights' inverse standard deviation, without writing `last_inv_s`"""
        rgb = self.trainer.rgb
        v = rgb.variance.detach() if forced_variance is None else torch.tensor(float(forced_variance), device=self.trainer.dev)
        return torch.exp(v * 10.0).clip(1e-6, 1e6).view(1)

    def _chunk(self, frame, first, count, it, cos_anneal_ratio, inv_s, out, transmittance, rot):
        """one chunk, start to finish; nothing it allocates outlives it"""
        t = self.trainer
        H, W = frame.height, frame.width
        o, d = frame_rays(frame, first, count)
        fg, bg = t._samples(o, d, it, jitter=False)
        if fg.samples_pos.shape[0] == 0:
            sdf = grad = rgb = None
        else:
            sdf, grad, feat = self._sdf_and_gradient(fg.samples_pos, it)
            rgb = _f32(t.rgb(fg.samples_pos, fg.samples_dirs, grad, feat))
            sdf, grad = _f32(sdf).view(-1, 1), _f32(grad)
        frame_composite_neus_raw(fg, sdf, grad, rgb, inv_s, cos_anneal_ratio, H, W, first, out.rgb, out.normals, out.weights_sum,
                                 transmittance, out.normals_cam, rot)
        if bg is not None:
            rgb_bg, dens = t.bg(bg.samples_pos_4d, bg.samples_dirs)
            frame_composite_nerf_raw(bg, _f32(dens).reshape(-1), _f32(rgb_bg), transmittance, H, W, first, out.rgb, out.rgb_bg)

    @torch.no_grad()
    def render(self, frame, it=None, cos_anneal_ratio=1.0, forced_variance="finish", pool_samples=OccupancyGrid.POOL,
               camera_normals=False):
        """-> RenderedFrame.  Defaults as create_my_images.py: evaluation mode, the lattice window fully open (`it` None; else
        the annealing iteration whose window to use), the variance forced to hp.forced_variance_finish ("finish"; a number
        forces that variance, None uses the learned one), no colour calibration.  pool_samples: the sample pool of the occupancy
        march, which bounds the rays of a chunk (FramePlan)."""
        t = self.trainer
        hp = t.hp
        dev = frame_device(frame, t.sdf)
        plan = FramePlan(frame.height, frame.width, hp.max_nr_samples_per_ray, pool_samples)
        it = IT_WINDOW_OPEN if it is None else it
        if isinstance(forced_variance, str):
            if forced_variance != "finish":
                raise ValueError("forced_variance must be 'finish', a number or None, got %r" % (forced_variance,))
            forced_variance = hp.forced_variance_finish
        inv_s = self._inv_s(forced_variance)
        t._params_ready()                     # a data-parallel trainer's parameters may still be on their way
        planes = functools.partial(new_planes, frame, dev=dev)
        out = RenderedFrame(rgb=planes(3), rgb_bg=None if t.with_mask else planes(3), normals=planes(3),
                            normals_cam=planes(3) if camera_normals else None, weights_sum=planes(1))
        rot = frame.rot_cam_world() if camera_normals else None
        transmittance = torch.empty(plan.rays_per_chunk, dtype=torch.float32, device=dev)
        with sample_pool(t.grid, pool_samples):
            for first, count in plan.chunks():
                self._chunk(frame, first, count, it, cos_anneal_ratio, inv_s, out, transmittance, rot)
        return out

    def _traced_chunk(self, frame, first, count, tracer, trace_args, it, out, rot, work):
        """one chunk of a sphere-traced frame, start to finish"""
        t = self.trainer
        scratch, slot, pos, dirs, nr_valid = work
        o, d = frame_rays(frame, first, count)
        pts = tracer.trace(o, d, *trace_args, return_gradients=False)[0]
        trace_frame_select_raw(t.grid, t.sphere, pts, d, tracer.no_hit, scratch, slot[:count], pos, dirs, nr_valid)
        # the one host wait of the chunk: how many rays ended on the surface
        pinned = t._pinned(1)
        pinned[:1].copy_(nr_valid, non_blocking=True)
        event = torch.cuda.Event()
        event.record()
        event.synchronize()
        M = int(pinned[0])
        if M == 0:
            p = grad = rgb = None
        else:
            p = pos[:M]
            _, grad, feat = self._sdf_and_gradient(p, it)
            rgb = _f32(t.rgb(p, dirs[:M], grad, feat))
            grad = _f32(grad)
        trace_frame_resolve_raw(slot[:count], M, o, d, p, grad, rgb, frame.height, frame.width, first, out.rgb, out.normals,
                                out.weights_sum, out.depth, out.normals_cam, rot)

    @torch.no_grad()
    def render_traced(self, frame, it=None, nr_sphere_traces=15, sdf_multiplier=0.9, sdf_converged_tresh=2e-4,
                      camera_normals=False, max_rays_per_chunk=OccupancyGrid.POOL):
        """-> TracedFrame: the surface a sphere trace finds, as run_net_sphere_traced renders it.  Defaults as
        render_from_frame.py:335; `it` as in `render` (None: the lattice window fully open).  max_rays_per_chunk bounds the rays
        traced at once (FramePlan with one sample per ray)."""
        t = self.trainer
        net = t.sdf
        dev = frame_device(frame, net)
        plan = FramePlan(frame.height, frame.width, 1, max_rays_per_chunk)
        it = IT_WINDOW_OPEN if it is None else it
        t._params_ready()                     # a data-parallel trainer's parameters may still be on their way
        tracer = SphereTracer(net.encoding, net.mlp_sdf, t.grid, t.sphere, _f32(net.window(it)))
        planes = functools.partial(new_planes, frame, dev=dev)
        out = TracedFrame(rgb=planes(3), normals=planes(3), normals_cam=planes(3) if camera_normals else None,
                          weights_sum=planes(1), depth=planes(1))
        rot = frame.rot_cam_world() if camera_normals else None
        R = plan.rays_per_chunk
        work = (torch.empty(2 * ((R + 255) // 256), dtype=torch.int32, device=dev), torch.empty(R, dtype=torch.int32, device=dev),
                torch.empty((R, 3), dtype=torch.float32, device=dev), torch.empty((R, 3), dtype=torch.float32, device=dev),
                torch.empty(1, dtype=torch.int32, device=dev))
        for first, count in plan.chunks():
            self._traced_chunk(frame, first, count, tracer, (nr_sphere_traces, sdf_multiplier, sdf_converged_tresh), it, out, rot,
                               work)
        return out

    def box(self):
        """the axis-aligned box of the scene, as a box_trace.Box: the cube of the occupancy grid"""
        g = self.trainer.grid
        return Box([g.m_grid_extent] * 3, g.m_grid_translation)

    def slice(self, plane, size=500, box=None, **kw):
        """-> sdf_slice.SliceImage: the isolines of the SDF net on `plane` (a sdf_slice.SlicePlane), as
        render_from_frame.py:71-166 draws them; box: default `self.box()`; kw: sdf_slice.render_slice's (`it` None: the lattice
        window fully open)"""
        self.trainer._params_ready()
        return render_slice(self.trainer.sdf, plane, self.box() if box is None else box, size, **kw)

    def mesh_colorizer(self, it=None):
        """-> mesh_color.MeshColorizer over the SDF and the colour network (`it` None: the lattice window fully open)"""
        self.trainer._params_ready()
        return MeshColorizer(self.trainer.sdf, self.trainer.rgb, it)

    def colored_mesh(self, nr_points_per_dim, min_val=-0.5, max_val=0.5, it=None, **extract_kw):
        """-> mesh.ExtractedMesh of the SDF's zero set with per-vertex colours `C` [V, 3] uint8 (each vertex seen head-on from
        outside); extract_kw: MeshExtractor.extract's"""
        from .mesh import MeshExtractor
        colorizer = self.mesh_colorizer(it)
        mesh = MeshExtractor.from_sdf_net(self.trainer.sdf, colorizer.it).extract(nr_points_per_dim, min_val, max_val, **extract_kw)
        return colorizer.colorize(mesh)

    def render_views(self, frames, mode="volumetric", **kwargs):
        """-> [N, 3, H, W] float32: the rgb of every frame (all of one size), ready for image_eval.evaluate_views; mode
        "volumetric": `render`, "traced": `render_traced`"""
        if mode not in ("volumetric", "traced"):
            raise ValueError("mode must be 'volumetric' or 'traced', got %r" % (mode,))
        return stack_views(self.render if mode == "volumetric" else self.render_traced, frames, **kwargs)
