"""Frame renderer: a held-out view rendered on the device into planar images, volumetrically (csrc/frame_rays.hip,
csrc/frame_composite.hip, csrc/frame_plan.h) or sphere-traced (csrc/sampling.hip: trace_select_*, csrc/frame_trace.hip).

The reference renders its evaluation views with permuto_sdf_py/experiments/evaluation/create_my_images.py: run_net_in_chunks
(train_permuto_sdf.py:172-209) over create_rays_from_frame (nerf_utils.py:459-500), 3 000 rays per chunk, every chunk's
results appended to Python lists, concatenated, and transposed into images (lin2nchw).  Here

  * `Frame(K, tf_world_cam, height, width)`   a pinhole camera; `Frame.from_reel(reel, i)` takes image i of an image reel;
  * `frame_rays(frame, first, count)`         the rays of a range of pixels, bit-for-bit the rays training draws for them;
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
from .bridge import OccupancyGrid, Sphere
from .encoding import PermutoEncodingFunc
from .sphere_trace import SphereTracer

_PLAN_FIELDS = 3            # PSDF_FRAME_PLAN_FIELDS of include/psdf.h
_IT_WINDOW_OPEN = 9999999   # create_my_images.py:81: far past the coarse-to-fine schedule, every lattice level fully open


class FramePlan:
    """the chunking of an H x W frame, from the library's host-only entry (csrc/frame_plan.h decides it)"""

    def __init__(self, height, width, max_nr_samples_per_ray, pool_samples):
        out = (L.c_l * _PLAN_FIELDS)()
        status = L.lib().psdf_frame_plan(L.c_i(int(height)), L.c_i(int(width)), L.c_i(int(max_nr_samples_per_ray)),
                                         L.c_l(int(pool_samples)), out)
        if status == -1:
            raise ValueError("no chunking for a %d x %d frame with %d samples per ray out of a pool of %d (extents and the cap "
                             "must be positive and the pool must hold 64 rays)" % (height, width, max_nr_samples_per_ray, pool_samples))
        L.check(status, "psdf_frame_plan")
        self.rays_per_chunk, self.nr_chunks, self.last_chunk = (int(v) for v in out)

    def chunks(self):
        """-> [(first pixel, rays)]"""
        return [(i * self.rays_per_chunk, self.rays_per_chunk if i < self.nr_chunks - 1 else self.last_chunk)
                for i in range(self.nr_chunks)]


def _f32(t):
    return t.detach().to(torch.float32).contiguous()


class Frame:
    """A pinhole camera: K [3, 3], tf_world_cam [4, 4] (row-major [R|t], camera to world) and the image extents: what an image
    reel holds per image."""

    def __init__(self, K, tf_world_cam, height, width):
        K, tf = torch.as_tensor(K), torch.as_tensor(tf_world_cam)
        if tuple(K.shape) != (3, 3) or tuple(tf.shape) != (4, 4):
            raise ValueError("Frame takes K [3, 3] and tf_world_cam [4, 4], got %s and %s" % (tuple(K.shape), tuple(tf.shape)))
        if int(height) < 1 or int(width) < 1:
            raise ValueError("empty frame: %d x %d" % (height, width))
        self.K, self.tf_world_cam = _f32(K), _f32(tf)
        self.height, self.width = int(height), int(width)

    @staticmethod
    def from_reel(reel, i):
        """image `i` of anything with K_reel [I, 3, 3], tf_world_cam_reel [I, 4, 4] and rgb_reel [I, 3, H, W]"""
        H, W = reel.rgb_reel.shape[-2:]
        return Frame(reel.K_reel[i], reel.tf_world_cam_reel[i], H, W)

    @property
    def nr_pixels(self):
        return self.height * self.width

    def rot_cam_world(self):
        """[3, 3]: the rotation of tf_cam_world = tf_world_cam^-1 (the transpose of a rigid transform's rotation)"""
        return self.tf_world_cam[:3, :3].t().contiguous()


def frame_rays(frame, first=0, count=None):
    """-> (origins [n, 3], dirs [n, 3]) of the pixels [first, first + count) of `frame` (all of them from `first` on by
    default); pixel p is (x, y) = (p % W, p / W) with its centre at +0.5"""
    L.require_cuda(frame.K, frame.tf_world_cam)
    first = int(first)
    count = frame.nr_pixels - first if count is None else int(count)
    if first < 0 or count < 0 or first + count > frame.nr_pixels:
        raise ValueError("pixels [%d, %d) lie outside a %d x %d frame" % (first, first + count, frame.height, frame.width))
    dev = frame.K.device
    o = torch.empty((count, 3), dtype=torch.float32, device=dev)
    d = torch.empty((count, 3), dtype=torch.float32, device=dev)
    L.call("psdf_frame_rays", L.c_i(frame.height), L.c_i(frame.width), L.ptr(frame.K), L.ptr(frame.tf_world_cam), L.c_l(first),
           L.c_i(count), L.ptr(o), L.ptr(d), L.stream())
    return o, d


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
        dev = self._check_devices(frame)
        H, W = frame.height, frame.width
        plan = FramePlan(H, W, hp.max_nr_samples_per_ray, pool_samples)
        it = _IT_WINDOW_OPEN if it is None else it
        if isinstance(forced_variance, str):
            if forced_variance != "finish":
                raise ValueError("forced_variance must be 'finish', a number or None, got %r" % (forced_variance,))
            forced_variance = hp.forced_variance_finish
        inv_s = self._inv_s(forced_variance)
        t._params_ready()                     # a data-parallel trainer's parameters may still be on their way

        def planes(c):
            return torch.empty((c, H, W), dtype=torch.float32, device=dev)      # every pixel belongs to one chunk, which writes it

        out = RenderedFrame(rgb=planes(3), rgb_bg=None if t.with_mask else planes(3), normals=planes(3),
                            normals_cam=planes(3) if camera_normals else None, weights_sum=planes(1))
        rot = frame.rot_cam_world() if camera_normals else None
        transmittance = torch.empty(plan.rays_per_chunk, dtype=torch.float32, device=dev)
        grid_pool = t.grid.max_nr_samples
        t.grid.max_nr_samples = int(pool_samples)        # the pool the plan was made for
        try:
            for first, count in plan.chunks():
                self._chunk(frame, first, count, it, cos_anneal_ratio, inv_s, out, transmittance, rot)
        finally:
            t.grid.max_nr_samples = grid_pool
        return out

    def _check_devices(self, frame):
        """the kernels take raw pointers: no one else would notice a frame on another device than the models"""
        L.require_cuda(frame.K, frame.tf_world_cam)
        dev = frame.K.device
        models_dev = self.trainer.sdf.encoding.lattice_values.device    # (a tensor's device carries its index; `t.dev` may be a bare "cuda")
        if dev != models_dev or frame.tf_world_cam.device != dev:
            raise L.PsdfError("the frame lives on %s, the models on %s" % (dev, models_dev))
        return dev

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
        dev = self._check_devices(frame)
        H, W = frame.height, frame.width
        plan = FramePlan(H, W, 1, max_rays_per_chunk)
        it = _IT_WINDOW_OPEN if it is None else it
        t._params_ready()                     # a data-parallel trainer's parameters may still be on their way
        net = t.sdf
        tracer = SphereTracer(net.encoding, net.mlp_sdf, t.grid, t.sphere, _f32(net.window(it)))

        def planes(c):
            return torch.empty((c, H, W), dtype=torch.float32, device=dev)      # every pixel belongs to one chunk, which writes it

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
        from .box_trace import Box
        g = self.trainer.grid
        return Box([g.m_grid_extent] * 3, g.m_grid_translation)

    def slice(self, plane, size=500, box=None, **kw):
        """-> sdf_slice.SliceImage: the isolines of the SDF net on `plane` (a sdf_slice.SlicePlane), as
        render_from_frame.py:71-166 draws them; box: default `self.box()`; kw: sdf_slice.render_slice's (`it` None: the lattice
        window fully open)"""
        from .sdf_slice import render_slice
        self.trainer._params_ready()
        return render_slice(self.trainer.sdf, plane, self.box() if box is None else box, size, **kw)

    def mesh_colorizer(self, it=None):
        """-> mesh_color.MeshColorizer over the SDF and the colour network (`it` None: the lattice window fully open)"""
        from .mesh_color import MeshColorizer
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
        render = self.render if mode == "volumetric" else self.render_traced
        frames = list(frames)
        if not frames:
            raise ValueError("render_views needs at least one frame")
        if len({(f.height, f.width) for f in frames}) != 1:
            raise ValueError("render_views takes frames of one size")
        return torch.stack([render(f, **kwargs).rgb for f in frames])
