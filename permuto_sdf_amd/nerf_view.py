"""Views of a trained NeRF: a camera's frame rendered on the device into planar images, with the expected depth
(csrc/frame_composite.hip: frame_render_nerf_kernel, frame_composite_nerf_kernel; csrc/frame_rays.hip; csrc/frame_plan.h).

The reference looks at a NeRF run with run_net_in_chunks (permuto_sdf_py/train_nerf.py:92-128, called at :259 for a held-out
camera): create_rays over the whole frame, torch.chunk into 200 x 200 rays, run_net (:61-89) per chunk, every chunk's results
appended to Python lists, concatenated and transposed into images (lin2nchw) -> pred_rgb_img, pred_rgb_bg_img,
pred_weights_sum_img.  Here

  * `frame_render_nerf_raw`                   the foreground container of one chunk rendered straight into the planes at the
                                              chunk's pixel offset: radiance, weight sum, optionally the expected depth sum w z,
                                              and the transmittance buffer the background launch reads;
  * `NerfFrameRenderer(trainer).render(frame)` -> `NerfRenderedFrame`: rgb, rgb_bg, weights_sum, depth as [C, H, W] float32
                                              tensors on the device; `NerfTrainer.renderer()` builds one;
  * `NerfFrameRenderer.from_checkpoint(folder, device)` the same from the file set of `NerfTrainer.save_checkpoint`;
  * `NerfFrameRenderer.render_views(frames)`  -> [N, 3, H, W], what `image_eval.evaluate_views` takes.

The camera, its rays and the chunking are frame.py's (`Frame`, `frame_rays`, `FramePlan`: the largest multiple of 64 rays whose
samples cannot overflow the march's pool).  Per chunk: rays -> the trainer's sampling without jitter (sphere intersection,
occupancy march, compaction: one host wait, as in a training step) -> the foreground net over the raw feature-major kernels
(`NerfTrainer._branch_forward`; skipped for a chunk without foreground samples) -> one launch that writes radiance, weight sum,
depth and transmittance -> unless with_mask, the background net on the inverse-depth samples and one more launch that adds
transmittance x background.  A NeRF has no surface and so no normal plane; the depth is the expectation of the samples' z
under the rendering weights, not normalised by the weight sum (divide by `weights_sum` where it is not zero for the mean).

Rendering reads a run and leaves it as it was: parameters, gradients, optimiser moments, `iter`, the grid's values and pool
size, the lattices' touched-rows buffers and the device's random state are not written.  No colour calibration (the reference
renders views with model_colorcal=None, train_nerf.py:107): of a run trained with `NerfTrainer(nr_images=...)` a view carries
the calibration of the fixed image, the identity.  No image files.  CPU tensors raise PsdfError: there is no CPU path.
"""
import dataclasses
import functools
import os
from types import SimpleNamespace
from typing import Optional

import torch

from . import _lib as L
from .bridge import OccupancyGrid, Sphere
from .frame import IT_WINDOW_OPEN, FramePlan, frame_device, frame_rays, new_planes, sample_pool, stack_views
from .nerf_train import FILES, HyperParams, NerfNet, NerfTrainer
from .render import frame_composite_nerf_raw


def frame_render_nerf_raw(rs, raw_density, rgb, height, width, pixel_first, rgb_img, weights_sum_img, transmittance, depth_img=None):
    """csrc/frame_composite.hip, NeRF foreground: the container `rs` with its per-sample raw_density [M] (before the softplus)
    and rgb [M, 3] (both None for a container without samples) rendered into the planes at pixel_first + ray; depth_img
    [1, H, W] (optional) receives sum w rs.samples_z; transmittance [>= R] the background transmittance of every ray"""
    L.require_cuda(rgb_img, weights_sum_img, transmittance, depth_img, raw_density, rgb)
    has = raw_density is not None
    L.call("psdf_nerf_frame_render", *rs._ri(), L.ptr(raw_density), L.ptr(rs.samples_dt if has else None),
           L.ptr(rs.samples_z if has and depth_img is not None else None), L.ptr(rgb), L.c_i(int(height)), L.c_i(int(width)),
           L.c_l(int(pixel_first)), L.ptr(rgb_img), L.ptr(weights_sum_img), L.ptr(depth_img), L.ptr(transmittance), L.stream())


@dataclasses.dataclass
class NerfRenderedFrame:
    """float32 planes on the device: what run_net_in_chunks returns (train_nerf.py:124-128), plus the expected depth"""
    rgb: torch.Tensor                       # [3, H, W] foreground + transmittance * background (foreground alone with a mask)
    rgb_bg: Optional[torch.Tensor]          # [3, H, W] transmittance * background; None in with_mask mode
    weights_sum: torch.Tensor               # [1, H, W]
    depth: Optional[torch.Tensor]           # [1, H, W] sum w z over the foreground samples; None unless asked for


class NerfFrameRenderer:
    def __init__(self, trainer):
        """trainer: a nerf_train.NerfTrainer, or anything with `net`, `net_bg` (None under with_mask), `grid`, `sphere`, `hp`
        and `with_mask`; its `iter`, where it has one, is the iteration `render` takes the coarse-to-fine windows of"""
        self.trainer = trainer

    @staticmethod
    def from_checkpoint(folder, device, hp=None, with_mask=False):
        """two NerfNets and the hp.grid_dim^3 occupancy grid, loaded from the file set of NerfTrainer.save_checkpoint (the
        reference's nerf_hash_model.pt / nerf_hash_model_bg.pt and the two grid tensors).  The files do not hold the
        iteration: `render` opens every lattice level unless it is given one"""
        from . import checkpoint
        hp = hp or HyperParams()
        dev = torch.device(device)
        L.require_cuda(torch.empty(0, device=dev))
        net = NerfNet(3, hp.foreground_nr_iters_for_c2f).to(dev)
        net_bg = None if with_mask else NerfNet(4, hp.background_nr_iters_for_c2f).to(dev)
        grid = OccupancyGrid(hp.grid_dim, 1.0, [0, 0, 0], device=dev)
        sd = torch.load(os.path.join(folder, FILES["fg"]), map_location=dev)
        net.load_state_dict(checkpoint.from_reference_keys("bg", sd))
        checkpoint.load(folder, bg=net_bg, grid=grid, map_location=dev)
        return NerfFrameRenderer(SimpleNamespace(net=net, net_bg=net_bg, grid=grid, sphere=Sphere(0.5, [0, 0, 0]), hp=hp,
                                                 with_mask=bool(with_mask), iter=IT_WINDOW_OPEN))

    def _chunk(self, frame, first, count, it, out, transmittance):
        """one chunk, start to finish; nothing it allocates outlives it"""
        t = self.trainer
        H, W = frame.height, frame.width
        o, d = frame_rays(frame, first, count)
        _, fg, bg = NerfTrainer.sample(t, o, d, False)
        raw = rgb = None
        if fg.samples_pos.shape[0]:
            B = NerfTrainer._branch_forward(t.net, fg.samples_pos, fg.samples_dirs, it, train=False)
            raw, rgb = B.raw_den, B.rgb
        frame_render_nerf_raw(fg, raw, rgb, H, W, first, out.rgb, out.weights_sum, transmittance, out.depth)
        if bg is not None:
            B = NerfTrainer._branch_forward(t.net_bg, bg.samples_pos_4d, bg.samples_dirs, it, train=False)
            frame_composite_nerf_raw(bg, B.raw_den, B.rgb, transmittance, H, W, first, out.rgb, out.rgb_bg)

    @torch.no_grad()
    def render(self, frame, it=None, pool_samples=OccupancyGrid.POOL, depth=False):
        """-> NerfRenderedFrame.  Evaluation mode (no jitter), no colour calibration.  it: the iteration whose coarse-to-fine
        windows both nets use; None: the trainer's current one (what train_nerf.py:259 passes), every level open for models
        that carry none.  pool_samples: the sample pool of the occupancy march, which bounds the rays of a chunk (FramePlan).
        depth: also the expected depth sum w z of the foreground."""
        t = self.trainer
        hp = t.hp
        dev = frame_device(frame, t.net)
        plan = FramePlan(frame.height, frame.width, hp.max_nr_samples_per_ray, pool_samples)
        if it is None:
            it = getattr(t, "iter", IT_WINDOW_OPEN)
        planes = functools.partial(new_planes, frame, dev=dev)
        out = NerfRenderedFrame(rgb=planes(3), rgb_bg=None if t.with_mask else planes(3), weights_sum=planes(1),
                                depth=planes(1) if depth else None)
        transmittance = torch.empty(plan.rays_per_chunk, dtype=torch.float32, device=dev)
        with sample_pool(t.grid, pool_samples):
            for first, count in plan.chunks():
                self._chunk(frame, first, count, it, out, transmittance)
        return out

    def render_views(self, frames, **kwargs):
        """-> [N, 3, H, W] float32: the rgb of every frame (all of one size), ready for image_eval.evaluate_views"""
        return stack_views(self.render, frames, **kwargs)
