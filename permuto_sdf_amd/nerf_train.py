"""NeRF training on the device: the reference's fourth trainer, permuto_sdf_py/train_nerf.py (csrc/nerf_render.hip).

The reference trains a plain NeRF -- NerfHash(3) for the foreground inside the bounding primitive, NerfHash(4) on inverse-depth
samples for the background, a 64^3 occupancy grid refreshed from the foreground's density -- with a masked squared colour error
and, under --with_mask, a clipped binary cross entropy that holds the per-ray weight sum to the mask (train_nerf.py:61-89,
178-218).  Every operator it calls was in the tree; what was missing is a renderer that returns all three per-ray results of
the FOREGROUND (radiance, weight sum, background transmittance) with their gradients, the loss tail, and a trainer.  Here:

  * `nerf_render`        softplus -> opacity -> transmittance -> weights -> (radiance, weights_sum, bg_transmittance) of a packed
                         container, one launch per direction, as one autograd Function over `nerf_render_raw` /
                         `nerf_render_backward_raw`; all three outputs are differentiable, an output nobody differentiates
                         sends no gradient into the kernel (a NULL pointer);
  * `nerf_loss`          the loss tail as one autograd Function over `nerf_loss_raw` (value, two terms and both gradients in
                         one call, deterministic); `nerf_loss_torch` is the same formula in torch operators;
  * `nerf_head_join_raw` [gelu(features); SH^T], the glue between NerfHash's two nets, and its backward, one launch each;
  * `NerfNet`            NerfHash for 3 and 4 dimensions (models.py:425-550) with the layers, initialisation and parameter
                         names of train_step.BgNet, the reference's coarse-to-fine window and `get_only_density`;
  * `NerfTrainer`        the optimisation step, written by hand over the raw feature-major kernels (`hand_written=True`) or as
                         a torch-autograd graph over the operators the tree had before (`hand_written=False`: the unfused chain
                         nerf_alpha -> cumprod -> multiply -> integrate -> sum_over_each_ray and torch's loss; the yardstick
                         the hand-written step is held against, not a fallback).

  * `colorcal_sigmoid`   the per-image colour calibration of train_nerf.py:52,158-161 (`Colorcal`, models.py:678-729) with the
                         sigmoid behind it, csrc/colorcal.hip: one launch forward, one backward and one fold of the per-ray
                         sums into the two [I, 3] gradients, deterministic; `NerfTrainer(nr_images=...)` trains with it.

Left out: the viewer branches and the dataset loaders.  The bounding primitive is the tree's `Sphere` of radius
0.5, as in the reference (create_bb_for_dataset returns Sphere(0.5) for every dataset name, common_utils.py:508-528); the
occupancy grid spans [-0.5, 0.5]^3.  Views of a trained run as image planes: nerf_view.py (`NerfTrainer.renderer()`).
"""
import contextlib
import os
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from . import _lib as L
from . import parallel
from .bridge import OccupancyGrid, PermutoSDF, RaySampler, Sphere, VolumeRendering, _per_sample
from .encoding import Coarse2Fine
from .mlp import FusedMLP, _grad_views, mlp_backward_raw, mlp_forward_raw, mlp_forward_wide_f16_raw, pack_params
from .net_eval import enc_backward, enc_forward, net_params, one_row_head, scalar_only, set_grads
from .neus import (nerf_alpha, nerf_composite, nerf_composite_backward_raw, nerf_composite_forward_raw, sigmoid_rows_backward_raw,
                   sigmoid_rows_raw)
from .optim import FusedAdamW
from .train_step import BgNet, Colorcal, _Cumprod, _Integrate, _SumRay, _lattice, cat_fm

PLAN_FIELDS = 4                    # PSDF_NERF_RENDER_PLAN_FIELDS of include/psdf.h
FUSED_MAX_PER_RAY = 256
MASK_WEIGHT = 0.1                  # train_nerf.py:207
CLIP_LO, CLIP_HI = 1e-3, 1.0 - 1e-3
FILES = {"fg": "nerf_hash_model.pt", "bg": "nerf_hash_model_bg.pt"}        # models.py:556-563, train_nerf.py:231-232
COLORCAL_FILE = "colorcal_model.pt"                                        # models.py:753-760
COLORCAL_COLS = 6                  # a row of the per-ray sums: COLS of csrc/colorcal_plan.h


def plan(nr_rays, max_per_ray=64):
    """-> (workgroups of the loss kernel, bytes of its workspace, rays of one pass of its full grid, register chunks of the ray
    backward), from the library's host-only entry (csrc/nerf_render_plan.h decides them)"""
    out = (L.c_l * PLAN_FIELDS)()
    L.call("psdf_nerf_render_plan", L.c_l(int(nr_rays)), L.c_i(int(max_per_ray)), out)
    return tuple(int(v) for v in out)


def _c(t):
    return t.detach().to(torch.float32).contiguous()


# ------------------------------------------------------------------------------------------------------------- the render
@torch.no_grad()
def nerf_render_raw(rs, raw_density, rgb, want_pred=True, want_weights_sum=True, want_bg=True):
    """-> (pred [R, 3], weights_sum [R, 1], bg_transmittance [R, 1]), None for what is not wanted.  raw_density [M] (before the
    softplus), rgb [M, 3]; rs: the packed container (its ray ranges and samples_dt).  Empty and overflowed rays: 0, 0, 1."""
    L.require_cuda(raw_density, rgb)
    R, dev = rs.ray_start_end_idx.shape[0], raw_density.device
    f = dict(dtype=torch.float32, device=dev)
    pred = torch.empty((R, 3), **f) if want_pred else None
    ws = torch.empty((R, 1), **f) if want_weights_sum else None
    bg = torch.empty((R, 1), **f) if want_bg else None
    L.call("psdf_nerf_render_forward", *rs._ri(), L.ptr(raw_density), L.ptr(rs.samples_dt), L.ptr(rgb if want_pred else None),
           L.ptr(pred), L.ptr(ws), L.ptr(bg), L.stream())
    return pred, ws, bg


@torch.no_grad()
def nerf_render_backward_raw(rs, max_per_ray, g_pred, g_weights_sum, g_bg, raw_density, rgb, need_rgb=True):
    """-> (g_raw_density [M], g_rgb [M, 3] or None) for the upstream gradients g_pred [R, 3], g_weights_sum [R, 1], g_bg [R, 1]:
    each may be None (no gradient arrives there), one at least is given.  PsdfError(-2) when a ray may hold more than 256
    samples; a ray longer than max_per_ray comes back as NaN."""
    M, dev = raw_density.shape[0], raw_density.device
    g_raw = _per_sample(rs, (M,), dev)
    g_rgb = _per_sample(rs, (M, 3), dev) if need_rgb else None
    L.call("psdf_nerf_render_backward", *rs._ri(), L.c_i(int(max_per_ray)), L.ptr(g_pred), L.ptr(g_weights_sum), L.ptr(g_bg),
           L.ptr(raw_density), L.ptr(rs.samples_dt), L.ptr(rgb), L.c_i(int(VolumeRendering.reference_compat)), L.ptr(g_raw),
           L.ptr(g_rgb), L.stream())
    return g_raw, g_rgb


class _NerfRender(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rs, max_per_ray, raw_density, rgb):
        raw, c = _c(raw_density).reshape(-1), _c(rgb)
        pred, ws, bg = nerf_render_raw(rs, raw, c)
        ctx.save_for_backward(raw, c)
        ctx.rs, ctx.max_per_ray, ctx.raw_shape = rs, int(max_per_ray), raw_density.shape
        ctx.set_materialize_grads(False)        # an output nobody differentiates: None, not a tensor of zeros
        return pred, ws, bg

    @staticmethod
    def backward(ctx, g_pred, g_ws, g_bg):
        raw, c = ctx.saved_tensors
        if g_pred is None and g_ws is None and g_bg is None:
            return None, None, None, None
        g = [None if t is None else _c(t) for t in (g_pred, g_ws, g_bg)]
        g_raw, g_rgb = nerf_render_backward_raw(ctx.rs, ctx.max_per_ray, g[0], g[1], g[2], raw, c, need_rgb=ctx.needs_input_grad[3])
        return None, None, g_raw.view(ctx.raw_shape) if ctx.needs_input_grad[2] else None, g_rgb


def nerf_render(rs, max_per_ray, raw_density, rgb):
    """-> (pred [R, 3], weights_sum [R, 1], bg_transmittance [R, 1]) of a packed container whose rays hold at most `max_per_ray`
    (<= 256) samples: NerfHash's softplus, VolumeRenderingNerf.compute_weights + integrate (volume_rendering_modules.py:72-90) in
    one launch per direction; gradients flow from all three outputs to raw_density and rgb"""
    return _NerfRender.apply(rs, max_per_ray, raw_density, rgb)


# --------------------------------------------------------------------------------------------------------------- the loss
@torch.no_grad()
def nerf_loss_raw(pred, gt, hit=None, weights_sum=None, gt_mask=None, mask_weight=MASK_WEIGHT, loss=None, want_grad=True,
                  workspace=None, terms=None):
    """-> (loss [1], terms [2], g_pred [R, 3] or None, g_weights_sum [R, 1] or None).  terms: mean over 3 R of (gt - pred)^2
    hit[ray], and (weights_sum and gt_mask given) mean over R of BCE(clip(weights_sum, 1e-3, 1 - 1e-3), gt_mask), else 0.
    loss: an accumulator to ADD terms[0] + mask_weight terms[1] to (a fresh zero otherwise).  The same inputs give the same
    bits on every call.  workspace / terms: buffers to reuse (float64 [plan(R)[1] / 8], float32 [2])."""
    L.require_cuda(pred, gt)
    R = pred.shape[0]
    if pred.dim() != 2 or pred.shape[1] != 3 or gt.shape != pred.shape or (weights_sum is None) != (gt_mask is None):
        raise ValueError("nerf_loss: pred and gt [R, 3], weights_sum and gt_mask [R] (both or neither); got %s, %s, %s, %s"
                         % (tuple(pred.shape), tuple(gt.shape), None if weights_sum is None else tuple(weights_sum.shape),
                            None if gt_mask is None else tuple(gt_mask.shape)))
    mask = gt_mask is not None
    if (hit is not None and hit.numel() != R) or (mask and (weights_sum.numel() != R or gt_mask.numel() != R)):
        raise ValueError("nerf_loss: hit, weights_sum and gt_mask hold one entry per ray")
    dev = pred.device
    loss = L.zeroed_scalar(dev) if loss is None else loss
    if terms is None:
        terms = torch.empty(2, dtype=torch.float32, device=dev)
    g_pred = torch.empty((R, 3), dtype=torch.float32, device=dev) if want_grad else None
    g_ws = torch.empty((R, 1), dtype=torch.float32, device=dev) if (want_grad and mask) else None
    if R == 0:
        terms.zero_()
        return loss, terms, g_pred, g_ws
    if workspace is None:
        workspace = torch.empty(max(1, plan(R)[1] // 8), dtype=torch.float64, device=dev)
    h = None if hit is None else hit.reshape(-1).to(torch.uint8).contiguous()
    L.call("psdf_nerf_loss", L.c_l(R), L.ptr(_c(pred)), L.ptr(_c(gt)), L.ptr(h), L.ptr(_c(weights_sum).reshape(-1) if mask else None),
           L.ptr(_c(gt_mask).reshape(-1) if mask else None), L.c_f(float(mask_weight)), L.ptr(workspace), L.ptr(terms), L.ptr(loss),
           L.ptr(g_pred), L.ptr(g_ws), L.stream())
    return loss, terms, g_pred, g_ws


class _NerfLoss(torch.autograd.Function):
    """first-order only: the value is the kernel's, its gradients w.r.t. pred and weights_sum are returned as constants"""

    @staticmethod
    def forward(ctx, pred, weights_sum, gt, hit, gt_mask, mask_weight):
        loss, terms, g_pred, g_ws = nerf_loss_raw(pred.detach(), gt, hit, None if weights_sum is None else weights_sum.detach(), gt_mask,
                                                  mask_weight)
        ctx.mask = g_ws is not None
        ctx.save_for_backward(g_pred, g_ws.view(weights_sum.shape) if ctx.mask else g_pred)
        ctx.mark_non_differentiable(terms)
        return loss.view(()), terms

    @staticmethod
    def backward(ctx, go, _):
        g_pred, g_ws = ctx.saved_tensors
        return g_pred * go, (g_ws * go) if ctx.mask else None, None, None, None, None


def nerf_loss(pred, gt, hit=None, weights_sum=None, gt_mask=None, mask_weight=MASK_WEIGHT):
    """-> (loss, terms [2]): train_nerf.py:203-207, ((gt - pred)^2 * hit).mean() [+ mask_weight * binary_cross_entropy(
    weights_sum.clip(1e-3, 1 - 1e-3), gt_mask)]; differentiable once w.r.t. pred and weights_sum (one call forward, one multiply
    each backward)"""
    return _NerfLoss.apply(pred, weights_sum, gt, hit, gt_mask, float(mask_weight))


def nerf_loss_torch(pred, gt, hit=None, weights_sum=None, gt_mask=None, mask_weight=MASK_WEIGHT):
    """the same loss in plain torch -> (loss, terms [2]): any dtype, any device, differentiable by autograd"""
    sq = (gt - pred) ** 2
    if hit is not None:
        sq = sq * hit.reshape(-1, 1).to(pred.dtype)
    loss_rgb = sq.mean()
    if weights_sum is None:
        return loss_rgb, torch.stack([loss_rgb.detach(), loss_rgb.new_zeros(())])
    loss_mask = F.binary_cross_entropy(weights_sum.reshape(-1).clip(CLIP_LO, CLIP_HI), gt_mask.reshape(-1).to(pred.dtype))
    return loss_rgb + loss_mask * mask_weight, torch.stack([loss_rgb.detach(), loss_mask.detach()])


# ---------------------------------------------------------------------------------------------------------- the head join
@torch.no_grad()
def nerf_head_join_raw(fd, sh):
    """fd [65, M] (the density net's feature-major output), sh [M, 16] -> x2 [80, M] = [gelu(fd[1:65]); sh^T], one launch"""
    L.require_cuda(fd, sh)
    M = fd.shape[1]
    if fd.shape[0] != 65 or tuple(sh.shape) != (M, 16):
        raise ValueError("nerf_head_join: fd [65, M] and sh [M, 16], got %s and %s" % (tuple(fd.shape), tuple(sh.shape)))
    x2 = torch.empty((80, M), dtype=torch.float32, device=fd.device)
    L.call("psdf_nerf_head_join", L.c_l(M), L.ptr(fd), L.ptr(sh), L.ptr(x2), L.stream())
    return x2


@torch.no_grad()
def nerf_head_join_backward_raw(g_raw, dX2, fd):
    """g_raw [M], dX2 [>= 64, M] (contiguous: the colour head's input gradient), fd [65, M] -> g_fd [65, M] = [g_raw; dX2[:64] *
    gelu'(fd[1:65])], one launch"""
    L.require_cuda(g_raw, dX2, fd)
    M = fd.shape[1]
    if fd.shape[0] != 65 or g_raw.numel() != M or dX2.dim() != 2 or dX2.shape[0] < 64 or dX2.shape[1] != M:
        raise ValueError("nerf_head_join_backward: g_raw [M], dX2 [>= 64, M], fd [65, M], got %s, %s, %s"
                         % (tuple(g_raw.shape), tuple(dX2.shape), tuple(fd.shape)))
    g_fd = torch.empty((65, M), dtype=torch.float32, device=fd.device)
    L.call("psdf_nerf_head_join_backward", L.c_l(M), L.ptr(g_raw.reshape(-1)), L.ptr(dX2), L.ptr(fd), L.ptr(g_fd), L.stream())
    return g_fd


# ------------------------------------------------------------------------------------------------- the colour calibration
def _cc_args(img_idx, colorcal):
    """the table arguments of the three entries: img_idx [R] int32, I, the fixed image, weight_delta [I, 3], bias [I, 3]"""
    idx = img_idx if img_idx.dtype == torch.int32 and img_idx.is_contiguous() else img_idx.to(torch.int32).contiguous()
    return idx, int(colorcal.weight_delta.shape[0]), int(colorcal.idx_with_fixed_calib)


@torch.no_grad()
def colorcal_sigmoid_raw(rs, raw_fm, img_idx, colorcal):
    """raw_fm [3, M] (the colour head's feature-major output) -> rgb [M, 3] = sigmoid(raw * (1 + weight_delta[img]) + bias[img]),
    img the image of the sample's ray; rays of the fixed image and of an image outside the tables keep the identity (there, and
    everywhere with zero tables, the bits of `sigmoid_rows_raw`).  rs: the packed container; colorcal: train_step.Colorcal."""
    L.require_cuda(raw_fm, img_idx, colorcal.weight_delta)
    if raw_fm.dim() != 2 or raw_fm.shape[0] != 3 or img_idx.numel() != rs.ray_start_end_idx.shape[0]:
        raise ValueError("colorcal_sigmoid: raw_fm [3, M] and one image index per ray, got %s and %s" % (tuple(raw_fm.shape), tuple(img_idx.shape)))
    M = raw_fm.shape[1]
    idx, I, fixed = _cc_args(img_idx, colorcal)
    rgb = _per_sample(rs, (M, 3), raw_fm.device)
    L.call("psdf_colorcal_sigmoid_forward", *rs._ri(), L.c_l(M), L.ptr(_c(raw_fm)), L.ptr(idx), L.c_i(I), L.c_i(fixed),
           L.ptr(_c(colorcal.weight_delta)), L.ptr(_c(colorcal.bias)), L.ptr(rgb), L.stream())
    return rgb


@torch.no_grad()
def colorcal_sigmoid_backward_raw(rs, g_rgb, rgb, raw_fm, img_idx, colorcal):
    """-> (g_raw_fm [3, M] = g_rgb rgb (1 - rgb) w, g_ray [R, 6]: per ray the sums over its samples of g_pre raw (columns 0-2) and
    of g_pre = g_rgb rgb (1 - rgb) (columns 3-5); zeros for empty rays and rays that keep the identity).  The same inputs give the
    same bits on every call."""
    L.require_cuda(g_rgb, rgb, raw_fm)
    M, R = raw_fm.shape[1], rs.ray_start_end_idx.shape[0]
    idx, I, fixed = _cc_args(img_idx, colorcal)
    g_raw_fm = _per_sample(rs, (M, 3), raw_fm.device).view(3, M)       # (zero-filled where the container has unowned slots)
    g_ray = torch.empty((R, COLORCAL_COLS), dtype=torch.float32, device=raw_fm.device)
    L.call("psdf_colorcal_sigmoid_backward", *rs._ri(), L.c_l(M), L.ptr(_c(g_rgb)), L.ptr(rgb), L.ptr(_c(raw_fm)), L.ptr(idx), L.c_i(I),
           L.c_i(fixed), L.ptr(_c(colorcal.weight_delta)), L.ptr(_c(colorcal.bias)), L.ptr(g_raw_fm), L.ptr(g_ray), L.stream())
    return g_raw_fm, g_ray


@torch.no_grad()
def colorcal_fold_raw(img_idx, colorcal, g_ray_a, g_ray_b=None):
    """per-ray sums of one branch, or of two (b: the background's, added first) -> (g_weight_delta [I, 3], g_bias [I, 3]): for every
    image the sum over its rays in ascending ray order; the fixed image's row and the row of an image no ray drew are exactly 0"""
    L.require_cuda(g_ray_a, g_ray_b)
    idx, I, fixed = _cc_args(img_idx, colorcal)
    R = idx.shape[0]
    if tuple(g_ray_a.shape) != (R, COLORCAL_COLS) or (g_ray_b is not None and g_ray_b.shape != g_ray_a.shape):
        raise ValueError("colorcal_fold: per-ray sums [R, 6] for %d rays, got %s" % (R, tuple(g_ray_a.shape)))
    make = torch.zeros if R == 0 else torch.empty        # (the entry writes nothing for an empty batch)
    g_wd = make((I, 3), dtype=torch.float32, device=g_ray_a.device)
    g_b = make((I, 3), dtype=torch.float32, device=g_ray_a.device)
    L.call("psdf_colorcal_fold", L.c_i(R), L.ptr(idx), L.c_i(I), L.c_i(fixed), L.ptr(g_ray_a), L.ptr(g_ray_b), L.ptr(g_wd), L.ptr(g_b),
           L.stream())
    return g_wd, g_b


class _ColorcalSigmoid(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rs, img_idx, colorcal, raw_fm, weight_delta, bias):
        raw = _c(raw_fm)
        rgb = colorcal_sigmoid_raw(rs, raw, img_idx, colorcal)
        ctx.save_for_backward(raw, rgb)
        ctx.rs, ctx.img_idx, ctx.colorcal = rs, img_idx, colorcal
        return rgb

    @staticmethod
    def backward(ctx, g_rgb):
        raw, rgb = ctx.saved_tensors
        g_raw_fm, g_ray = colorcal_sigmoid_backward_raw(ctx.rs, g_rgb, rgb, raw, ctx.img_idx, ctx.colorcal)
        g_wd = g_b = None
        if ctx.needs_input_grad[4] or ctx.needs_input_grad[5]:
            g_wd, g_b = colorcal_fold_raw(ctx.img_idx, ctx.colorcal, g_ray)
        return None, None, None, g_raw_fm, g_wd, g_b


def colorcal_sigmoid(rs, raw_fm, img_idx, colorcal):
    """-> rgb [M, 3]: Colorcal.calib_RGB_samples_packed + sigmoid of the feature-major raw colours raw_fm [3, M] of the container
    `rs`, differentiable once w.r.t. raw_fm and the module's two parameters (one launch forward; backward one launch and the
    fold)"""
    return _ColorcalSigmoid.apply(rs, img_idx, colorcal, raw_fm, colorcal.weight_delta, colorcal.bias)


# ------------------------------------------------------------------------------------------------------------ the network
class NerfNet(BgNet):
    """NerfHash(in_channels = pos_dim), models.py:425-550: a 24-level lattice of capacity 2^18 over `pos_dim` dimensions with
    the position appended, the density + feature net C -> 64 x 3 -> 65 and the colour head [64 + 16] -> 64 -> 64 -> 3.  Layer
    shapes, initialisation and parameter names are train_step.BgNet's (`encoding`, `mlp_feat_and_density`, `mlp_rgb`), so
    checkpoint.py's key renaming for "bg" serves both; BgNet itself is built for 4 dimensions with an open window, this class
    adds the dimension and the reference's window map_range_val(it, 0, nr_iters_for_c2f, 0.3, 1.0)."""

    def __init__(self, pos_dim=3, nr_iters_for_c2f=1):
        torch.nn.Module.__init__(self)
        if pos_dim not in (3, 4):
            raise ValueError("NerfNet: pos_dim must be 3 or 4")
        self.pos_dim = int(pos_dim)
        self.encoding = _lattice(self.pos_dim, 1.0)
        self.mlp_feat_and_density = FusedMLP([self.encoding.output_dims(), 64, 64, 64, 65], reference_init=True,
                                             last_layer_linear_init=False)
        self.mlp_rgb = FusedMLP([64 + 16, 64, 64, 3], reference_init=True)
        self.register_buffer("_win", torch.ones(24), persistent=False)
        self.c2f = Coarse2Fine(24)
        self.nr_iters_for_c2f = nr_iters_for_c2f

    def window(self, it):
        return self.c2f.window_at(it, self.nr_iters_for_c2f, self.encoding.lattice_values.device)

    def forward(self, pos, dirs, it, colorcal=None, img_indices=None, ray_start_end_idx=None):
        """-> (colour [N, 3] after the sigmoid, RAW density [N, 1]: the softplus is the renderer's).  colorcal (train_step.Colorcal)
        with the rays' images and the container's ranges: the raw colours are calibrated first (models.py:520-523), in torch
        operators"""
        with torch.no_grad():
            sh = PermutoSDF.spherical_harmonics(dirs, 4)
        fd = self.mlp_feat_and_density(self.encoding(pos, self.window(it)))
        rgb = self.mlp_rgb(cat_fm([F.gelu(fd[:, 1:65]), sh]))
        if colorcal is not None:
            rgb = colorcal.calib_RGB_samples_packed(rgb, img_indices, ray_start_end_idx)
        return torch.sigmoid(rgb), fd[:, 0:1]

    @torch.no_grad()
    def get_only_density(self, points, it):
        """[N, 1]: softplus of the density alone (models.py:528-550), no graph: the lattice kernel and the density net with a
        1-row head"""
        head = one_row_head(self.mlp_feat_and_density)      # (packed behind the lattice kernel)
        raw = scalar_only(self.encoding, head, points.view(-1, self.pos_dim).contiguous(), self.window(it).contiguous())
        return F.softplus(raw.view(-1, 1))


class HyperParams:
    """train_nerf.py:45-55"""
    lr = 1e-3
    nr_samples_bg = 32
    min_dist_between_samples = 1e-4
    max_nr_samples_per_ray = 64
    nr_rays = 512
    foreground_nr_iters_for_c2f = 1
    background_nr_iters_for_c2f = 10000
    grid_dim = 64                        # OccupancyGrid(64, 1.0, [0, 0, 0]), :163
    grid_refresh_every = 8               # :188
    grid_refresh_points = 256 * 256      # :189
    grid_decay = 0.7                     # :191
    grid_occupancy_thresh = 1e-3
    mask_weight = MASK_WEIGHT            # :207


# ------------------------------------------------------------------------------------------------------------ the trainer
class NerfTrainer:
    """One optimisation step of train_nerf.py:178-218 per `step(reel)`: every 8th iteration the occupancy grid is refreshed from
    the foreground's density at 65 536 random voxel centres; 512 rays of the reel, their intersection with the bounding sphere,
    at most 64 foreground samples per ray in occupied voxels and 32 background samples; both nets, the render, the loss; AdamW
    (betas 0.9 / 0.99, eps 1e-15, no decay, constant rate).  with_mask: no background net, and the mask term on the weight sum.

    hand_written=True: per net  encode forward -> density net -> head join -> colour head -> sigmoid;  the new render for the
    foreground, psdf_nerf_composite_* with the foreground's radiance and transmittance for the background, the loss kernel
    (value and gradients), then every backward in reverse over the raw kernels into zero-filled gradient views and the
    lattices' touched-rows buffers -> AdamW.  No autograd; the loss stays on the device (the step's one host synchronisation
    is the sample count of the march, as in the reference).
    hand_written=False: the same step as an autograd graph over NerfNet.forward, the unfused compositing chain, nerf_composite
    and `nerf_loss_torch`, from the same batch: what the hand-written step is measured against.

    nr_images: train the reference's per-image colour calibration too (train_nerf.py:52,158-161,169-172): a
    train_step.Colorcal(nr_images, idx_with_fixed_calib) whose two parameters join the nets' AdamW group (no decay).  By hand the
    sigmoid of both branches becomes colorcal.hip's fused entry and the per-ray sums of both are folded once per step; as a graph
    the module goes through NerfNet.forward.  None: no calibration, the step as it was."""

    def __init__(self, device, with_mask=False, hand_written=True, hp=None, seed=0, colorcal=None, nr_images=None,
                 idx_with_fixed_calib=0):
        if colorcal is not None:
            raise NotImplementedError("NerfTrainer builds its own calibration module: pass nr_images= (and idx_with_fixed_calib=), "
                                      "not colorcal=")
        if nr_images is not None:
            if int(nr_images) < 1:
                raise ValueError("NerfTrainer: nr_images must be at least 1, got %r" % (nr_images,))
            if not 0 <= int(idx_with_fixed_calib) < int(nr_images):
                raise ValueError("NerfTrainer: idx_with_fixed_calib %r is no image of %d" % (idx_with_fixed_calib, int(nr_images)))
        self.hp = hp or HyperParams()
        self.dev = torch.device(device)
        L.require_cuda(torch.empty(0, device=self.dev))
        if self.hp.max_nr_samples_per_ray > FUSED_MAX_PER_RAY or self.hp.nr_samples_bg > FUSED_MAX_PER_RAY:
            raise ValueError("NerfTrainer: at most %d samples per ray" % FUSED_MAX_PER_RAY)
        self.with_mask, self.hand_written = bool(with_mask), bool(hand_written)
        torch.manual_seed(seed)
        self.net = NerfNet(3, self.hp.foreground_nr_iters_for_c2f).to(self.dev)
        self.net_bg = None if self.with_mask else NerfNet(4, self.hp.background_nr_iters_for_c2f).to(self.dev)
        self.nets = [n for n in (self.net, self.net_bg) if n is not None]
        self.sphere = Sphere(0.5, [0, 0, 0])
        self.grid = OccupancyGrid(self.hp.grid_dim, 1.0, [0, 0, 0], device=self.dev)
        self.colorcal = None if nr_images is None else Colorcal(int(nr_images), int(idx_with_fixed_calib)).to(self.dev)
        self.params = [p for n in self.nets for p in n.parameters() if p.requires_grad]
        if self.colorcal is not None:
            self.params += [self.colorcal.weight_delta, self.colorcal.bias]
        self.opt = FusedAdamW([{"params": self.params, "weight_decay": 0.0}], lr=self.hp.lr, betas=(0.9, 0.99), eps=1e-15,
                              weight_decay=0.0)
        self.touched = []
        for n in self.nets:
            tr = n.encoding.enable_touched_rows()
            self.opt.attach(n.encoding.lattice_values, tr)
            self.touched.append(tr)
        lattices = {id(n.encoding.lattice_values) for n in self.nets}
        self.dense = [p for p in self.params if id(p) not in lattices]
        # the dense parameter gradients of a step: views of ONE buffer, one fill per step (the kernels accumulate into them)
        self._mlps = [m for n in self.nets for m in (n.mlp_feat_and_density, n.mlp_rgb)]
        self._arena_sizes = [_grad_views(m.dims, dev="meta")[0].numel() for m in self._mlps]
        self._seed = seed + 1
        self.iter = 0
        self.capture_grads = None     # set to {} to have step() record the gradients it hands to the optimiser
        self.last_terms = None        # [2] on the device: the unweighted terms of the last step
        self.last = {}
        self._workspace = torch.empty(max(1, plan(max(self.hp.nr_rays, 1))[1] // 8), dtype=torch.float64, device=self.dev)

    # ---- the grid
    @torch.no_grad()
    def refresh_grid(self, it):
        """train_nerf.py:188-191, from the same random voxels for the same iteration and seed"""
        hp = self.hp
        parallel.seed_generators(977 + self._seed * 1000003 + it, self.dev)
        centres, idx = self.grid.compute_random_sample_of_grid_points(hp.grid_refresh_points, True)
        self.grid.update_with_density_random_sample(idx, self.net.get_only_density(centres, it), hp.grid_decay, hp.grid_occupancy_thresh)

    # ---- the batch
    @torch.no_grad()
    def draw(self, reel, it=None):
        """-> the batch of iteration `it` (default: the current one): rays of the reel with their colours, masks and hits of the
        bounding sphere, the foreground container (compacted) and the background container (None under with_mask)"""
        hp = self.hp
        it = self.iter if it is None else it
        parallel.seed_generators(parallel.step_seed(self._seed, 0, it, world=1), self.dev)
        o, d, gt, gt_mask, img_idx = PermutoSDF.random_rays_from_reel(reel, hp.nr_rays)
        hit, fg, bg = self.sample(o, d, True)
        return SimpleNamespace(gt=gt, gt_mask=gt_mask, hit=hit, fg=fg, bg=bg, R=o.shape[0], n_fg=fg.samples_pos.shape[0], img_idx=img_idx)

    @torch.no_grad()
    def sample(self, o, d, jitter):
        """create_samples (nerf_utils.py:502-526) -> (hits of the bounding sphere, the foreground container (compacted: one host
        wait), the background container (None under with_mask)); jitter: model.training.  Reads `sphere`, `grid`, `hp` and
        `with_mask` alone: nerf_view.NerfFrameRenderer calls it for models that come without a trainer."""
        hp = self.hp
        _, te, _, tx, hit = self.sphere.ray_intersection(o, d)
        fg = self.grid.compute_samples_in_occupied_regions(o, d, te, tx, hp.min_dist_between_samples, hp.max_nr_samples_per_ray,
                                                           jitter).compact_to_valid_samples()
        bg = None
        if not self.with_mask:
            bg = RaySampler.compute_samples_bg(o, d, tx, hp.nr_samples_bg, self.sphere.m_radius, self.sphere.m_center, jitter, False)
        return hit, fg, bg

    # ---- one net, by hand
    def _grad_arena(self):
        flat = torch.zeros(sum(self._arena_sizes), dtype=torch.float32, device=self.dev)
        views, at = [], 0
        for m, sz in zip(self._mlps, self._arena_sizes):
            views.append(_grad_views(m.dims, flat=flat[at:at + sz])[1:])
            at += sz
        return views

    @staticmethod
    def _branch_forward(net, pts, dirs, it, train=True, calib=None):
        """lattice -> density + feature net -> [gelu(features); SH4(dir)] (one launch) -> colour head -> sigmoid.  train=False
        (rendering): the lattice rows read are not marked for the optimiser.  calib = (container, img_idx, Colorcal): the
        calibrated sigmoid of colorcal.hip in the plain one's place"""
        win = net.window(it).contiguous()
        feat = enc_forward(net.encoding, pts, win, train)
        net1 = d1, _, w1, b1 = net_params(net.mlp_feat_and_density)
        fd = mlp_forward_wide_f16_raw(d1, feat, w1, b1)                      # [65, M] on the fp16 matrix pipe
        if fd is None:      # (the library declined: fp32 MFMAs)
            fd = mlp_forward_raw(d1, feat, pack_params(d1, w1, b1))
        x2 = nerf_head_join_raw(fd, PermutoSDF.spherical_harmonics(dirs, 4))  # [80, M]
        net2 = d2, _, w2, b2 = net_params(net.mlp_rgb)
        raw_fm = mlp_forward_raw(d2, x2, pack_params(d2, w2, b2))                 # [3, M]
        rgb = sigmoid_rows_raw(raw_fm) if calib is None else colorcal_sigmoid_raw(calib[0], raw_fm, calib[1], calib[2])   # [M, 3]
        return SimpleNamespace(net=net, pts=pts, win=win, feat=feat, fd=fd, x2=x2, net1=net1, net2=net2, rgb=rgb, raw_den=fd[0],
                               calib=calib, raw_fm=raw_fm if calib is not None else None)

    @staticmethod
    def _branch_backward(B, g_raw, g_rgb, into1, into2):
        """the net's gradients into the zero-filled views into1 (density + feature net) / into2 (colour head), the lattice's
        into its touched-rows buffer -> the calibration's per-ray sums [R, 6] (None without calibration)"""
        (d1, l1, w1, b1), (d2, l2, w2, b2) = B.net1, B.net2
        g_ray = None
        if B.calib is None:
            g_raw_fm = sigmoid_rows_backward_raw(g_rgb, B.rgb)
        else:
            g_raw_fm, g_ray = colorcal_sigmoid_backward_raw(B.calib[0], g_rgb, B.rgb, B.raw_fm, B.calib[1], B.calib[2])
        dX2, dW2, db2 = mlp_backward_raw(d2, B.x2, w2, b2, g_raw_fm, need_dx=True, into=into2)
        set_grads(l2, dW2, db2)
        g_fd = nerf_head_join_backward_raw(g_raw, dX2, B.fd)                  # [65, M]
        dX, dW1, db1 = mlp_backward_raw(d1, B.feat, w1, b1, g_fd, need_dx=True, into=into1)
        set_grads(l1, dW1, db1)
        enc_backward(B.net.encoding, B.pts, B.win, dX)
        return g_ray

    # ---- the two forms of a step
    @torch.no_grad()
    def _step_hand_written(self, b, it):
        hp, dev = self.hp, self.dev
        arena = self._grad_arena()
        for m, (dWs, dbs) in zip(self._mlps, arena):       # every dense parameter has a gradient, samples or not
            for l, dW, db in zip(m.layers, dWs, dbs):
                l.weight.grad, l.bias.grad = dW, db
        fg = ws = None
        cc = self.colorcal
        g_ray_fg = g_ray_bg = None
        if b.n_fg:
            fg = self._branch_forward(self.net, b.fg.samples_pos, b.fg.samples_dirs, it, calib=None if cc is None else (b.fg, b.img_idx, cc))
            pred_fg, ws, bgT = nerf_render_raw(b.fg, fg.raw_den, fg.rgb, want_weights_sum=self.with_mask, want_bg=not self.with_mask)
        else:
            pred_fg = torch.zeros(b.R, 3, device=dev)
            ws, bgT = (torch.zeros(b.R, 1, device=dev), None) if self.with_mask else (None, torch.ones(b.R, 1, device=dev))
        self.last_terms = torch.empty(2, dtype=torch.float32, device=dev)
        work = self._workspace if b.R <= hp.nr_rays else None
        if self.with_mask:
            loss, _, g_pred, g_ws = nerf_loss_raw(pred_fg, b.gt, b.hit, ws, b.gt_mask, hp.mask_weight, workspace=work, terms=self.last_terms)
            g_bgT = None
        else:
            bg = self._branch_forward(self.net_bg, b.bg.samples_pos_4d, b.bg.samples_dirs, it, calib=None if cc is None else (b.bg, b.img_idx, cc))
            # the background's render and pred = pred_fg + bgT * pred_bg: one launch per direction
            _, pred = nerf_composite_forward_raw(b.bg, bg.raw_den, bg.rgb, pred_fg, bgT)
            loss, _, g_pred, g_ws = nerf_loss_raw(pred, b.gt, b.hit, workspace=work, terms=self.last_terms)
            g_rawb, g_rgbb, g_bgT = nerf_composite_backward_raw(b.bg, hp.nr_samples_bg, g_pred, bg.raw_den, bg.rgb, bgT)
            g_ray_bg = self._branch_backward(bg, g_rawb, g_rgbb, arena[2], arena[3])
        if fg is not None:
            g_raw, g_rgb = nerf_render_backward_raw(b.fg, hp.max_nr_samples_per_ray, g_pred, g_ws, g_bgT, fg.raw_den, fg.rgb)
            g_ray_fg = self._branch_backward(fg, g_raw, g_rgb, arena[0], arena[1])
        if cc is not None:      # one fold per step, the background's sums first; one branch alone; no samples at all: zeros
            if g_ray_fg is None and g_ray_bg is None:
                cc.weight_delta.grad, cc.bias.grad = torch.zeros_like(cc.weight_delta), torch.zeros_like(cc.bias)
            elif g_ray_fg is None or g_ray_bg is None:
                cc.weight_delta.grad, cc.bias.grad = colorcal_fold_raw(b.img_idx, cc, g_ray_bg if g_ray_fg is None else g_ray_fg)
            else:
                cc.weight_delta.grad, cc.bias.grad = colorcal_fold_raw(b.img_idx, cc, g_ray_fg, g_ray_bg)
        return loss

    def _step_autograd(self, b, it):
        hp, dev = self.hp, self.dev
        ws = None
        cc = self.colorcal
        if b.n_fg:
            rgb, raw = self.net(b.fg.samples_pos, b.fg.samples_dirs, it, cc, b.img_idx, b.fg.ray_start_end_idx)
            alpha, one_minus = nerf_alpha(raw, b.fg.samples_dt)
            T, bgT = _Cumprod.apply(b.fg, one_minus)
            w = (alpha * T).view(-1, 1)
            ws, _ = _SumRay.apply(b.fg, w)
            pred = _Integrate.apply(b.fg, rgb, w)
        else:
            pred, ws, bgT = torch.zeros(b.R, 3, device=dev), torch.zeros(b.R, 1, device=dev), torch.ones(b.R, 1, device=dev)
        if self.with_mask:
            loss, terms = nerf_loss_torch(pred, b.gt, b.hit, ws, b.gt_mask, hp.mask_weight)
        else:
            rgb_b, raw_b = self.net_bg(b.bg.samples_pos_4d, b.bg.samples_dirs, it, cc, b.img_idx, b.bg.ray_start_end_idx)
            pred = nerf_composite(b.bg, hp.nr_samples_bg, raw_b, rgb_b, pred, bgT.view(-1, 1))
            loss, terms = nerf_loss_torch(pred, b.gt, b.hit)
        self.last_terms = terms
        with contextlib.ExitStack() as stack:       # the persistent buffers are open for THIS backward only
            for tr in self.touched:
                stack.enter_context(tr.accumulate())
            if loss.requires_grad:
                loss.backward()
        for p in self.dense:
            if p.grad is None:
                p.grad = torch.zeros_like(p)
        return loss.detach().view(1)

    def step(self, reel=None, batch=None):
        """one optimisation step -> the loss [1] on the device.  batch: a `draw()` to use instead of drawing one from `reel`"""
        it, hp = self.iter, self.hp
        if it % hp.grid_refresh_every == 0:
            self.refresh_grid(it)
        b = self.draw(reel, it) if batch is None else batch
        for p in self.params:
            p.grad = None
        loss = self._step_hand_written(b, it) if self.hand_written else self._step_autograd(b, it)
        for n, tr in zip(self.nets, self.touched):      # a lattice gradient that reached autograd joins its buffer
            p = n.encoding.lattice_values
            if p.grad is not None:
                tr.grad.add_(p.grad)
                p.grad = None
        if self.capture_grads is not None:      # tests: the gradients of this step as the optimiser is about to see them
            self.capture_grads = {"dense": [p.grad.detach().clone() for p in self.dense],
                                  "lattices": [tr.grad.clone() for tr in self.touched], "loss": loss.detach().clone()}
        self.opt.step()
        self.iter += 1
        self.last = {"nr_rays": b.R, "nr_fg_samples": b.n_fg}
        return loss

    def renderer(self):
        """-> nerf_view.NerfFrameRenderer over this trainer's nets, grid and sphere: views of a camera as image planes"""
        from .nerf_view import NerfFrameRenderer
        return NerfFrameRenderer(self)

    # ---- checkpoints: the reference's nerf_hash_model.pt / nerf_hash_model_bg.pt and the two grid tensors (train_nerf.py:230-238)
    def save_checkpoint(self, folder):
        # (one process, no collectives: no parameter all-gather is ever in flight here, unlike train_step.Trainer.save_checkpoint,
        # which waits for its own first; a data-parallel step added to this trainer has to bring that wait along)
        from . import checkpoint
        os.makedirs(folder, exist_ok=True)
        torch.save(checkpoint.to_reference_keys("bg", self.net.state_dict()), os.path.join(folder, FILES["fg"]))
        checkpoint.save(folder, bg=self.net_bg, grid=self.grid, colorcal=self.colorcal)      # colorcal_model.pt: weight_delta, bias

    def load_checkpoint(self, folder):
        from . import checkpoint
        sd = torch.load(os.path.join(folder, FILES["fg"]), map_location=self.dev)
        self.net.load_state_dict(checkpoint.from_reference_keys("bg", sd))
        # a checkpoint of a run without calibration loads into a calibrated trainer: the tables stay as they are (zero when new)
        cc = self.colorcal if os.path.exists(os.path.join(folder, COLORCAL_FILE)) else None
        checkpoint.load(folder, bg=self.net_bg, grid=self.grid, colorcal=cc, map_location=self.dev)
