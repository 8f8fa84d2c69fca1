"""Image evaluation on the device: the masked PSNR and SSIM of rendered views (csrc/image_eval.hip).

The reference scores its held-out views with permuto_sdf_py/experiments/evaluation/evaluate_psnr.py: piq.psnr and piq.ssim on
8-bit images, both multiplied by the mask, averaged per scene and over scenes.  Here the two scores are kernels that accumulate
in float64 over tensors that are already on the device, however they were rendered:

  * `psnr(pred, gt, mask)`            -10 log10(mse + 1e-8), mse over C H W of every image, masked pixels included;
  * `ssim(pred, gt, mask)`            piq's SSIM: pooling by round(min(H, W) / 256), 11-tap Gaussian window, valid positions only;
  * `to_u8(img)`                      the 8-bit conversion the reference's images went through: clamp(rint(255 img), 0, 255);
  * `evaluate_views(pred, gt, mask)`  the reference's scoring of a batch of views: 8-bit, then both scores per view;
  * `SceneScores`                     per-scene means, their mean over scenes and the reference's table lines.

Images are (N, C, H, W) or (C, H, W) tensors, float32 or uint8 (a uint8 value v stands for v / 255), each read in place through
its own strides: an NHWC buffer passed as `buf.permute(0, 3, 1, 2)` costs no copy, and `pred` and `gt` may differ in dtype and
layout.  The mask is (N, 1, H, W) or (1, 1, H, W): float32, bool, or uint8 read like an 8-bit image (255 keeps a pixel).  Results are float64 tensors on the
device; nothing here reads them back.  The views come from `render.FrameRenderer.render_views` or from anywhere else; reading or
writing image files stays the caller's business.
"""
import ctypes

import torch

from . import _lib as L

_PLAN_FIELDS = 14          # PSDF_IMAGE_EVAL_PLAN_FIELDS of include/psdf.h


class SsimPlan:
    """the launch plan of `ssim` for one shape, from the library's host-only entry (csrc/image_eval_plan.h decides it)"""

    def __init__(self, N, C, H, W, kernel_size=11, downsample=True):
        out = (L.c_l * _PLAN_FIELDS)()
        status = L.lib().psdf_image_eval_plan(L.c_l(N), L.c_i(C), L.c_i(H), L.c_i(W), L.c_i(kernel_size), L.c_i(int(bool(downsample))), out)
        if status == -1:
            raise ValueError("ssim: no plan for %d x %d images with a %d-tap window (the window must be odd, at most %d taps and "
                             "no larger than the pooled image)" % (H, W, kernel_size, max_kernel_size()))
        L.check(status, "psdf_image_eval_plan")
        (self.factor, self.pooled_h, self.pooled_w, self.map_h, self.map_w, self.tile_h, self.tile_w, self.tiles_y, self.tiles_x,
         self.workspace_bytes, self.sq_partials, self.sq_workspace_bytes, self.max_kernel, self.lds_bytes) = list(out)


def max_kernel_size():
    out = (L.c_l * _PLAN_FIELDS)()
    L.call("psdf_image_eval_plan", L.c_l(1), L.c_i(1), L.c_i(1), L.c_i(1), L.c_i(1), L.c_i(0), out)
    return int(out[12])


class _Image:
    """one argument triple of the C ABI: first element, element type, host strides.  Keeps its tensor alive."""

    def __init__(self, t):
        self.tensor = t
        self.ptr = ctypes.c_void_p(t.data_ptr())
        self.u8 = L.c_i(1 if t.dtype == torch.uint8 else 0)
        self.strides = (L.c_l * 4)(*t.stride())

    def args(self):
        return self.ptr, self.u8, self.strides


_NO_MASK = (None, L.c_i(0), None)


def _image(t, name):
    if not isinstance(t, torch.Tensor):
        raise ValueError("%s must be a tensor" % name)
    L.require_cuda(t)
    if t.ndim == 3:
        t = t.unsqueeze(0)
    if t.ndim != 4:
        raise ValueError("%s must be (N, C, H, W) or (C, H, W), got %s" % (name, tuple(t.shape)))
    t = t.detach()
    if t.dtype == torch.bool and name == "mask":
        t = t.to(torch.float32)
    elif t.dtype not in (torch.float32, torch.uint8):
        raise ValueError("%s must be float32 or uint8, got %s" % (name, t.dtype))
    return t


def _prepare(pred, gt, mask, data_range, check_range):
    for other, name in ((gt, "gt"), (mask, "mask")):
        if isinstance(pred, torch.Tensor) and isinstance(other, torch.Tensor) and other.device != pred.device:
            raise ValueError("pred and %s live on different devices (%s, %s)" % (name, pred.device, other.device))
    pred, gt = _image(pred, "pred"), _image(gt, "gt")
    if pred.shape != gt.shape:
        raise ValueError("pred %s and gt %s differ in shape" % (tuple(pred.shape), tuple(gt.shape)))
    N, C, H, W = pred.shape
    if N and (C < 1 or H < 1 or W < 1):
        raise ValueError("empty images: %s" % (tuple(pred.shape),))
    if max(C, H, W) > 2 ** 31 - 1:
        raise L.PsdfError("image extents beyond int32")
    data_range = float(data_range)
    if not (data_range > 0.0 and data_range != float("inf")):
        raise ValueError("data_range must be positive and finite")
    if mask is not None:
        mask = _image(mask, "mask")
        if mask.shape[1] != 1 or mask.shape[2:] != pred.shape[2:] or mask.shape[0] not in (1, N):
            raise ValueError("mask must be (N, 1, H, W) = (%d, 1, %d, %d), got %s" % (N, H, W, tuple(mask.shape)))
        mask = mask.expand(N, 1, H, W)
    if check_range and N:
        lo = torch.stack([pred.amin().double(), gt.amin().double()]).min()
        hi = torch.stack([pred.amax().double() / (255.0 if pred.dtype == torch.uint8 else 1.0),
                          gt.amax().double() / (255.0 if gt.dtype == torch.uint8 else 1.0)]).max()
        lo, hi = torch.stack([lo, hi]).tolist()         # the one host read, on request only
        if lo < 0.0 or hi > data_range or lo != lo or hi != hi:
            raise ValueError("image values span [%g, %g], outside [0, %g]" % (lo, hi, data_range))
    return pred, gt, mask, data_range


def _reduce(per_image, reduction):
    if reduction == "none":
        return per_image
    if reduction == "mean":
        return per_image.mean() if per_image.numel() else per_image.new_full((), float("nan"))
    raise ValueError("reduction must be 'mean' or 'none', got %r" % (reduction,))


def _check_reduction(reduction):
    if reduction not in ("mean", "none"):
        raise ValueError("reduction must be 'mean' or 'none', got %r" % (reduction,))


@torch.no_grad()
def sq_diff(pred, gt, mask=None, data_range=1.0, check_range=False):
    """-> [N] float64: the sum over (c, h, w) of (pred - gt)^2 of the masked, range-divided values"""
    pred, gt, mask, data_range = _prepare(pred, gt, mask, data_range, check_range)
    N, C, H, W = pred.shape
    out = torch.empty(N, dtype=torch.float64, device=pred.device)
    if N == 0:
        return out
    fn = L.lib().psdf_image_sq_diff_partials
    fn.restype = ctypes.c_int64
    workspace = torch.empty(N * int(fn(L.c_i(H), L.c_i(W))), dtype=torch.float64, device=pred.device)
    p, g = _Image(pred), _Image(gt)
    m = _Image(mask).args() if mask is not None else _NO_MASK
    L.call("psdf_image_sq_diff", *p.args(), *g.args(), *m, L.c_l(N), L.c_i(C), L.c_i(H), L.c_i(W), ctypes.c_double(data_range),
           L.ptr(workspace), L.ptr(out), L.stream())
    return out


@torch.no_grad()
def psnr(pred, gt, mask=None, data_range=1.0, reduction="mean", check_range=False):
    """-10 log10(mse + 1e-8) of every image, mse over all C H W values (masked pixels count as zero error, as in piq and the
    reference) -> float64 on the device: a scalar (reduction "mean") or [N] ("none")"""
    _check_reduction(reduction)
    total = sq_diff(pred, gt, mask, data_range, check_range)
    C, H, W = (pred.shape if pred.ndim == 4 else pred.unsqueeze(0).shape)[1:]
    return _reduce(-10.0 * torch.log10(total / float(C * H * W) + 1e-8), reduction)


@torch.no_grad()
def ssim(pred, gt, mask=None, data_range=1.0, kernel_size=11, kernel_sigma=1.5, k1=0.01, k2=0.03, downsample=True,
         reduction="mean", return_map=False, check_range=False):
    """piq's SSIM of every image -> float64 on the device: a scalar (reduction "mean") or [N] ("none"); with return_map:
    (score, map [N, C, h', w'] float64), h' = H // f - kernel_size + 1 with f = max(1, round(min(H, W) / 256)) (1 without
    `downsample`)"""
    _check_reduction(reduction)
    pred, gt, mask, data_range = _prepare(pred, gt, mask, data_range, check_range)
    N, C, H, W = pred.shape
    kernel_size, kernel_sigma = int(kernel_size), float(kernel_sigma)
    if not kernel_sigma > 0.0 or kernel_sigma == float("inf"):
        raise ValueError("kernel_sigma must be positive and finite")
    dev = pred.device
    out = torch.empty(N, dtype=torch.float64, device=dev)
    if N == 0:
        empty_map = torch.empty((0, C, 0, 0), dtype=torch.float64, device=dev)
        return (_reduce(out, reduction), empty_map) if return_map else _reduce(out, reduction)
    plan = SsimPlan(N, C, H, W, kernel_size, downsample)        # ValueError: no such window for this image
    workspace = torch.empty(plan.workspace_bytes // 8, dtype=torch.float64, device=dev)
    smap = torch.empty((N, C, plan.map_h, plan.map_w), dtype=torch.float64, device=dev) if return_map else None
    p, g = _Image(pred), _Image(gt)
    m = _Image(mask).args() if mask is not None else _NO_MASK
    L.call("psdf_image_ssim", *p.args(), *g.args(), *m, L.c_l(N), L.c_i(C), L.c_i(H), L.c_i(W), ctypes.c_double(data_range),
           L.c_i(kernel_size), ctypes.c_double(kernel_sigma), ctypes.c_double(float(k1)), ctypes.c_double(float(k2)),
           L.c_i(int(bool(downsample))), L.ptr(workspace), L.ptr(out), L.ptr(smap), L.stream())
    return (_reduce(out, reduction), smap) if return_map else _reduce(out, reduction)


@torch.no_grad()
def to_u8(img):
    """clamp(rint(img * 255), 0, 255) as uint8, ties to even: the 8-bit conversion the reference's views go through before they
    are scored (it writes them as 8-bit images and loads them again).  uint8 input is returned as it is."""
    if img.dtype == torch.uint8:
        return img
    if not img.is_floating_point():
        raise ValueError("to_u8 takes a floating-point or uint8 image, got %s" % img.dtype)
    return torch.round(img * 255).clamp(0, 255).to(torch.uint8)


@torch.no_grad()
def evaluate_views(pred, gt, mask=None):
    """the reference's scoring of a batch of views: floating-point images become 8-bit (`to_u8`), then -> (psnr [N], ssim [N]),
    float64 on the device, at the reference's settings (data_range 1, the default window, pooling on)"""
    pred, gt = to_u8(pred), to_u8(gt)
    return psnr(pred, gt, mask, reduction="none"), ssim(pred, gt, mask, reduction="none")


class SceneScores:
    """per-scene running means of PSNR and SSIM and their mean over scenes: the reference's EvalResults without its LPIPS column
    (always 0.0 there).  `update` takes Python numbers or tensors of any shape: every element is one view."""

    def __init__(self, name=""):
        self.name = name
        self._scenes = {}

    def update(self, scene, psnr, ssim):
        p = torch.as_tensor(psnr, dtype=torch.float64).reshape(-1).tolist()
        s = torch.as_tensor(ssim, dtype=torch.float64).reshape(-1).tolist()
        if len(p) != len(s):
            raise ValueError("%d PSNR values for %d SSIM values" % (len(p), len(s)))
        acc = self._scenes.setdefault(scene, [0.0, 0.0, 0])
        acc[0] += sum(p)
        acc[1] += sum(s)
        acc[2] += len(p)

    def scenes(self):
        return sorted(k for k, v in self._scenes.items() if v[2])

    def scene_mean(self, scene):
        """-> (psnr, ssim) averaged over the views of one scene"""
        p, s, n = self._scenes[scene]
        if not n:
            raise KeyError(scene)
        return p / n, s / n

    def mean(self):
        """-> (psnr, ssim): the mean over scenes of the per-scene means"""
        means = [self.scene_mean(k) for k in self.scenes()]
        if not means:
            return float("nan"), float("nan")
        return sum(m[0] for m in means) / len(means), sum(m[1] for m in means) / len(means)

    def table(self):
        """the lines evaluate_psnr.py prints for a method: scenes, `psnr: name a & b & `, `ssim: ...` and the two averages"""
        names = self.scenes()
        means = [self.scene_mean(k) for k in names]
        avg = self.mean()
        return "\n".join([
            "scenes_string  " + "".join("%s " % k for k in names),
            "psnr:  %s    %s" % (self.name, "".join("%2.2f & " % m[0] for m in means)),
            "ssim:  %s    %s" % (self.name, "".join("%2.3f & " % m[1] for m in means)),
            "psnr_avg  %s   %s" % (self.name, avg[0]),
            "ssim_avg  %s   %s" % (self.name, avg[1])])
