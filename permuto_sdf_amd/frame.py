"""The camera and the planes of a rendered view: what every writer of image planes needs before its first launch (render.py,
nerf_view.py, box_trace.py, sdf_slice.py, mesh_color.py; csrc/frame_rays.hip, csrc/frame_plan.h).

  * `Frame(K, tf_world_cam, height, width)`   a pinhole camera; `Frame.from_reel(reel, i)` takes image i of an image reel;
  * `frame_rays(frame, first, count)`         the rays of a range of pixels, bit-for-bit the rays training draws for them;
  * `FramePlan(height, width, cap, pool)`     the chunks of a frame: the largest multiple of 64 rays whose samples fit the pool;
  * `IT_WINDOW_OPEN`, `open_window(net, it)`  the lattice window of an evaluation view: every level open unless `it` is given;
  * `frame_device(frame, net)`                the one device of a frame and of the net a view is rendered from;
  * `new_planes(frame, channels, dev)`        an image the chunks of a frame fill;
  * `sample_pool(grid, pool_samples)`         the occupancy march's pool set to the one a plan was made for, and put back;
  * `stack_views(render, frames)`             -> [N, 3, H, W], what `image_eval.evaluate_views` takes.

A leaf module: it imports nothing of the package but the library's loader, so the writers import it at the top of their files.
CPU tensors raise PsdfError: there is no CPU path.
"""
import contextlib

import torch

from . import _lib as L

_PLAN_FIELDS = 3            # PSDF_FRAME_PLAN_FIELDS of include/psdf.h
IT_WINDOW_OPEN = 9999999    # create_my_images.py:81: far past every coarse-to-fine schedule, every lattice level fully open


def open_window(net, it=None):
    """the lattice window of `net` at the annealing iteration `it`; None: fully open"""
    return net.window(IT_WINDOW_OPEN if it is None else it)


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


def frame_device(frame, net):
    """-> the device of the lattice of `net` (anything with `encoding.lattice_values`: a tensor's device carries its index, a
    module's `dev` may be a bare "cuda"), after making sure `frame` lives there too; the frame is looked at first.  The kernels
    take raw pointers: no one else would notice a frame on another device than the models."""
    L.require_cuda(frame.K, frame.tf_world_cam)
    lattice = net.encoding.lattice_values
    L.require_cuda(lattice)
    dev = lattice.device
    if frame.K.device != dev or frame.tf_world_cam.device != dev:
        raise L.PsdfError("the frame lives on %s, the models on %s" % (frame.K.device, dev))
    return dev


def new_planes(frame, channels, dev):
    """[channels, H, W] float32, uninitialised: every pixel belongs to one chunk, which writes it"""
    return torch.empty((channels, frame.height, frame.width), dtype=torch.float32, device=dev)


@contextlib.contextmanager
def sample_pool(grid, pool_samples):
    """`grid.max_nr_samples` is the pool a FramePlan was made for while the frame's chunks run, and what it was afterwards"""
    before = grid.max_nr_samples
    grid.max_nr_samples = int(pool_samples)
    try:
        yield
    finally:
        grid.max_nr_samples = before


def stack_views(render, frames, **kwargs):
    """-> [N, 3, H, W] float32: the rgb of `render(frame, **kwargs)` for every frame (all of one size), ready for
    image_eval.evaluate_views"""
    frames = list(frames)
    if not frames:
        raise ValueError("render_views needs at least one frame")
    if len({(f.height, f.width) for f in frames}) != 1:
        raise ValueError("render_views takes frames of one size")
    return torch.stack([render(f, **kwargs).rgb for f in frames])
