"""Coloured meshes: the colour network asked about the vertices of an extracted surface (csrc/mesh_color.hip,
csrc/mesh_color_plan.h).

`MeshExtractor.extract` returns positions, faces and normals; the colour network that was trained beside the SDF knows the
surface's colour and is never asked.  `MeshColorizer(sdf_net, rgb_net).colors(points)` asks it, per vertex:

    SDF net (lattice + MLP) -> sdf, geometry features;  its input gradient -> the normal
    colour net: [colour lattice | SH5(view direction) | unit normal | geometry features] -> Lipschitz MLP -> sigmoid -> 8 bits

That is `ManualTrainer._fg_forward`'s chain over the raw feature-major kernels, outside autograd, with two launches of its own:
`psdf_mesh_color_inputs` writes the SH, normal and geometry rows of the colour network's input straight into the buffer the
colour encoding was written into (no SH launch, no normalize launch, no torch.cat, no transpose), `psdf_mesh_color_finish`
turns the head's output into float and 8-bit colours in place in the result.  A vertex has no ray, so its view direction is made
up: `view="normal"` looks at every vertex head-on from outside (d = -normal: a view-independent "albedo-like" colour),
a `frame.Frame` or a 3-vector looks from that camera centre (d = normalize(p - eye), no visibility test).

Evaluation mode as `FrameRenderer.render`: the lattice window fully open unless `it` is given, no colour calibration
(create_my_images.py passes None).  Vertices are streamed in the chunks of `ColorPlan`; the buffers this module owns are allocated
once per call (what `net_eval.sdf_gradient` allocates inside comes from the caching allocator per chunk); nothing waits for the device.  The default evaluates the colour MLP with fp32 MFMAs (`mlp_forward_raw`): the wide fp16 kernel's refusal is
sticky process state (a value beyond the fp16 range met earlier), and an export should not depend on what ran before it;
`fast=True` tries that kernel first.

Out of scope: texture atlases, blending over several cameras with visibility, projecting the vertices onto the zero set before
colouring, and meshes of a NeRF's density.
"""
from types import SimpleNamespace
from typing import NamedTuple

import torch

from . import _lib as L
from .frame import IT_WINDOW_OPEN as _IT_WINDOW_OPEN
from .mlp import lipshitz_normalize_all_raw, mlp_forward_raw, mlp_forward_wide_f16_raw, pack_params
from .net_eval import enc_forward, net_params, sdf_gradient

_PLAN_FIELDS = 7            # PSDF_MESH_COLOR_PLAN_FIELDS of include/psdf.h
MODE_NORMAL, MODE_CAMERA = 0, 1     # csrc/mesh_color_plan.h


class VertexColors(NamedTuple):
    rgb: torch.Tensor       # [N, 3] float32 in [0, 1]
    rgb_u8: torch.Tensor    # [N, 3] uint8: image_eval.to_u8 of rgb
    normals: torch.Tensor   # [N, 3] float32: the outward unit normals the colour network was given


class ColorPlan:
    """rows of the colour network's input and the chunks of a call, from the library's host-only entry (csrc/mesh_color_plan.h
    decides them)"""

    def __init__(self, rgb_enc_width, g, mlp_in, n, chunk):
        out = (L.c_l * _PLAN_FIELDS)()
        status = L.lib().psdf_mesh_color_plan(L.c_i(int(rgb_enc_width)), L.c_i(int(g)), L.c_i(int(mlp_in)), L.c_l(int(n)),
                                              L.c_l(int(chunk)), out)
        if status == -1:
            raise ValueError("no colour plan: a colour encoding of %d channels and %d geometry features do not make the %d inputs "
                             "of the colour MLP, or n = %d < 0, or chunk = %d < 1" % (rgb_enc_width, g, mlp_in, n, chunk))
        L.check(status, "psdf_mesh_color_plan")
        self.c_enc, self.c_sh, self.c_normal, self.c_geom, self.C, self.nr_chunks, self.last_chunk = (int(v) for v in out)


def _view(view, dev):
    """-> (mode, eye [3] on dev | None)"""
    if isinstance(view, str):
        if view != "normal":
            raise ValueError("view must be 'normal', a render.Frame or a 3-vector, got %r" % (view,))
        return MODE_NORMAL, None
    if hasattr(view, "tf_world_cam"):
        eye = view.tf_world_cam[:3, 3]
    else:
        try:
            eye = torch.as_tensor(view)
        except (TypeError, ValueError, RuntimeError):
            raise ValueError("view must be 'normal', a render.Frame or a 3-vector, got %r" % (view,)) from None
    if eye.numel() != 3 or eye.is_complex() or eye.dtype == torch.bool:
        raise ValueError("view must be 'normal', a render.Frame or a 3-vector, got a tensor of shape %s" % (tuple(eye.shape),))
    return MODE_CAMERA, eye.detach().reshape(3).to(device=dev, dtype=torch.float32).contiguous()


class MeshColorizer:
    """sdf_net, rgb_net: a train_step.SdfNet and RgbNet on one device; it: the annealing iteration whose lattice window to use
    (None: fully open, as FrameRenderer.render)"""

    def __init__(self, sdf_net, rgb_net, it=None):
        self.sdf, self.rgb = sdf_net, rgb_net
        self.it = _IT_WINDOW_OPEN if it is None else it
        self.last_used_wide_f16 = None      # of the last `colors(fast=True)`: whether the wide fp16 kernel took every chunk

    @torch.no_grad()
    def colors(self, points, view="normal", chunk=1 << 18, fast=False):
        """points [N, 3] -> VertexColors.  view: "normal", a render.Frame or a 3-vector (the eye); chunk: vertices per pass;
        fast: the colour MLP on the wide fp16 kernel where the library takes it"""
        sdf, rgbn = self.sdf, self.rgb
        dev = sdf.encoding.lattice_values.device
        L.require_cuda(points, sdf.encoding.lattice_values, rgbn.encoding.lattice_values)
        if points.device != dev or rgbn.encoding.lattice_values.device != dev:
            raise L.PsdfError("the points live on %s, the SDF net on %s, the colour net on %s"
                              % (points.device, dev, rgbn.encoding.lattice_values.device))
        if points.ndim != 2 or points.shape[1] != 3:
            raise ValueError("points must be [N, 3], got %s" % (tuple(points.shape),))
        chunk = int(chunk)
        if chunk < 1:
            raise ValueError("chunk must be at least 1, got %d" % chunk)
        mode, eye = _view(view, dev)
        pts = points.detach().to(torch.float32).contiguous()
        N = pts.shape[0]
        out = VertexColors(torch.empty((N, 3), dtype=torch.float32, device=dev), torch.empty((N, 3), dtype=torch.uint8, device=dev),
                           torch.empty((N, 3), dtype=torch.float32, device=dev))
        if N == 0:
            return out
        dims, _, ws, bs = net_params(sdf.mlp_sdf)
        g, m = dims[-1] - 1, rgbn.mlp
        c_feat = sdf.encoding.cfg.channels
        chunk = min(chunk, N)                   # (one chunk takes them all: a larger one is not a larger launch)
        plan = ColorPlan(rgbn.encoding.cfg.channels, g, m.dims[0], N, chunk)
        # once per call: the SDF net's packed weight image (as ManualTrainer._main_forward builds st.net), the colour net's
        # Lipschitz-normalised weights and their packed image
        net = SimpleNamespace(dims=dims, ws=ws, bs=bs, win=sdf.window(self.it).detach().to(torch.float32).contiguous(),
                              packed=pack_params(dims, ws, bs))
        rgb_win = rgbn._win.detach().contiguous()
        wn = lipshitz_normalize_all_raw(m.weights_per_layer, m.lipshitz_bound_per_layer)
        bsr = [b.detach() for b in m.biases_per_layer]
        packed_rgb = None if fast else pack_params(m.dims, wn, bsr)
        wide = bool(fast)
        new = lambda rows: torch.empty(rows * chunk, dtype=torch.float32, device=dev)   # noqa: E731
        feat_flat, y_flat, x_flat, raw_flat = new(c_feat), new(1 + g), new(plan.C), new(3)
        grad_buf = torch.empty((chunk, 3), dtype=torch.float32, device=dev)
        for i in range(plan.nr_chunks):
            a, n = i * chunk, (chunk if i < plan.nr_chunks - 1 else plan.last_chunk)
            p = pts[a:a + n]
            fm = lambda flat, rows: flat[:rows * n].view(rows, n)                        # noqa: E731
            x_fm, raw_fm = fm(x_flat, plan.C), fm(raw_flat, 3)
            feat = enc_forward(sdf.encoding, p, net.win, train=False, out=fm(feat_flat, c_feat))
            y = mlp_forward_raw(dims, feat, net.packed, out=fm(y_flat, 1 + g))
            grad, _, _ = sdf_gradient(sdf.encoding, feat, p, net, zeroed=grad_buf[:n].zero_())
            enc_forward(rgbn.encoding, p, rgb_win, train=False, out=x_fm[:plan.c_enc])
            L.call("psdf_mesh_color_inputs", L.c_l(n), L.ptr(p), L.ptr(grad), L.ptr(y), L.c_i(g), L.c_i(mode), L.ptr(eye), L.ptr(x_fm),
                   L.c_i(plan.C), L.c_i(plan.c_enc), None, L.ptr(out.normals[a:a + n]), L.stream())
            if wide and mlp_forward_wide_f16_raw(m.dims, x_fm, wn, bsr, out=raw_fm) is None:
                wide = False                    # the library declined: fp32 MFMAs from here on
            if not wide:
                if packed_rgb is None:
                    packed_rgb = pack_params(m.dims, wn, bsr)
                mlp_forward_raw(m.dims, x_fm, packed_rgb, out=raw_fm)
            L.call("psdf_mesh_color_finish", L.c_l(n), L.ptr(raw_fm), L.ptr(out.rgb[a:a + n]), L.ptr(out.rgb_u8[a:a + n]), L.stream())
        self.last_used_wide_f16 = wide if fast else None
        return out

    def colorize(self, mesh, **kw):
        """sets mesh.C [V, 3] uint8, the colours of its vertices, and returns the mesh; kw: `colors`'"""
        mesh.C = self.colors(mesh.V, **kw).rgb_u8
        return mesh
