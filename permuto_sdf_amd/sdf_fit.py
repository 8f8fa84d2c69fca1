"""Fitting the SDF network directly to a mesh or an oriented point cloud, in three or four dimensions (csrc/sdf_fit.hip).

The reference gets a field without images in permuto_sdf_py/train_sdf_from_mesh.py (3-D) and train_4d_sdf.py (3-D plus time):
every iteration draws 3 000 points of the cloud with their normals and 30 000 (3 000 in 4-D) points of the bounding box,
evaluates the SDF and its gradient there, and minimises sdf_loss (permuto_sdf_py/utils/sdf_utils.py:16-57) / 30 000 with AdamW.
Here:

  * `OrientedCloud`     points [M, P] and normals [M, 3] on the device; from a mesh, from an extracted mesh, stacked in time;
  * `sdf_fit_batch_raw` the batch of a step, one launch (gather by index, affine map of uniform numbers);
  * `sdf_fit_loss`      the loss tail as one autograd Function over `sdf_fit_loss_raw` (value, four terms and gradient in one
                        call, deterministic); `sdf_fit_loss_torch` is the same formula in plain torch;
  * `SdfFitNet`         the reference's SDF(in_channels = 3 or 4, ...) (models.py:131-251) with the surface of
                        train_step.SdfNet, so the mesh extractor and the sphere tracer take a 3-D one as they are;
  * `SdfFitter`         the optimisation step, written by hand over the raw feature-major kernels (`hand_written=True`) or as
                        a torch-autograd graph over `SdfFitNet.sdf_and_gradient` and plain torch (`hand_written=False`: the
                        yardstick the hand-written step is held against, not a fallback).
"""
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib as L
from .encoding import Coarse2Fine, PermutoEncoding
from .mlp import FusedMLP, mlp_backward_raw, mlp_forward_raw, pack_params
from .net_eval import enc_forward, net_params, one_row_head, scalar_only, sdf_gradient, sdf_gradient_backward
from .optim import FusedAdamW

PLAN_FIELDS = 4                              # PSDF_SDF_FIT_PLAN_FIELDS of include/psdf.h
REFERENCE_WEIGHTS = (5e1, 1e2, 3e3, 1e2)     # sdf_utils.py:43: eikonal, normal, surface |sdf|, off-surface
REFERENCE_SCALE = 1.0 / 30000.0              # train_sdf_from_mesh.py:136


def plan(n_surf, n_off):
    """-> (workgroups of the loss kernel, bytes of its workspace, rows of one pass of its full grid, workgroups of the batch
    kernel), from the library's host-only entry (csrc/sdf_fit_plan.h decides them)"""
    out = (L.c_l * PLAN_FIELDS)()
    L.call("psdf_sdf_fit_plan", L.c_l(int(n_surf)), L.c_l(int(n_off)), out)
    return tuple(int(v) for v in out)


# ---------------------------------------------------------------------------------------------------------------- the cloud
class OrientedCloud:
    """points [M, P] (P = 3, or 4 with time as the last column) and normals [M, 3], float32, contiguous, on one device"""

    def __init__(self, points, normals):
        points, normals = torch.as_tensor(points), torch.as_tensor(normals)
        if points.dim() != 2 or points.shape[1] not in (3, 4) or normals.shape != (points.shape[0], 3):
            raise ValueError("OrientedCloud takes points [M, 3 or 4] and normals [M, 3], got %s and %s"
                             % (tuple(points.shape), tuple(normals.shape)))
        if points.device != normals.device:
            raise ValueError("points and normals live on different devices")
        self.points = points.detach().to(torch.float32).contiguous()
        self.normals = normals.detach().to(torch.float32).contiguous()

    pos_dim = property(lambda self: self.points.shape[1])
    device = property(lambda self: self.points.device)

    def __len__(self):
        return self.points.shape[0]

    def to(self, device):
        return OrientedCloud(self.points.to(device), self.normals.to(device))

    @classmethod
    def from_mesh(cls, V, F_):
        """the vertices of a triangle mesh with area-weighted vertex normals: every face adds its cross product
        (v1 - v0) x (v2 - v0), whose length is twice its area, to its three vertices; the sums are normalised.  The reference
        takes easypbr's `recalculate_normals` (train_sdf_from_mesh.py:88,93), whose weighting is not documented: the rule here
        is a restatement of what such a function commonly does and is NOT pinned to easypbr's.  Set-up, not the hot path."""
        V = torch.as_tensor(V).to(torch.float32)
        F_ = torch.as_tensor(F_).to(device=V.device, dtype=torch.int64)
        v0, v1, v2 = (V.index_select(0, F_[:, k]) for k in range(3))
        fn = torch.cross(v1 - v0, v2 - v0, dim=1)
        nv = torch.zeros_like(V)
        for k in range(3):
            nv.index_add_(0, F_[:, k], fn)
        return cls(V, F.normalize(nv, dim=1))

    @classmethod
    def from_extracted(cls, mesh):
        """from a mesh.ExtractedMesh: its vertices and its analytic outward normals (area-weighted ones where it has none)"""
        if mesh.NV is not None and len(mesh.NV) == len(mesh.V):
            return cls(mesh.V, mesh.NV)
        return cls.from_mesh(mesh.V, mesh.F)

    @classmethod
    def stack_in_time(cls, clouds):
        """the [M, 4] cloud of train_4d_sdf.py:122-141: cloud i of K gets the time i / (K - 1) as its fourth column"""
        clouds = list(clouds)
        if len(clouds) < 2 or any(c.pos_dim != 3 for c in clouds):
            raise ValueError("stack_in_time takes two or more 3-D clouds")
        pts = [torch.cat([c.points, torch.full((len(c), 1), i / (len(clouds) - 1), dtype=torch.float32, device=c.device)], 1)
               for i, c in enumerate(clouds)]
        return cls(torch.cat(pts, 0), torch.cat([c.normals for c in clouds], 0))


# ---------------------------------------------------------------------------------------------------------------- the batch
def _host_floats(v, P, name):
    v = [float(x) for x in (v.tolist() if hasattr(v, "tolist") else v)]
    if len(v) != P:
        raise ValueError("%s must have %d entries, got %d" % (name, P, len(v)))
    return (L.c_f * P)(*v)


@torch.no_grad()
def sdf_fit_batch_raw(cloud, indices, uniforms, lo, hi):
    """-> (points [n_surf + n_off, P], normals [n_surf, 3]): rows `indices` [n_surf] (int64) of the cloud, then
    lo + uniforms [n_off, P] * (hi - lo); lo, hi: P host numbers.  One launch.  An index is clamped to [0, M - 1]."""
    P, M = cloud.pos_dim, len(cloud)
    L.require_cuda(cloud.points, indices, uniforms)
    n_surf, n_off = int(indices.shape[0]), int(uniforms.shape[0])
    if indices.dtype != torch.int64 or uniforms.dtype != torch.float32 or (n_off and uniforms.shape[1] != P):
        raise ValueError("indices must be int64 [n_surf] and uniforms float32 [n_off, %d]" % P)
    if n_surf and M == 0:
        raise ValueError("surface rows asked of an empty cloud")
    dev = cloud.device
    points = torch.empty((n_surf + n_off, P), dtype=torch.float32, device=dev)
    normals = torch.empty((n_surf, 3), dtype=torch.float32, device=dev)
    L.call("psdf_sdf_fit_batch", L.c_i(P), L.c_l(M), L.c_l(n_surf), L.c_l(n_off), L.ptr(cloud.points), L.ptr(cloud.normals),
           L.ptr(indices.contiguous()), L.ptr(uniforms.contiguous()), _host_floats(lo, P, "lo"), _host_floats(hi, P, "hi"),
           L.ptr(points), L.ptr(normals), L.stream())
    return points, normals


def sdf_fit_batch_torch(cloud, indices, uniforms, lo, hi):
    """the same batch from torch operators (train_sdf_from_mesh.py:118-123): the same bits for indices inside the cloud"""
    dev = cloud.device
    lo_t, hi_t = (torch.tensor([float(x) for x in v], dtype=torch.float32, device=dev) for v in (lo, hi))
    surf = cloud.points.index_select(0, indices)
    off = lo_t + uniforms * (hi_t - lo_t)
    return torch.cat([surf, off], 0), cloud.normals.index_select(0, indices)


# ---------------------------------------------------------------------------------------------------------------- the loss
@torch.no_grad()
def sdf_fit_loss_raw(sdf, gradients, normals, n_surf, weights=REFERENCE_WEIGHTS, sharpness=1e2, eik_clamp=None,
                     scale=REFERENCE_SCALE, loss=None, want_grad=True, workspace=None, terms=None):
    """-> (loss [1], terms [4], grad_sdf [N] or None, grad_gradients [N, P] or None).  sdf [N] (or [N, 1]), gradients [N, P],
    normals [n_surf, 3]; the first n_surf rows lie on the surface.  loss: an accumulator to ADD scale * sum_k weights[k] terms[k]
    to (a fresh zero otherwise).  terms: the four unweighted means (eikonal, normal, surface |sdf|, off-surface).  The same
    inputs give the same bits on every call.  workspace / terms: buffers to reuse (float64 [plan(...)[1] / 8], float32 [4])."""
    L.require_cuda(sdf, gradients)
    N, P = gradients.shape
    n_surf = int(n_surf)
    n_off = N - n_surf
    if sdf.numel() != N or P not in (3, 4) or not 0 <= n_surf <= N or (n_surf and tuple(normals.shape) != (n_surf, 3)):
        raise ValueError("sdf_fit_loss: sdf [N], gradients [N, 3 or 4], normals [n_surf, 3] with 0 <= n_surf <= N; got %s, %s, %s, "
                         "n_surf = %d" % (tuple(sdf.shape), tuple(gradients.shape), None if normals is None else tuple(normals.shape), n_surf))
    dev = gradients.device
    loss = L.zeroed_scalar(dev) if loss is None else loss
    if terms is None:
        terms = torch.empty(4, dtype=torch.float32, device=dev)
    g_sdf = torch.empty(N, dtype=torch.float32, device=dev) if want_grad else None
    g_grad = torch.empty((N, P), dtype=torch.float32, device=dev) if want_grad else None
    if N == 0:
        terms.zero_()
        return loss, terms, g_sdf, g_grad
    if workspace is None:
        workspace = torch.empty(plan(n_surf, n_off)[1] // 8, dtype=torch.float64, device=dev)
    w = (L.c_f * 4)(*[float(x) for x in weights])
    L.call("psdf_sdf_fit_loss", L.c_i(P), L.c_l(n_surf), L.c_l(n_off), L.ptr(sdf.contiguous()), L.ptr(gradients.contiguous()),
           L.ptr(normals.contiguous()) if n_surf else None, w, L.c_f(float(sharpness)),
           L.c_f(float(eik_clamp) if eik_clamp is not None else 0.0), L.c_f(float(scale)), L.ptr(workspace), L.ptr(terms),
           L.ptr(loss), L.ptr(g_sdf), L.ptr(g_grad), L.stream())
    return loss, terms, g_sdf, g_grad


class _SdfFitLoss(torch.autograd.Function):
    """first-order only: the value is the kernel's, its gradients w.r.t. `sdf` and `gradients` are returned as constants"""

    @staticmethod
    def forward(ctx, sdf, gradients, normals, n_surf, weights, sharpness, eik_clamp, scale):
        loss, terms, g_sdf, g_grad = sdf_fit_loss_raw(sdf.detach().reshape(-1), gradients.detach(), normals.detach(), n_surf, weights,
                                                      sharpness, eik_clamp, scale)
        ctx.save_for_backward(g_sdf.view(sdf.shape), g_grad)
        ctx.mark_non_differentiable(terms)
        return loss.view(()), terms

    @staticmethod
    def backward(ctx, go, _):
        g_sdf, g_grad = ctx.saved_tensors
        return g_sdf * go, g_grad * go, None, None, None, None, None, None


def sdf_fit_loss(sdf, gradients, normals, n_surf, weights=REFERENCE_WEIGHTS, sharpness=1e2, eik_clamp=None, scale=REFERENCE_SCALE):
    """-> (loss, terms [4]): sdf_loss of permuto_sdf_py/utils/sdf_utils.py:16-57 times `scale` over a batch whose first n_surf
    rows lie on the surface; differentiable once w.r.t. sdf and gradients (one call forward, one multiply backward)"""
    return _SdfFitLoss.apply(sdf, gradients, normals, int(n_surf), tuple(weights), sharpness, eik_clamp, scale)


def sdf_fit_loss_torch(sdf, gradients, normals, n_surf, weights=REFERENCE_WEIGHTS, sharpness=1e2, eik_clamp=None,
                       scale=REFERENCE_SCALE):
    """the same loss in plain torch -> (loss, terms [4]): any dtype, any device, differentiable by autograd"""
    sdf = sdf.reshape(-1)
    g = gradients[:, :3]
    eik = (g.norm(dim=-1) - 1.0).abs()
    if eik_clamp is not None and eik_clamp > 0:
        x = sdf.abs().detach()
        eik = eik * torch.exp(-(x * x) / (2.0 * eik_clamp * eik_clamp))
    zero = sdf.new_zeros(())
    surf, off = sdf[:n_surf], sdf[n_surf:]
    terms = [eik.mean() if eik.numel() else zero,
             (1.0 - F.cosine_similarity(g[:n_surf], normals, dim=-1)).mean() if n_surf else zero,
             surf.abs().mean() if n_surf else zero,
             torch.exp(-sharpness * off.abs()).mean() if off.numel() else zero]
    loss = sum(t * float(w) for t, w in zip(terms, weights)) * scale
    return loss, torch.stack([t.detach() for t in terms])


# ---------------------------------------------------------------------------------------------------------------- the network
class SdfFitNet(torch.nn.Module):
    """models.py:131-251 for in_channels = pos_dim: a 24-level lattice of capacity 2^18 over `pos_dim` dimensions with the
    scaled position appended (concat_points_scaling 1e-3), Linear(C, 32)-GELU-(32, 32)-GELU-(32, 32)-GELU-(32, 1 + geom_feat_size),
    leaky_relu_init, sdf_shift 1e-2 on the last bias.  Attribute names and methods are train_step.SdfNet's (`encoding`, `mlp_sdf`,
    `window(it)`, `sdf_only`, `sdf_and_gradient`): `MeshExtractor.from_sdf_net`, `SphereTracer(net.encoding, net.mlp_sdf, ...)` and
    checkpoint.save(sdf=net) take a 3-D one as they are; a 4-D one is cut at a time with `time_slice` for the mesh extractor, and
    traced as it is, at a time, inside a box: `box_trace.BoxTracer(net.encoding, net.mlp_sdf, box)`, `render_box_traced`,
    `BoxPlayer` (a 3-D one too, with no occupancy grid)."""

    def __init__(self, pos_dim=3, geom_feat_size=0, nr_iters_for_c2f=5000):
        super().__init__()
        if pos_dim not in (3, 4):
            raise ValueError("SdfFitNet: pos_dim must be 3 or 4")
        self.pos_dim, self.geom_feat_size = int(pos_dim), int(geom_feat_size)
        self.encoding = PermutoEncoding(self.pos_dim, 2 ** 18, 24, 2, np.geomspace(1.0, 1e-4, 24), appply_random_shift_per_level=True,
                                        concat_points=True, concat_points_scaling=1e-3)
        self.mlp_sdf = FusedMLP([self.encoding.output_dims(), 32, 32, 32, 1 + self.geom_feat_size], reference_init=True)
        with torch.no_grad():  # models.py:163-165: `mlp_sdf[-1].bias += sdf_shift`, the whole bias vector
            self.mlp_sdf.layers[-1].bias += 1e-2
        self.c2f = Coarse2Fine(24)
        self.nr_iters_for_c2f = nr_iters_for_c2f

    def window(self, it):
        return self.c2f.window_at(it, self.nr_iters_for_c2f, self.encoding.lattice_values.device)

    def forward(self, points, it):
        """-> (sdf [N, 1], geometry features [N, geom_feat_size] or None)"""
        y = self.mlp_sdf(self.encoding(points, self.window(it)))
        if self.geom_feat_size == 0:
            return y, None
        return y[:, 0:1], y[:, 1:]

    @torch.no_grad()
    def sdf_only(self, points, it, key=None):
        """[N, 1]: the SDF alone (row 0 of the last layer), no graph: the lattice kernel and the MLP with a 1-row head"""
        head = one_row_head(self.mlp_sdf, pack=True)
        return scalar_only(self.encoding, head, points.contiguous(), self.window(it).contiguous()).view(-1, 1)

    def sdf_and_gradient(self, points, it):  # models.py:236-251
        """-> (sdf [N, 1], d sdf / d points [N, pos_dim] with its graph, geometry features or None)"""
        with torch.enable_grad():
            if not points.requires_grad:
                points = points.detach().requires_grad_(True)
            sdf, feat = self.forward(points, it)
            # autograd would compute the lattice and the MLP parameter gradients here and drop them
            with self.encoding.positions_gradient_only(), self.mlp_sdf.input_gradient_only():
                (grad,) = torch.autograd.grad(sdf, points, torch.ones_like(sdf), create_graph=True, retain_graph=True)
        return sdf, grad, feat

    def time_slice(self, t, it=None):
        """the 3-D field of a 4-D net at time t: a callable points [N, 3] -> sdf [N, 1], what `MeshExtractor(fn)` accepts.
        it: the training iteration whose coarse-to-fine window is used (default: fully open)"""
        if self.pos_dim != 4:
            raise ValueError("time_slice cuts a 4-D net")
        it = self.nr_iters_for_c2f if it is None else it
        t = float(t)

        def fn(points):
            p4 = torch.cat([points.to(torch.float32), points.new_full((points.shape[0], 1), t, dtype=torch.float32)], 1)
            return self.sdf_only(p4, it)
        return fn


# ---------------------------------------------------------------------------------------------------------------- the fitter
class SdfFitter:
    """One optimisation step of train_sdf_from_mesh.py:113-165 / train_4d_sdf.py:194-241 per `step()`: n_surf points of the
    cloud and n_off points of the box [box_lo, box_hi] (P numbers each; the reference's box is [-0.5, 0.5]^3, and [0, 1] in
    time), the SDF and its gradient there, sdf_loss * scale, AdamW (betas 0.9 / 0.99, eps 1e-15, no decay, constant rate).

    hand_written=True: batch kernel -> encode forward -> MLP forward -> n = d sdf / d p (MLP data backward of the unit output
    gradient, then the encoding's position backward) -> loss kernel (value and gradient) -> MLP backward of grad_sdf ->
    double backward (encoding gather, MLP double backward into the parameter buffer, ONE lattice scatter that also carries the
    plain backward) -> AdamW.  No autograd, no host synchronisation; the loss stays on the device.
    hand_written=False: the same step as an autograd graph over `SdfFitNet.sdf_and_gradient` and `sdf_fit_loss_torch`, from the
    same random numbers: what the hand-written step is measured against."""

    def __init__(self, cloud, box_lo=(-0.5, -0.5, -0.5), box_hi=(0.5, 0.5, 0.5), pos_dim=None, n_surf=3000, n_off=None, lr=1e-3,
                 nr_iters_for_c2f=None, geom_feat_size=0, weights=REFERENCE_WEIGHTS, sharpness=1e2, eik_clamp=None,
                 scale=REFERENCE_SCALE, hand_written=True, seed=0, device=None):
        pos_dim = cloud.pos_dim if pos_dim is None else int(pos_dim)
        if pos_dim != cloud.pos_dim:
            raise ValueError("a %d-D cloud for a %d-D fit" % (cloud.pos_dim, pos_dim))
        self.dev = torch.device(device) if device is not None else cloud.device
        L.require_cuda(torch.empty(0, device=self.dev))
        self.cloud = cloud.to(self.dev)
        self.pos_dim = pos_dim
        box_lo, box_hi = [float(x) for x in box_lo], [float(x) for x in box_hi]
        if pos_dim == 4 and len(box_lo) == 3:      # the reference draws the time of an off-surface point in [0, 1)
            box_lo, box_hi = box_lo + [0.0], box_hi + [1.0]
        if len(box_lo) != pos_dim or len(box_hi) != pos_dim:
            raise ValueError("box_lo and box_hi must have %d entries" % pos_dim)
        self.box_lo, self.box_hi = box_lo, box_hi
        self.n_surf = int(n_surf)
        self.n_off = int(n_off) if n_off is not None else (30000 if pos_dim == 3 else 3000)   # train_4d_sdf.py:205
        if nr_iters_for_c2f is None:
            nr_iters_for_c2f = 5000 if pos_dim == 3 else 3000      # train_sdf_from_mesh.py:104, train_4d_sdf.py:185
        self.weights, self.sharpness, self.eik_clamp, self.scale = tuple(float(w) for w in weights), float(sharpness), eik_clamp, float(scale)
        self.hand_written = bool(hand_written)
        torch.manual_seed(seed)
        self.net = SdfFitNet(pos_dim, geom_feat_size, nr_iters_for_c2f).to(self.dev)
        self.params = [p for p in self.net.parameters() if p.requires_grad]
        self.opt = FusedAdamW([{"params": self.params, "weight_decay": 0.0}], lr=lr, betas=(0.9, 0.99), eps=1e-15, weight_decay=0.0)
        self.touched = self.net.encoding.enable_touched_rows()
        self.opt.attach(self.net.encoding.lattice_values, self.touched)
        self.grad_buffer = self.net.mlp_sdf.enable_grad_buffer()
        self._rng = torch.Generator(device=self.dev)
        self._rng.manual_seed(seed + 1)
        self.iter = 0
        self.capture_grads = None     # set to {} to have step() record the gradients it hands to the optimiser
        self.last_terms = None        # [4] on the device: the unweighted terms of the last step
        p = plan(self.n_surf, self.n_off)
        self._workspace = torch.empty(max(1, p[1] // 8), dtype=torch.float64, device=self.dev)

    # ---- the batch
    def draw(self):
        """-> (indices [n_surf] int64, uniforms [n_off, P]) from this fitter's generator (torch's, as everywhere in the package)"""
        idx = torch.randint(len(self.cloud), (self.n_surf,), generator=self._rng, device=self.dev)
        u = torch.rand((self.n_off, self.pos_dim), generator=self._rng, device=self.dev)
        return idx, u

    # ---- the two forms of a step
    @torch.no_grad()
    def _step_hand_written(self, idx, u, it):
        net_m, enc, mlp = self.net, self.net.encoding, self.net.mlp_sdf
        points, normals = sdf_fit_batch_raw(self.cloud, idx, u, self.box_lo, self.box_hi)
        dims, _, ws, bs = net_params(mlp)
        net = SimpleNamespace(dims=dims, ws=ws, bs=bs, win=net_m.window(it).contiguous(), packed=pack_params(dims, ws, bs),
                              gb=self.grad_buffer)
        feat = enc_forward(enc, points, net.win)
        y = mlp_forward_raw(dims, feat, net.packed)                                        # [1 + geom, N]; row 0: the SDF
        n, dfeat, e0 = sdf_gradient(enc, feat, points, net, torch.zeros_like(points))
        self.last_terms = torch.empty(4, dtype=torch.float32, device=self.dev)
        loss, _, g_sdf, g_n = sdf_fit_loss_raw(y[0], n, normals, self.n_surf, self.weights, self.sharpness, self.eik_clamp, self.scale,
                                               workspace=self._workspace, terms=self.last_terms)
        # the loss reads nothing but the SDF row of the net's outputs
        g_y = g_sdf.view(1, -1) if dims[-1] == 1 else torch.cat([g_sdf.view(1, -1), g_sdf.new_zeros((dims[-1] - 1, g_sdf.shape[0]))], 0)
        dX1, _, _ = mlp_backward_raw(dims, feat, ws, bs, g_y, need_dx=True, into=(net.gb.dWs, net.gb.dbs))
        # the 1-output net has no double_backward_plus row: the plain backward's data gradient joins the double backward's
        # before the one lattice scatter (the two-launch form)
        sdf_gradient_backward(enc, mlp, g_n, feat, dfeat, e0, points, net, extra_dfeat=dX1)
        return loss

    def _step_autograd(self, idx, u, it):
        points, normals = sdf_fit_batch_torch(self.cloud, idx, u, self.box_lo, self.box_hi)
        sdf, grad, _ = self.net.sdf_and_gradient(points, it)
        loss, terms = sdf_fit_loss_torch(sdf, grad, normals, self.n_surf, self.weights, self.sharpness, self.eik_clamp, self.scale)
        self.last_terms = terms
        with self.touched.accumulate(), self.grad_buffer.accumulate():      # the persistent buffers are open for THIS backward only
            loss.backward()
        return loss.detach().view(1)

    def step(self, batch=None):
        """one optimisation step -> the loss [1] on the device (no synchronisation).  batch: (indices, uniforms) to use instead
        of drawing them"""
        it = self.iter
        idx, u = self.draw() if batch is None else batch
        for p in self.params:
            p.grad = None
        loss = self._step_hand_written(idx, u, it) if self.hand_written else self._step_autograd(idx, u, it)
        self.net.mlp_sdf.assign_grads()
        lat = self.net.encoding.lattice_values
        if self.capture_grads is not None:      # tests: the gradients of this step as the optimiser is about to see them
            extra = lat.grad if lat.grad is not None else 0.0
            self.capture_grads = {"dense": [g.detach().clone() for g in self.grad_buffer.dWs + self.grad_buffer.dbs],
                                  "lattice": (self.touched.grad + extra).clone(), "loss": loss.detach().clone()}
        self.opt.step()
        self.grad_buffer.zero()
        self.iter += 1
        return loss

    # ---- what a fit is for
    @torch.no_grad()
    def surface_error(self, points):
        """mean |sdf| at points [K, P] of the true surface, on the device"""
        return self.net.sdf_only(points.to(self.dev, torch.float32), self.iter).abs().mean()

    def extractor(self, t=None):
        """a mesh.MeshExtractor over the fitted field (a 4-D one cut at time t)"""
        from .mesh import MeshExtractor
        if self.pos_dim == 3:
            return MeshExtractor.from_sdf_net(self.net, self.iter)
        return MeshExtractor(self.net.time_slice(0.0 if t is None else t, self.iter), device=self.dev)

    def box(self):
        """the box the off-surface points are drawn from, as a box_trace.Box"""
        from .box_trace import Box
        lo, hi = self.box_lo[:3], self.box_hi[:3]
        return Box([h - l for l, h in zip(lo, hi)], [(h + l) / 2 for l, h in zip(lo, hi)])

    def tracer(self, box=None):
        """a box_trace.BoxTracer over the fitted field inside `box` (default: the fit's own), with the current window"""
        from .box_trace import BoxTracer
        return BoxTracer(self.net.encoding, self.net.mlp_sdf, self.box() if box is None else box, self.net.window(self.iter))

    def render(self, frame, t=None, box=None, slice=None, slice_style=None, **kw):
        """-> box_trace.BoxTracedFrame: the fitted field as `frame` sees it (a 4-D one at time t); kw: render_box_traced's.
        slice: a sdf_slice.SlicePlane to cut into the view -> sdf_slice.SlicedFrame instead: rgb = (normal + 1) / 2 as
        vis_4d_sdf.py:108 maps it, with the layer's isolines where the layer is in front of the surface or there is none; the
        depth and weights_sum planes of its `base` are cut in place"""
        from .box_trace import render_box_traced
        kw.setdefault("it", self.iter)
        box = self.box() if box is None else box
        out = render_box_traced(self.net, box, frame, time_val=t, **kw)
        if slice is None:
            return out
        from .sdf_slice import IsoStyle, SlicedFrame, cut_slice_into
        rgb = (out.normals + 1.0) * 0.5
        chunk = {"max_rays_per_chunk": kw["max_rays_per_chunk"]} if "max_rays_per_chunk" in kw else {}
        mask = cut_slice_into(self.net, slice, box, frame, rgb, out.depth, out.weights_sum, IsoStyle() if slice_style is None else
                              slice_style, it=kw["it"], time_val=t, **chunk)
        return SlicedFrame(base=out, rgb=rgb, depth=out.depth, weights_sum=out.weights_sum, slice_mask=mask)

    def slice(self, plane, size=500, t=None, box=None, **kw):
        """-> sdf_slice.SliceImage: the isolines of the fitted field on `plane` (a 4-D one at time t); kw: render_slice's"""
        from .sdf_slice import render_slice
        kw.setdefault("it", self.iter)
        return render_slice(self.net, plane, self.box() if box is None else box, size, time_val=t, **kw)

    # ---- checkpoints: the reference's sdf_model.pt (models.py:296-307) through checkpoint.py
    def save_checkpoint(self, folder):
        # (one process, no collectives: no parameter all-gather is ever in flight here, unlike train_step.Trainer.save_checkpoint,
        # which waits for its own first; a data-parallel step added to this fitter has to bring that wait along)
        from . import checkpoint
        checkpoint.save(folder, sdf=self.net)

    def load_checkpoint(self, folder):
        from . import checkpoint
        checkpoint.load(folder, sdf=self.net, map_location=self.dev)
