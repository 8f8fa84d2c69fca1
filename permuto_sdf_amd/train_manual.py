"""BASELINE config 4 with a HAND-WRITTEN backward: the same optimisation step as `train_step.Trainer` (same networks, samplers,
losses, schedule, optimiser, data-parallel reduction -- it IS a Trainer), but the main phase's forward and backward are
written out over the raw feature-major kernels instead of being recorded and replayed by torch autograd.

Why: the step is host bound (train_step.py, DESIGN.md sections 4.5 and 8): ~250 launches, the autograd engine's bookkeeping
(`run_backward` alone is a third of the host time), [N, C] <-> [C, N] glue around every Function, gradient-accumulation adds
and zero fills that autograd inserts.  Written by hand, every tensor stays feature-major, every gradient is produced once where
it is needed, the three evaluations of the SDF network share one parameter image, and the four contributions to the SDF
network's parameter gradient land in one buffer.

What is differentiated (train_permuto_sdf.py:311-429, run_net :111-169; names as in train_step.py):
  fg samples -> SDF net: y = mlp(enc(p)) -> sdf = y[0], geom = y[1:33];  n = d sdf / d p  (MLP data backward of e0, then the
  encoding's position backward);  colour = sigmoid(Lipshitz-MLP([enc2(p), SH5(dir), normalize(n), geom]));
  (radiance, bgT) = NeuS(sdf, n, colour);  bg samples -> NerfHash -> radiance_bg;  pred = radiance + bgT * radiance_bg;
  loss = L1(pred, gt) + w_e eikonal(n) + w_c curvature(n, n(p + eps cross(norm n, norm r))) + w_o offsurface(sdf(p_off)) [+ Lipschitz].
A `--with_mask` run (train_permuto_sdf.py:153-154,381-383) has no background branch: pred = radiance, and the loss gains
w_m BCE(clip(sum of the NeuS weights per ray, 1e-3, 1 - 1e-3), mask): the render with that sum and the colour + mask loss tail are
csrc/neus_render.hip (`_masked_render_and_loss`; tests/test_gpu_train_mask_step.py holds it against the autograd trainer).
The backward of  n = d sdf / d p  is the double backward: `psdf_encode_double_backward` (gradient w.r.t. the lattice and w.r.t.
the feature gradient) -> `psdf_mlp_double_backward` (gradient w.r.t. features and parameters) -> the encoding's lattice backward.
`tests/test_gpu_train_step.py::test_manual_backward_equals_autograd` holds every gradient of this file against the autograd
trainer's on the same batch.

Layout: `_main_phase` = `_main_forward` (sampling, every forward, every loss kernel, grid refresh, prefetch) -> a `_Step` record
-> `_main_backward`; each half is a sequence of stages (`_fg_forward` / `_fg_backward`, `_curvature_*`, `_offsurface_*`, `_calib_*`).
"""
import os
from types import SimpleNamespace

import torch

from . import _lib as L
from .bridge import PermutoSDF, RaySamplesPacked, VolumeRendering as VR
from .encoding import map_range_val
from .mlp import (_grad_views, double_backward_plus_supported, mlp_forward_wide_f16_raw, lipshitz_normalize_all_backward_raw, lipshitz_normalize_all_raw, mlp_backward_raw,
                  mlp_forward_raw, pack_params)
from .net_eval import enc_backward, enc_forward, net_params, sdf_gradient, sdf_gradient_backward, set_grads
from .neus import (eikonal_loss_raw, l1_loss_raw, nerf_composite_backward_raw, nerf_composite_forward_raw, neus_composite_backward_raw,
                   neus_composite_forward_raw, neus_mask_loss_raw, neus_render_backward_raw, neus_render_forward_raw,
                   sigmoid_rows_backward_raw, sigmoid_rows_raw)
from .train_step import Trainer


def _normalize3(x, gy=None):
    out = torch.empty_like(x)
    L.call("psdf_normalize3", L.c_l(x.shape[0]), L.ptr(x), L.ptr(gy), L.ptr(out), L.stream())
    return out


class _Step:
    """What `_main_forward` hands to `_main_backward`: every field exists from the start, None until its stage has run, so the
    backward tests the field (calib, g_cw_bg, g_cb_bg: colour calibration; fg, g_n: foreground samples; curv: curvature weight
    > 0; g_ws: the weight sum's gradient of a masked step, which has no bg, g_bgT, g_cw_bg, g_cb_bg) and not the condition the
    forward ran under.  calib, net, bg, fg, curv are small records (SimpleNamespace), each built
    in one place: `_calib_build`, `_main_forward`, `_bg_forward`, `_fg_forward`, `_curvature_forward`."""
    __slots__ = ("it", "R", "n_fg", "loss", "calib", "net", "inv_s", "cos_r", "arena", "bg", "fg", "curv", "off", "feat_o",
                 "g_pred", "g_bgT", "g_ws", "g_n", "g_cw_bg", "g_cb_bg")

    def __init__(self, **kw):
        for name in self.__slots__:
            setattr(self, name, kw.pop(name, None))
        assert not kw, kw


def _calib_sigmoid(calib, raw_fm, ray_start_end_idx):
    """[3, N] raw colours -> ((calibrated) sigmoid [N, 3], raw colours [N, 3], ray of each sample [N]); the last two with
    calibration only"""
    if calib is None:
        return sigmoid_rows_raw(raw_fm), None, None
    raw = raw_fm.t().contiguous()
    ridx = RaySamplesPacked.compute_per_sample_ray_idx(ray_start_end_idx, raw.shape[0]).long()
    return torch.sigmoid(raw * calib.cw.index_select(0, ridx) + calib.cb.index_select(0, ridx)), raw, ridx


def _calib_sigmoid_backward(calib, g_rgb, rgb, raw, ridx):
    """-> (gradient of the raw colours [3, N], g_cw [R, 3], g_cb [R, 3]); the last two None without calibration"""
    if calib is None:
        return sigmoid_rows_backward_raw(g_rgb, rgb), None, None                         # one launch
    g_pre = g_rgb * rgb * (1.0 - rgb)                                                     # sigmoid
    g_cb = torch.zeros(calib.cb.shape, device=g_pre.device).index_add_(0, ridx, g_pre)
    g_cw = torch.zeros(calib.cb.shape, device=g_pre.device).index_add_(0, ridx, g_pre * raw)
    return (g_pre * calib.cw.index_select(0, ridx)).t().contiguous(), g_cw, g_cb


class ManualTrainer(Trainer):
    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        assert self.touched, "ManualTrainer accumulates the lattice gradients in the touched-rows buffers"
        self._g_yo = None
        # the NEXT step's rays, sphere intersection, occupancy march and background samples are issued on a side stream as soon
        # as this step's grid refresh is enqueued, and run beside this step's backward (PSDF_TRAIN_PREFETCH=0: off)
        self.prefetch_sampling = os.environ.get("PSDF_TRAIN_PREFETCH", "1") != "0"
        self._prefetched = None
        self._prefetch_side = None
        self._pos_pool = None
        # the SDF net's plain backward (g_y) inside the double backward's launch (g_n); PSDF_TRAIN_FUSE_SDF_BWD=0: two launches
        self.fuse_sdf_backward = os.environ.get("PSDF_TRAIN_FUSE_SDF_BWD", "1") != "0"

    # ------------------------------------------------------------------ next step's sampling, first half, ahead of time
    def _prefetch_valid(self, git, reel=None):
        """reel: the image reel the coming step samples from (None: not checked).  A prefetch drawn from ANOTHER reel must be
        dropped by the step's own validity test too -- step() skips its seeding on the strength of this answer."""
        pf = self._prefetched
        return (pf is not None and pf["git"] == git and pf["nr_rays"] == self.nr_rays and self._hand_written_step_applies()
                and (reel is None or pf["reel"] == id(reel))
                and "_draw_rays" not in self.__dict__ and "_samples" not in self.__dict__)

    def _drop_prefetch(self):
        """A prefetch that does not fit the coming step is undone as far as the random streams go: the jitter generators
        (process-global PCG32 streams of the occupancy grid / ray sampler / volume renderer, advanced once by the prefetched
        launches) return to their state before it.  The caller re-seeds torch's generators for its iteration."""
        pf, self._prefetched = self._prefetched, None
        if pf is not None and pf.get("pcg") is not None:
            from .bridge import OccupancyGrid, RaySampler, VolumeRendering
            owners = (OccupancyGrid, RaySampler, VolumeRendering)
            # only where the stream still stands where the prefetch left it: a caller that has set the generators itself since
            # (tools/reference_step_parity.py copies the reference's states in) keeps what it set
            for cls, (st, inc), after in zip(owners, pf["pcg"], pf["pcg_after"]):
                if (cls._rng.state, cls._rng.inc) == after:
                    cls._rng.state, cls._rng.inc = st, inc

    def _launch_prefetch(self, reel, next_git):
        """The march is the largest kernel of the step (0.21 ms) and runs on 12 waves: nothing it needs -- the grid, the image
        reel, the ray count -- changes after `_refresh_and_adapt`, and nothing else of the step draws from torch's generators
        after that point.  So the generators are seeded for the next iteration HERE, its rays are drawn, intersected and marched
        and its background samples placed on a side stream while this step's backward and optimiser run; the next step skips
        its own seeding and starts from the generator state this leaves -- the very state it would have had after drawing its
        rays itself.  The side stream first waits for the main stream (the refreshed grid), the next step's main stream waits
        for the side stream's event.  Tensors allocated here live in the side stream's pool and are next reused by the NEXT
        prefetch, whose work again starts behind a fresh event of the main stream: no kernel of either stream can still be
        reading them.  A prefetch that does not fit the step that comes (iteration counter or ray count changed from outside,
        samplers patched by a test) is dropped."""
        if (not self.prefetch_sampling or self.dev.type != "cuda" or "_draw_rays" in self.__dict__
                or "_samples" in self.__dict__):
            self._prefetched = None
            return
        from . import parallel
        main = torch.cuda.current_stream(self.dev)
        if self._prefetch_side is None:
            self._prefetch_side = torch.cuda.Stream(device=self.dev)
        side = self._prefetch_side
        ev = torch.cuda.Event()
        ev.record(main)
        side.wait_event(ev)
        from .bridge import OccupancyGrid, RaySampler, VolumeRendering
        pcg = [(c._rng.state, c._rng.inc) for c in (OccupancyGrid, RaySampler, VolumeRendering)]     # (see _drop_prefetch)
        parallel.seed_generators(parallel.step_seed(self._seed, parallel.rank(), next_git), self.dev)
        with torch.cuda.stream(side), torch.no_grad():
            rays = self._draw_rays(reel)
            begun = self._samples_begin(rays[0], rays[1], True)
            done = torch.cuda.Event()
            done.record(side)
        pcg_after = [(c._rng.state, c._rng.inc) for c in (OccupancyGrid, RaySampler, VolumeRendering)]
        self._prefetched = dict(git=next_git, nr_rays=self.nr_rays, reel=id(reel), rays=rays, begun=begun, done=done, pcg=pcg,
                                pcg_after=pcg_after)

    def _hand_written_step_applies(self):
        """The hand-written step is built on the fused compositing kernels (at most 256 samples per ray: foreground
        max_nr_samples_per_ray + 2 * nr_samples_imp_sampling, background nr_samples_bg).  Both of the reference's modes run it:
        the default one (background network, csrc/composite_fused.hip) and `--with_mask` (no background: only the foreground
        bound applies; the render with the per-ray weight sum and the colour + mask loss tail of csrc/neus_render.hip).
        Anything else runs `Trainer._main_phase`: the same step as an autograd graph over the per-operator chain -- slower, any
        ray length."""
        hp = self.hp
        fg_fits = hp.max_nr_samples_per_ray + 2 * hp.nr_samples_imp_sampling <= 256
        return fg_fits if self.with_mask else (fg_fits and hp.nr_samples_bg <= 256)

    # ------------------------------------------------------------------ the SDF network, one evaluation
    def _sdf_gradient(self, feat, pts, net):
        return sdf_gradient(self.sdf.encoding, feat, pts, net, self._zeroed_pos(pts))

    def _zeroed_pos(self, pts):
        """a zero-filled [N, 3] tensor for a position gradient: the step needs three of the same size (normals of the samples, of
        the shifted samples, gradient of the shifted points) -- ONE fill launch for the three instead of one each"""
        pool = self._pos_pool
        if pool is None or pool[0].shape[1:] != pts.shape or pool[1] >= pool[0].shape[0]:
            pool = self._pos_pool = [torch.zeros((3,) + tuple(pts.shape), dtype=torch.float32, device=pts.device), 0]
        pool[1] += 1
        return pool[0][pool[1] - 1]

    def _grad_arena(self):
        """zero-filled parameter-gradient views for the three nets without a persistent gradient buffer (background density net,
        background colour head, colour network's normalised weights) and the four Lipschitz bounds: ONE fill launch per step
        instead of four (the kernels accumulate into what they are given) -> (bg1, bg2, rgb, dc_flat), each (dWs, dbs)"""
        lay = self.__dict__.get("_arena_layout")
        if lay is None:
            def need(dims):
                return sum(((dims[l + 1] * dims[l] + 3) & ~3) + ((dims[l + 1] + 3) & ~3) for l in range(len(dims) - 1))
            d1, d2, dc = self.bg.mlp_feat_and_density.dims, self.bg.mlp_rgb.dims, self.rgb.mlp.dims
            offs = [0]
            for sz in (need(d1), need(d2), need(dc), 4 * (len(dc) - 1)):
                offs.append(offs[-1] + sz)
            lay = self._arena_layout = (offs, d1, d2, dc)
        offs, d1, d2, dc = lay
        flat = torch.zeros(offs[-1], dtype=torch.float32, device=self.dev)
        views = [_grad_views(d, flat=flat[offs[i]:offs[i + 1]])[1:] for i, d in enumerate((d1, d2, dc))]
        return views[0], views[1], views[2], flat[offs[3]:offs[4]]

    def _sdf_gradient_backward(self, g_n, feat, dfeat, e0, pts, net, want_pos=False, extra_dfeat=None, extra_gy=None):
        return sdf_gradient_backward(self.sdf.encoding, self.sdf.mlp_sdf, g_n, feat, dfeat, e0, pts, net, extra_dfeat=extra_dfeat,
                                     extra_gy=extra_gy, zeroed=self._zeroed_pos(pts) if want_pos else None)

    # ------------------------------------------------------------------ the background branch (NerfHash, models.py:431-526)
    def _bg_forward(self, bg, calib):
        """4-D lattice -> density + feature net -> [gelu(features), SH4(dir)] -> colour head -> (calibrated) sigmoid.  Everything
        the compositing and the backward need, as a record (net1, net2: `net_params` of the two MLPs; rgbb_raw, ridx: None without calibration)."""
        bgn = self.bg
        self._params_ready(2)              # the background lattice's parameters (all-gather of the previous step, data parallel)
        p4, dirs_b = bg.samples_pos_4d, bg.samples_dirs
        feat4 = enc_forward(bgn.encoding, p4, bgn._win)
        net1 = d1, _, w1b, b1b = net_params(bgn.mlp_feat_and_density)
        fd = mlp_forward_wide_f16_raw(d1, feat4, w1b, b1b)                                # [65, M] on the fp16 matrix pipe (round 6)
        if fd is None:      # (the library declined: fp32 MFMAs)
            fd = mlp_forward_raw(d1, feat4, pack_params(d1, w1b, b1b))
        gel = torch.nn.functional.gelu(fd[1:65])
        sh4 = PermutoSDF.spherical_harmonics(dirs_b, 4)
        x2 = torch.cat([gel, sh4.t()], 0)                                                 # [80, M]
        net2 = d2, _, w2b, b2b = net_params(bgn.mlp_rgb)
        rgbb_fm = mlp_forward_raw(d2, x2, pack_params(d2, w2b, b2b))                      # [3, M]
        rgbb, rgbb_raw, ridx = _calib_sigmoid(calib, rgbb_fm, bg.ray_start_end_idx)
        return SimpleNamespace(p4=p4, feat4=feat4, fd=fd, x2=x2, net1=net1, net2=net2, rgbb=rgbb, rgbb_raw=rgbb_raw, ridx=ridx,
                               raw_den=fd[0])         # raw_den [M]: a row of the feature-major output

    def _bg_backward(self, B, g_raw, g_rgbb, calib, into1, into2):
        """-> (g_cw, g_cb) of the colour calibration (or None, None); the networks' gradients are accumulated into the zero-filled
        views into1 (density + feature net) / into2 (colour head) and set, the lattice's into its buffer"""
        bgn, (d1, l1b, w1b, b1b), (d2, l2b, w2b, b2b) = self.bg, B.net1, B.net2
        g_pre_b_fm, g_cw, g_cb = _calib_sigmoid_backward(calib, g_rgbb, B.rgbb, B.rgbb_raw, B.ridx)
        dX2b, dW2b, db2b = mlp_backward_raw(d2, B.x2, w2b, b2b, g_pre_b_fm, need_dx=True, into=into2)
        set_grads(l2b, dW2b, db2b)
        g_fd = torch.cat([g_raw.view(1, -1), torch.ops.aten.gelu_backward(dX2b[:64], B.fd[1:65])], 0)      # [65, M]
        dX4, dW1b, db1b = mlp_backward_raw(d1, B.feat4, w1b, b1b, g_fd, need_dx=True, into=into1)
        set_grads(l1b, dW1b, db1b)
        enc_backward(bgn.encoding, B.p4, bgn._win, dX4)
        return g_cw, g_cb

    # ------------------------------------------------------------------ per-ray colour calibration (the sigmoids: _calib_sigmoid*)
    def _calib_build(self, img_idx):
        """per-ray calibration of both branches (models.py:384-385,523-524): colour = sigmoid(raw * cw + cb), [R, 3] each; cam [R]:
        the ray's image, fixed [R, 1]: rays of the image that keeps the identity.  None without a calibration model."""
        cc = self.colorcal
        if cc is None:
            return None
        cam = img_idx.long()
        fixed = (cam == cc.idx_with_fixed_calib)[:, None]
        cw = torch.where(fixed, torch.ones_like(cc.weight_delta[:1]), 1.0 + cc.weight_delta.index_select(0, cam))
        cb = torch.where(fixed, torch.zeros_like(cc.bias[:1]), cc.bias.index_select(0, cam))
        return SimpleNamespace(cw=cw, cb=cb, fixed=fixed, cam=cam)

    def _calib_assign_grads(self, calib, g_cw_bg, g_cb_bg, g_cw, g_cb):
        """per-ray gradients of both branches (the foreground's None without foreground samples) -> weight_delta.grad, bias.grad"""
        cc = self.colorcal
        if g_cw_bg is None:                                        # a masked step: the foreground's alone ...
            if g_cw is None:                                       # ... and nothing without foreground samples (step() fills zeros)
                return
        else:
            g_cw = g_cw_bg if g_cw is None else g_cw_bg + g_cw     # background first: the order the sums have always been taken in
            g_cb = g_cb_bg if g_cb is None else g_cb_bg + g_cb
        fixed3 = calib.fixed.expand(-1, 3)
        gwd = torch.zeros_like(cc.weight_delta).index_add_(0, calib.cam, torch.where(fixed3, torch.zeros_like(g_cw), g_cw))
        gbi = torch.zeros_like(cc.bias).index_add_(0, calib.cam, torch.where(fixed3, torch.zeros_like(g_cb), g_cb))
        cc.weight_delta.grad, cc.bias.grad = gwd, gbi

    # ------------------------------------------------------------------ the foreground branch: SDF net, colour net, NeuS compositing
    def _fg_forward(self, st, fgs):
        """-> (pred_fg [R, 3], bgT [R, 1]), a masked step: (pred [R, 3], weights_sum [R, 1]); st.fg: what the curvature term and
        the backward need (c_enc, c_sh: row offsets in x_rgb = [colour encoding | SH | normal | geometry features]; rgb_raw, ridx:
        None without calibration)"""
        net, rgbn = st.net, self.rgb
        pts = fgs.samples_pos
        feat = enc_forward(self.sdf.encoding, pts, net.win)
        y = mlp_forward_raw(net.dims, feat, net.packed)                                   # [33, N]: sdf, geometry features
        n, dfeat, e0 = self._sdf_gradient(feat, pts, net)
        self._params_ready(1)              # the colour lattice's parameters: before the colour encode, not earlier
        feat2 = enc_forward(rgbn.encoding, pts, rgbn._win)
        sh = PermutoSDF.spherical_harmonics(fgs.samples_dirs, 5)
        nn = _normalize3(n)
        x_rgb = torch.cat([feat2, sh.t(), nn.t(), y[1:]], 0)                              # [111, N]
        m = rgbn.mlp
        wn = lipshitz_normalize_all_raw(m.weights_per_layer, m.lipshitz_bound_per_layer)      # all four layers, one launch
        bsr = [b.detach() for b in m.biases_per_layer]
        rgb_fm = mlp_forward_wide_f16_raw(m.dims, x_rgb, wn, bsr)                         # [3, N]
        if rgb_fm is None:      # (the library declined: fp32 MFMAs)
            rgb_fm = mlp_forward_raw(m.dims, x_rgb, pack_params(m.dims, wn, bsr))
        rgb, rgb_raw, ridx = _calib_sigmoid(st.calib, rgb_fm, fgs.ray_start_end_idx)
        st.fg = SimpleNamespace(samples=fgs, pts=pts, feat=feat, dfeat=dfeat, e0=e0, n=n, sdf_col=y[0].view(-1, 1), x_rgb=x_rgb,
                                c_enc=feat2.shape[0], c_sh=feat2.shape[0] + sh.shape[1], wn=wn, bsr=bsr, rgb=rgb, rgb_raw=rgb_raw, ridx=ridx)
        if self.with_mask:                 # no background behind it: the radiance IS the prediction, the weight sum feeds the mask loss
            pred, ws, _ = neus_render_forward_raw(fgs, st.fg.sdf_col, n, rgb, st.inv_s, st.cos_r)
            return pred, ws
        pred_fg, bgT, _ = neus_composite_forward_raw(fgs, st.fg.sdf_col, n, rgb, st.inv_s, st.cos_r)
        return pred_fg, bgT

    def _fg_backward(self, st):
        """NeuS compositing -> colour net (+ Lipschitz normalisation) -> colour lattice; then everything that reached n and the
        SDF net's outputs, through the SDF net once -> (g_cw, g_cb) of the colour calibration (or None, None)"""
        fg, net, hp, rgbn, m = st.fg, st.net, self.hp, self.rgb, self.rgb.mlp
        per_ray = hp.max_nr_samples_per_ray + 2 * hp.nr_samples_imp_sampling
        if st.g_ws is not None:            # a masked step: gradients of the colour and of the weight sum, none of the bg transmittance
            g_sdf, g_nc, g_rgb, _ = neus_render_backward_raw(fg.samples, per_ray, st.g_pred, st.g_ws, None, fg.sdf_col, fg.n, fg.rgb,
                                                             st.inv_s, st.cos_r, need_grad=True, need_rgb=True, need_inv_s=False)
        else:
            g_sdf, g_nc, g_rgb, _ = neus_composite_backward_raw(fg.samples, per_ray, st.g_pred.contiguous(), st.g_bgT.contiguous(), fg.sdf_col,
                                                                fg.n, fg.rgb, st.inv_s, st.cos_r, need_grad=True, need_rgb=True, need_inv_s=False)
        g_pre_fm, g_cw, g_cb = _calib_sigmoid_backward(st.calib, g_rgb, fg.rgb, fg.rgb_raw, fg.ridx)
        dXr, dWn, dbr = mlp_backward_raw(m.dims, fg.x_rgb, fg.wn, fg.bsr, g_pre_fm, need_dx=True, into=st.arena[2])
        dws, dcs = lipshitz_normalize_all_backward_raw(m.weights_per_layer, m.lipshitz_bound_per_layer, dWn, dc_flat=st.arena[3])
        for i, (w, c) in enumerate(zip(m.weights_per_layer, m.lipshitz_bound_per_layer)):
            w.grad, c.grad, m.biases_per_layer[i].grad = dws[i], dcs[i].view_as(c), dbr[i]
        enc_backward(rgbn.encoding, fg.pts, rgbn._win, dXr[:fg.c_enc])
        self._dp_lattice_final(1)          # right after the colour encode backward: the colour lattice's gradient is final
        g_n = st.g_n + g_nc + _normalize3(fg.n, dXr[fg.c_sh:fg.c_sh + 3].t().contiguous())
        g_y = torch.cat([g_sdf.view(1, -1), dXr[fg.c_sh + 3:]], 0)                        # [33, N]
        if st.curv is not None:
            g_n = self._curvature_backward(st, g_n)
        # first evaluation: from (sdf, geom) directly and from n through the double backward; ONE lattice scatter
        if self.fuse_sdf_backward and double_backward_plus_supported(net.dims):
            self._sdf_gradient_backward(g_n, fg.feat, fg.dfeat, fg.e0, fg.pts, net, extra_gy=g_y)
        else:
            dX1, _, _ = mlp_backward_raw(net.dims, fg.feat, net.ws, net.bs, g_y, need_dx=True, into=(net.gb.dWs, net.gb.dbs))
            self._sdf_gradient_backward(g_n, fg.feat, fg.dfeat, fg.e0, fg.pts, net, extra_dfeat=dX1)
        return g_cw, g_cb

    def _masked_render_and_loss(self, st, fgs, gt, hit, gt_mask):
        """The `--with_mask` form of render + colour loss (train_permuto_sdf.py:153-154,372,381-383): the foreground's radiance is
        the prediction, its per-ray weight sum is held to the mask.  One render launch and ONE loss launch that adds both terms
        to st.loss and leaves st.g_pred, st.g_ws.  Without foreground samples the render is 0, 0: the tail still runs (its value
        is part of the loss), nothing flows back."""
        if st.n_fg:
            pred, ws = self._fg_forward(st, fgs)
        else:
            pred, ws = torch.zeros(st.R, 3, device=self.dev), torch.zeros(st.R, 1, device=self.dev)
        _, st.g_pred, st.g_ws = neus_mask_loss_raw(pred, gt, hit, ws, gt_mask, self.hp.mask_weight, loss=st.loss)

    # ------------------------------------------------------------------ curvature term: n against n at a point 1e-4 along a tangent
    def _curvature_forward(self, st, weight):
        """st.curv: the shifted points' evaluation; ga, gb2: the loss kernel's gradients w.r.t. n and the shifted points' normals"""
        fg, net, n_fg = st.fg, st.net, st.n_fg
        rnd = torch.randn_like(fg.pts)     # torch's first random draw of the step after the rays
        shifted = torch.empty_like(fg.pts)
        L.call("psdf_curvature_shift", L.c_l(n_fg), L.ptr(fg.pts), L.ptr(fg.n), L.ptr(rnd), L.c_f(1e-4), None, L.ptr(shifted), L.stream())
        feat_s = enc_forward(self.sdf.encoding, shifted, net.win)
        n2, dfeat_s, _ = self._sdf_gradient(feat_s, shifted, net)
        ga, gb2 = torch.empty_like(fg.n), torch.empty_like(n2)
        L.call("psdf_curvature_loss", L.c_l(n_fg), L.ptr(fg.n), L.ptr(n2), L.c_f(weight / n_fg), L.ptr(st.loss), L.ptr(ga), L.ptr(gb2),
               L.stream())
        st.curv = SimpleNamespace(rnd=rnd, shifted=shifted, feat_s=feat_s, dfeat_s=dfeat_s, ga=ga, gb2=gb2)

    def _curvature_backward(self, st, g_n):
        """-> g_n plus the term's two contributions: directly, and through the shifted points (which depend on n)"""
        fg, net, cv = st.fg, st.net, st.curv
        g_n = g_n + cv.ga
        g_shift = self._sdf_gradient_backward(cv.gb2, cv.feat_s, cv.dfeat_s, fg.e0, cv.shifted, net, want_pos=True)
        g_from_shift = torch.empty_like(fg.n)
        L.call("psdf_curvature_shift", L.c_l(st.n_fg), None, L.ptr(fg.n), L.ptr(cv.rnd), L.c_f(1e-4), L.ptr(g_shift), L.ptr(g_from_shift),
               L.stream())
        return g_n + g_from_shift

    # ------------------------------------------------------------------ off-surface term: 1024 points inside the sphere
    def _offsurface_forward(self, st):
        net = st.net
        st.off = self.sphere.rand_points_inside(1024)      # torch's random draw after the curvature shift's
        st.feat_o = enc_forward(self.sdf.encoding, st.off, net.win)
        y_o = mlp_forward_raw(net.dims, st.feat_o, net.packed)
        # the term's gradient w.r.t. the net's 33 outputs is zero except in row 0 (the SDF): a persistent [33, 1024] buffer whose
        # rows 1.. stay zero, row 0 rewritten by the loss kernel every step (no fill, no copy)
        if self._g_yo is None:
            self._g_yo = torch.zeros((net.dims[-1], 1024), dtype=torch.float32, device=self.dev)
        L.call("psdf_offsurface_loss", L.c_l(1024), L.ptr(y_o[0]), L.c_f(1e2), L.c_f(self.hp.offsurface_weight / 1024.0), L.ptr(st.loss),
               L.ptr(self._g_yo[0]), L.stream())

    def _offsurface_backward(self, st):
        net = st.net
        dXo, _, _ = mlp_backward_raw(net.dims, st.feat_o, net.ws, net.bs, self._g_yo, need_dx=True, into=(net.gb.dWs, net.gb.dbs))
        enc_backward(self.sdf.encoding, st.off, net.win, dXo)

    # ------------------------------------------------------------------ one iteration of the main phase
    def _main_phase(self, reel, it, git, eikonal_weight):
        """One stream.  (The background branch on a second stream was measured and lost 9 %: LABNOTES.md, "The background branch
        on a second stream", profiles/r04_train_streams_ab.jsonl.)"""
        if not self._hand_written_step_applies():
            return Trainer._main_phase(self, reel, it, git, eikonal_weight)
        st = self._main_forward(reel, it, git, eikonal_weight)
        self._main_backward(st)
        return st.loss.view(()), st.n_fg, st.R, True

    def _step_rays(self, reel, git):
        """-> (rays, the prefetched first half of their sampling or None)"""
        if self._prefetch_valid(git, reel):
            pf, self._prefetched = self._prefetched, None
            torch.cuda.current_stream(self.dev).wait_event(pf["done"])
            return pf["rays"], pf["begun"]
        # (step() has seeded this iteration itself in that case: it asks the same question with the same reel)
        self._drop_prefetch()
        return self._draw_rays(reel), None

    @torch.no_grad()
    def _main_forward(self, reel, it, git, eikonal_weight):
        """Sampling, every forward, every loss kernel (each produces its gradient in the same launch), grid refresh, prefetch.
        The background branch's backward belongs to this half too: it needs nothing but the compositing's gradients, and enqueued
        right behind them its lattice's reduction (data parallel) overlaps all the rest -- the background is finished when this
        returns, `_main_backward` is the foreground's and the off-surface points'."""
        hp, dev, sdfn = self.hp, self.dev, self.sdf
        (o, d, gt, hit, img_idx, gt_mask), begun = self._step_rays(reel, git)
        st = _Step(it=it, R=o.shape[0], calib=self._calib_build(img_idx),
                   cos_r=map_range_val(it, 0.0, hp.forced_variance_finish_iter, 0.0, 1.0))
        # the background network's forward is enqueued from the hook, while the host waits for the march's sample counts (it needs
        # the background samples only), so the step's one host sync leaves no bubble on the GPU
        if self.with_mask:                 # no background samples, no background network: nothing to enqueue meanwhile
            fgs, bgs = self._samples(o, d, it, True, begun=begun)
            self._params_ready(2)          # (the background lattice is not read: its gather of the previous step is retired here)
        else:
            fgs, bgs = self._samples(o, d, it, True, begun=begun, between=lambda bg_: setattr(st, "bg", self._bg_forward(bg_, st.calib)))
            if st.bg is None:              # (a sampler replaced from outside that left the hook alone)
                st.bg = self._bg_forward(bgs, st.calib)
        st.n_fg = fgs.samples_pos.shape[0]
        # the SDF lattice's parameters, before anything below reads them (data parallel): a no-op after `Trainer._samples`, which
        # waits before its first sdf_only; it counts for a sampler replaced from outside
        self._params_ready(0)
        dims, _, ws, bs = net_params(sdfn.mlp_sdf)
        # the SDF network as the step's three evaluations share it; win: this iteration's lattice window, gb: its gradient buffer
        st.net = SimpleNamespace(dims=dims, ws=ws, bs=bs, win=sdfn.window(it).contiguous(), packed=pack_params(dims, ws, bs),
                                 gb=self.grad_buffers[0])
        # exp(10 v) clipped, as RgbNet.neus_render computes it: evaluated in float32 on the host and uploaded (one 4-byte copy
        # instead of a copy + exp + clamp on the device; the schedule is a host scalar anyway)
        forced_variance = map_range_val(it, 0.0, hp.forced_variance_finish_iter, 0.3, hp.forced_variance_finish)
        st.inv_s = torch.exp(torch.tensor(float(forced_variance) * 10.0, dtype=torch.float32, device="cpu")).clip(1e-6, 1e6).view(1).to(dev)
        self.rgb.last_inv_s = st.inv_s.view(())
        st.loss = L.zeroed_scalar(dev)     # ONE accumulator: every loss kernel of the step adds its (already weighted) term to it
        self._pos_pool = None              # (zero-filled position gradients: a fresh pool per step)
        st.arena = self._grad_arena()      # zero-filled parameter gradients of the nets without a persistent buffer: one fill
        if self.with_mask:
            self._masked_render_and_loss(st, fgs, gt, hit, gt_mask)
        else:
            if st.n_fg:
                pred_fg, bgT = self._fg_forward(st, fgs)
            else:
                pred_fg, bgT = torch.zeros(st.R, 3, device=dev), torch.ones(st.R, 1, device=dev)
            # softplus -> opacity -> transmittance -> weights -> background radiance -> pred = pred_fg + bgT * pred_bg: one launch
            _, pred = nerf_composite_forward_raw(bgs, st.bg.raw_den, st.bg.rgbb, pred_fg, bgT)
            _, st.g_pred = l1_loss_raw(pred, gt, hit, loss=st.loss)
            # pred = pred_fg + bgT * pred_bg and the whole background compositing backward, one launch
            g_raw, g_rgbb, st.g_bgT = nerf_composite_backward_raw(bgs, hp.nr_samples_bg, st.g_pred, st.bg.raw_den, st.bg.rgbb, bgT)
            st.g_cw_bg, st.g_cb_bg = self._bg_backward(st.bg, g_raw, g_rgbb, st.calib, st.arena[0], st.arena[1])
        # right after the background backward: its lattice's reduction overlaps what follows (a masked step: the buffer is zero
        # and final from the start; the collective keeps its place so that every rank issues the same sequence)
        self._dp_lattice_final(2)
        if st.n_fg:
            _, st.g_n = eikonal_loss_raw(st.fg.n, scale=eikonal_weight / st.n_fg, loss=st.loss)
            gw = map_range_val(it, hp.iter_start_reduce_curv, hp.iter_finish_reduce_curv, 1.0, 0.0)
            if gw > 0.0:
                self._curvature_forward(st, hp.curvature_weight * gw)
        self._offsurface_forward(st)
        # after the last loss kernel, before the first foreground backward launch: the refresh, THEN the next step's sampling
        self._refresh_and_adapt(it, git, st.n_fg)
        self._launch_prefetch(reel, git + 1)
        return st

    def _main_backward(self, st):
        """The foreground's and the off-surface points' backward from what `_main_forward` left in `st` (the background's is under
        way), the colour calibration's gradients of both branches, the Lipschitz bound's term (added to st.loss)."""
        hp = self.hp
        with torch.no_grad():
            g_cw = g_cb = None
            if st.fg is not None:
                g_cw, g_cb = self._fg_backward(st)
            else:
                self._dp_lattice_final(1)      # (no foreground samples on this rank: the same collective at the same point)
            self._offsurface_backward(st)
            if st.calib is not None:
                self._calib_assign_grads(st.calib, st.g_cw_bg, st.g_cb_bg, g_cw, g_cb)
        if st.it >= hp.iter_start_reduce_curv:      # the Lipschitz bound: four scalars, autograd is fine
            bounds = list(self.rgb.mlp.lipshitz_bound_per_layer)
            lb = self.rgb.mlp.lipshitz_bound_full().mean() * hp.lipshitz_weight
            for c, g in zip(bounds, torch.autograd.grad(lb, bounds)):
                c.grad = g if c.grad is None else c.grad + g
            st.loss = st.loss + lb.detach()
