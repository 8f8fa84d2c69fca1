"""A lattice + MLP net evaluated outside autograd: the ONE home of what the trainers, the tracers and the mesh extractor share.

  * `one_row_head(mlp)`         the net with a 1-row head: channel 0 of the last layer is the SDF (models.py:190-192) or the raw
                                density (models.py:528-550), and whoever needs nothing else evaluates the same arithmetic for
                                that row with 1/33 (1/65) of the output traffic;
  * `scalar_only`               lattice kernel, then the MLP with that head: two launches, every point;
  * `masked_sdf`                the same pair under a per-point mask (masked points: no gathers; fully masked 32-sample tiles: no
                                MLP), into buffers the caller keeps;
  * `masked_sdf_gradient`       d sdf / d x of the points that are not masked: the MLP's data backward of a unit output gradient,
                                then the encoding's position backward;
  * `raw`, `enc_forward`, ...   one pass of a hand-written training step over the raw feature-major kernels, and
                                `sdf_gradient` / `sdf_gradient_backward`: n = d sdf / d p with its double backward.

Nothing here synchronises with the host, and every function issues exactly the launches its docstring names: the callers are
host bound (the cfg-4 step), captured into hipGraphs (`SphereTracer.capture`, `BoxPlayer`) or run beside a side stream.  Imports
nothing of the package but `_lib`, `encoding` and `mlp`.
"""
import ctypes

import torch

from . import _lib as L
from .encoding import _head, _tail, encode_backward_raw, encode_double_backward_raw, encode_forward_raw
from .mlp import _dims_array, mlp_backward_raw, mlp_double_backward, mlp_forward_raw, pack_params


# ---------------------------------------------------------------------------------------------------------------- the 1-row head
class OneRowHead:
    """dims, ws, bs of an MLP whose last layer is cut to its row 0 (views of the module's parameters, no copy), and `packed`, the
    MFMA-operand image of them: None until `pack()` (one small launch)"""
    __slots__ = ("dims", "ws", "bs", "packed", "_pointers")

    def __init__(self, dims, ws, bs):
        self.dims, self.ws, self.bs, self.packed, self._pointers = dims, ws, bs, None, None

    def pack(self):
        if self.packed is None:
            self.packed = pack_params(self.dims, self.ws, self.bs)
        return self.packed

    def pointers(self):
        """(n_layers, weights, biases) as the unpacked kernels take them: two arrays of device pointers"""
        if self._pointers is None:
            n = len(self.dims) - 1
            self._pointers = (n, (ctypes.c_void_p * n)(*[w.data_ptr() for w in self.ws]),
                              (ctypes.c_void_p * n)(*[b.data_ptr() for b in self.bs]))
        return self._pointers


def one_row_head(mlp, pack=False):
    """-> OneRowHead of a FusedMLP.  pack: build the packed image now (otherwise on the first `pack()`)"""
    ws = [l.weight.detach().contiguous() for l in mlp.layers]
    bs = [l.bias.detach().contiguous() for l in mlp.layers]
    ws[-1], bs[-1] = ws[-1][0:1].contiguous(), bs[-1][0:1].contiguous()
    head = OneRowHead(list(mlp.dims[:-1]) + [1], ws, bs)
    if pack:
        head.pack()
    return head


# ---------------------------------------------------------------------------------------------------------------- evaluation
def _field(enc):
    return enc.cfg, enc.lattice_values.detach(), enc.scale_factor, enc.random_shift_per_level.detach()


def scalar_only(enc, head, points, window):
    """channel 0 of the net at points [N, P] -> [1, N]: the lattice kernel, then the MLP with the 1-row head (packed here unless
    it is already)"""
    cfg, lat, sf, sh = _field(enc)
    feat = encode_forward_raw(cfg, points, lat, sf, sh, window)
    return mlp_forward_raw(head.dims, feat, head.pack())


def masked_sdf(enc, window, dims, packed, pts, skip=None, out=None, feat_buf=None):
    """SDF channel of the net at `pts` -> (feat [C, N], sdf [1, N]).  Two launches: the level-major encode kernel keeps one 2-MiB
    table at a time in every XCD's L2 and runs at full occupancy, which beats the single fused launch (csrc/fused.hip, whose 24
    tables thrash the L2) even more clearly at 24 levels; both honour the per-point mask `skip` [N] (masked points: no gathers
    and their entries of `out` / `feat_buf` stay; fully masked 32-sample tiles: no MLP)."""
    cfg, lat, sf, sh = _field(enc)
    feat = encode_forward_raw(cfg, pts, lat, sf, sh, window, skip=skip, out=feat_buf)
    return feat, mlp_forward_raw(dims, feat, packed, skip=skip, out=out)


def masked_sdf_gradient(enc, window, head, pts, feat, skip, out=None, d_feat=None, scratch=False):
    """analytic d sdf / d x = encode_backward_positions( mlp_backward_dX( 1 ) ) at the points of pts [N, P] that `skip` [N] does
    not mask -> [N, P]; feat [C, N]: their features.  The position backward ACCUMULATES: `out` (default: a fresh zero tensor)
    must hold zeros where a gradient is wanted; d_feat: a [C, N] buffer for the feature gradient.  scratch: the level groups of
    the position backward meet in a scratch buffer of this call, in group order, instead of in float atomics -- the same bits
    on every replay of a captured trace."""
    cfg, lat, sf, sh = _field(enc)
    N, dev = pts.shape[0], pts.device
    n_layers, Wp, Bp = head.pointers()
    if d_feat is None:
        d_feat = torch.empty_like(feat)
    gy = torch.ones((1, N), dtype=torch.float32, device=dev)
    L.call("psdf_mlp_backward_data_masked", L.c_i(n_layers), _dims_array(head.dims), L.c_l(N), L.ptr(feat), Wp, Bp, L.ptr(gy),
           L.ptr(skip), L.ptr(d_feat), L.stream())
    if out is None:
        out = torch.zeros((N, cfg.pos_dim), dtype=torch.float32, device=dev)
    args = (*_head(cfg, N), L.ptr(pts), L.ptr(lat), L.ptr(sf), L.ptr(sh), L.ptr(window), *_tail(cfg), L.ptr(d_feat), L.ptr(skip),
            L.ptr(out))
    if scratch:
        fn = L.lib().psdf_encode_backward_positions_workspace_bytes
        fn.restype = ctypes.c_int64
        nbytes = int(fn(L.c_i(cfg.pos_dim), L.c_i(cfg.nr_feat), L.c_l(N), L.c_i(cfg.nr_levels), L.c_i(int(cfg.concat_mode))))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes > 0 else None
        L.call("psdf_encode_backward_positions_masked_ws", *args, L.ptr(ws), L.c_l(nbytes), L.stream())
    else:
        L.call("psdf_encode_backward_positions_masked", *args, L.stream())
    return out


# ---------------------------------------------------------------------------------------------------------------- raw passes
def raw(enc):
    """(cfg, lattice, scale factors, shifts, touched-rows record) of an encoding as the raw kernels take them.  Kept on the module:
    a step asks 17 times, and every ask is five nn.Module attribute lookups and two detach() calls on the host -- the step is host
    bound at iteration 0 (tools/prof_step.py).  Rebuilt when the parameter's storage has moved (.to(), load of a new tensor) or the
    touched-rows record was replaced."""
    lat = enc._parameters["lattice_values"]
    r = enc.__dict__.get("_psdf_raw")
    if r is None or r[5] != lat.data_ptr() or r[4] is not enc.__dict__.get("touched_rows"):
        r = (enc.cfg, lat.detach(), enc.scale_factor, enc.random_shift_per_level.detach(), enc.__dict__.get("touched_rows"),
             lat.data_ptr())
        enc.__dict__["_psdf_raw"] = r
    return r


def enc_forward(enc, pts, win, train=True, out=None):
    """train=False: the lattice is read and no row is marked (an encoding without a touched-rows record can be evaluated so)"""
    cfg, lat, sf, sh, tr, _ = raw(enc)
    if not train:
        return encode_forward_raw(cfg, pts, lat, sf, sh, win, out=out)
    return encode_forward_raw(cfg, pts, lat, sf, sh, win, out=out, touched=tr.touched if train else None,
                              block_rows_log2=tr.block_rows_log2)


def enc_backward(enc, pts, win, g_fm, want_pos=False, want_lattice=True, zeroed=None):
    """lattice gradient into the encoding's persistent buffer; optionally the position gradient [N, P] (the kernels accumulate:
    `zeroed` = a zero-filled [N, P] tensor to use for it, else one is filled here)"""
    g_pos = (zeroed if zeroed is not None else torch.zeros_like(pts)) if want_pos else None
    cfg, lat, sf, sh, tr, _ = raw(enc)
    encode_backward_raw(cfg, pts, lat, sf, sh, win, g_fm, tr.grad if want_lattice else None, g_pos)
    return g_pos


def enc_double_gather(enc, pts, win, dd_pos, g_fm):
    """backward of the position gradient, first half: the gradient w.r.t. the feature gradient [C, N] (a gather)"""
    gg = torch.empty_like(g_fm)
    cfg, lat, sf, sh, _, _ = raw(enc)
    encode_double_backward_raw(cfg, pts, lat, sf, sh, win, dd_pos, g_fm, None, gg)
    return gg


def enc_double_scatter(enc, pts, win, dd_pos, g_fm, direct_fm):
    """second half, together with the plain backward of `direct_fm` (the gradient that reached the features): ONE scatter of both
    into the lattice buffer -- they land on the same rows of the same simplices"""
    cfg, lat, sf, sh, tr, _ = raw(enc)
    encode_double_backward_raw(cfg, pts, lat, sf, sh, win, dd_pos, g_fm, tr.grad, None, direct_fm)


def net_params(mlp):
    """(dims, layers, weights, biases) of an MLP module as the raw kernels take them"""
    layers = list(mlp.layers)
    return mlp.dims, layers, [l.weight for l in layers], [l.bias for l in layers]


def set_grads(layers, dWs, dbs):
    for l, dW, db in zip(layers, dWs, dbs):
        l.weight.grad, l.bias.grad = dW, db


def sdf_gradient(enc, feat, pts, net, zeroed=None):
    """n = d sdf / d p and the feature gradient it came through, for the SDF network (encoding `enc`, MLP `net`: a record with
    dims, ws, bs, win) evaluated at pts with features feat -> (n [N, P], dfeat [C, N], e0).  zeroed: a zero-filled [N, P] tensor
    for n (one is filled here otherwise)"""
    e0 = None       # "the unit gradient of output 0": the kernels take NULL for it (no [33, N] tensor that is 1 in one row)
    dfeat, _, _ = mlp_backward_raw(net.dims, feat, net.ws, net.bs, e0, need_dx=True, need_dw=False)
    n = enc_backward(enc, pts, net.win, dfeat, want_pos=True, want_lattice=False, zeroed=zeroed)
    return n, dfeat, e0


def sdf_gradient_backward(enc, mlp_module, g_n, feat, dfeat, e0, pts, net, extra_dfeat=None, extra_gy=None, zeroed=None):
    """backward of  n = d sdf / d p  for an upstream g_n [N, P]: lattice and parameter gradients are accumulated (into the
    encoding's touched-rows buffer and net.gb); returns the position gradient when `zeroed`, a zero-filled [N, P] tensor for it,
    is given (the shifted points of the curvature term depend on n).  extra_gy [33, N]: an upstream gradient of the net's outputs
    on the same samples -- its plain backward rides in the double backward's launch (round 6: one forward recomputation and one
    sweep for both); extra_dfeat: a data gradient to add instead (the two-launch form)"""
    win = net.win
    gg = enc_double_gather(enc, pts, win, g_n, dfeat)
    dX2, _, _ = mlp_double_backward(net.dims, feat, net.ws, net.bs, e0, gg, into=(net.gb.dWs, net.gb.dbs), module=mlp_module,
                                    gy2_fm=extra_gy)
    if extra_dfeat is not None:
        dX2 = dX2 + extra_dfeat
    enc_double_scatter(enc, pts, win, g_n, dfeat, dX2)
    return enc_backward(enc, pts, win, dX2, want_pos=True, want_lattice=False, zeroed=zeroed) if zeroed is not None else None
