"""GPU: the fused encode -> MLP forward (fused_fwd_kernel of csrc/fused.hip, through the C entry psdf_encode_mlp_forward) entry by
entry against float64, on every CASE row of its dispatch and every path of its launch.  tests/test_gpu_fused.py keeps its own
claim (the bits of the unfused fp32 pair); this file holds the kernel against references that are no HIP code of this project.

The cases, batch sizes, launch arithmetic and skip patterns: tests/fused_float64.py, asserted on the host by
tests/test_fused_cases.py.  Every case prints psdf_mlp_packed_size, the grid its N implies and `tensor ours/torch fp32/bar`; the
worst figures are in LABNOTES.md.

What is asserted in every case:
  feat   the by-product is bit-equal to psdf_encode_forward on the same arguments (all three concat modes); rows of closed
         levels are exactly 0; it lies in a sentinel-filled buffer and nothing outside [C, N] changes (appended layout: row 2L+3
         is never written).  Where the case says feat64, every entry is also held against Encoding64.forward with the derived
         bar (m + R_FWD) u sum|t| + m 2^-126 of tests/test_gpu_encode_float64.py
  Y      per entry |ours - f64| / S <= max(4 t, 5e-6) against the float64 MLP (tests/mlp_float64.py) evaluated on the kernel's
         own fp32 features: S the entry's absolute sum, t the worst figure of unmodified torch.nn fp32 on the same device,
         features and metric -- the rule for fp32-MFMA kernels of tests/test_gpu_mlp_single_wave_float64.py; no constant is
         fitted to what the kernel returns.  Y lies in a sentinel-filled buffer, nothing outside [out, N] changes, every entry
         is finite, and the call without feat returns the same bits
  mask   Y and feat start as sentinels; the columns of fully masked tiles keep them bit for bit; every column of a live tile,
         masked samples included, is held to the per-entry bar
  no launch / argument errors: the status of the C entry, with both outputs still sentinels"""
import ctypes
import functools

import pytest
import torch

from tests import fused_float64 as F
from tests.mlp_float64 import _f64_trace, _per_entry
from tests.test_gpu_encode_float64 import R_FWD, check
from tests.test_gpu_mlp_single_wave_float64 import FLOOR, SENTINEL, _guarded, _untouched

pytestmark = pytest.mark.gpu

OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -2            # csrc/psdf_common.h


def _entry(s, dims, N, pts, packed, skip, feat, y):
    """psdf_encode_mlp_forward with the test's own buffers -> status"""
    from permuto_sdf_amd import _lib as L
    from permuto_sdf_amd.mlp import _dims_array
    fn = L.lib().psdf_encode_mlp_forward
    fn.restype = ctypes.c_int
    rc = fn(L.c_l(N), L.c_i(s.cfg.nr_levels), L.c_i(s.cfg.capacity), L.ptr(pts), L.ptr(s.lat), L.ptr(s.sf), L.ptr(s.sh),
            L.ptr(s.win), L.c_i(int(s.cfg.concat_mode)), L.c_f(s.cfg.points_scaling), L.c_i(len(dims) - 1), _dims_array(dims),
            L.ptr(packed), L.ptr(skip), L.ptr(feat), L.ptr(y), L.stream())
    torch.cuda.synchronize()
    return int(rc)


class _Conventions:
    def __init__(self, kw):
        self.kw = kw

    def __enter__(self):
        if self.kw:
            from permuto_sdf_amd import conventions
            conventions.set(**self.kw)

    def __exit__(self, *exc):
        if self.kw:
            from permuto_sdf_amd import conventions
            conventions.reset()


def _describe(case):
    from permuto_sdf_amd.mlp import packed_size
    g = F.fused_launch(case.N)
    return "fused %r: psdf_mlp_packed_size %d B (staged in LDS: %d B), grid %d x 4 waves over %d tiles (at most %d per wave, " \
           "last tile %d samples)" % (case, 4 * packed_size(list(case.dims)), 4 * F.packed_floats(case.dims), g["workgroups"],
                                      g["tiles"], g["most"], g["last"])


@functools.lru_cache(maxsize=2)
def _reference(case):
    """the case on the device, one unmasked call of the kernel (feat and Y in guarded buffers), the unfused encoding of the same
    arguments, the float64 MLP on the kernel's own features with every entry's absolute sum, and the figure t of unmodified
    torch.nn fp32; shared by the unmasked test and every skip pattern of the case and never written to"""
    from permuto_sdf_amd.encoding import encode_forward_raw
    from permuto_sdf_amd.mlp import pack_params
    dev = torch.device("cuda:0")
    dims, N = list(case.dims), case.N
    s = F.make_setup(dev, case)
    pts = s.points(case.points, N)
    lin = [l.to(dev) for l in case.net()]
    packed = pack_params(dims, [l.weight for l in lin], [l.bias for l in lin])
    with _Conventions(case.conv):
        unfused = encode_forward_raw(s.cfg, pts, s.lat, s.sf, s.sh, s.win)
        feat_flat, feat = _guarded(dims[0], N, dev)
        y_flat, y = _guarded(dims[-1], N, dev)
        rc = _entry(s, dims, N, pts, packed, None, feat, y)
        y2_flat, y2 = _guarded(dims[-1], N, dev)
        rc2 = _entry(s, dims, N, pts, packed, None, None, y2)
    x = feat.t().contiguous()
    with torch.no_grad():
        y64, SY, _, _, _, _ = _f64_trace(lin, x, torch.zeros(N, dims[-1], device=dev))
        h = x
        for i, l in enumerate(lin):
            h = l(h)
            if i < len(lin) - 1:
                h = torch.nn.functional.gelu(h)
    t = _per_entry(h, y64, SY)[0]
    return {"s": s, "pts": pts, "packed": packed, "unfused": unfused, "rc": (rc, rc2), "feat": feat, "feat_flat": feat_flat,
            "y": y, "y_flat": y_flat, "y2": y2, "y2_flat": y2_flat, "y64": y64, "SY": SY, "t": t}


def _hold_y(label, y, ref, failures, only=None):
    y64, SY = ref["y64"], ref["SY"]
    got = y.t()
    if only is not None:
        got, y64, SY = got[only], y64[only], SY[only]
    if not bool(torch.isfinite(got).all()):
        failures.append((label, "Y not finite"))
        return
    e, bad = _per_entry(got, y64, SY)
    bar = max(4 * ref["t"], FLOOR)
    print("fused %s, per entry (ours/torch fp32/bar): Y %.1e/%.1e/%.1e" % (label, e, ref["t"], bar))
    if bad:
        failures.append((label, "an entry without terms is not zero"))
    if not e <= bar:
        failures.append((label, "Y", e, bar))


def _closed_rows(s):
    rows = []
    for l in range(s.L):
        if float(s.win[l]) == 0.0:
            rows += [2 * l, 2 * l + 1]
    return rows


@pytest.mark.parametrize("case", F.CASES, ids=repr)
def test_forward_per_entry(dev, case):
    print(_describe(case))
    ref = _reference(case)
    s, failures, label = ref["s"], [], repr(case)
    assert ref["rc"] == (OK, OK), ref["rc"]
    # feat: the bits of the unfused encoding, closed levels exactly 0, nothing outside [C, N]
    assert ref["unfused"].shape == ref["feat"].shape == (s.C, case.N)
    if not torch.equal(ref["feat"].view(torch.int32), ref["unfused"].view(torch.int32)):
        d = ref["feat"] != ref["unfused"]
        failures.append(("feat differs from psdf_encode_forward", int(d.sum()), d.nonzero()[:4].tolist()))
    if not _untouched(ref["feat_flat"]):
        failures.append("feat: written beyond [C, N]")
    closed = _closed_rows(s)
    assert closed, "the window closes no level: this case checks less than it says"
    if float(ref["feat"][closed].abs().max()) != 0.0:
        failures.append("a row of a closed level is not 0")
    if case.feat64:
        check("fused feat " + label, ref["feat"].t(), s.evaluator(ref["pts"]).forward(), R_FWD)
    # Y
    if not _untouched(ref["y_flat"]) or not _untouched(ref["y2_flat"]):
        failures.append("Y: written beyond [out, N]")
    if not torch.equal(ref["y"].view(torch.int32), ref["y2"].view(torch.int32)):
        failures.append("Y of the call without feat differs")
    _hold_y(label, ref["y"], ref, failures)
    assert not failures, (case, failures)


@pytest.mark.parametrize("case", F.MASK_CASES, ids=repr)
def test_skip_masks(dev, case):
    print(_describe(case))
    ref = _reference(case)
    s, failures, N, dims = ref["s"], [], case.N, list(case.dims)
    assert ref["rc"] == (OK, OK), ref["rc"]
    for pattern in (F.FUSED_MASKS_CAP if N == F.N_CAP else F.FUSED_MASKS):
        skip, skipped = F.fused_mask(N, pattern)
        skip, skipped = skip.to(dev), skipped.to(dev)
        feat_flat, feat = _guarded(dims[0], N, dev)
        y_flat, y = _guarded(dims[-1], N, dev)
        assert _entry(s, dims, N, ref["pts"], ref["packed"], skip, feat, y) == OK
        if not (_untouched(feat_flat) and _untouched(y_flat)):
            failures.append((pattern, "written beyond [C, N] or [out, N]"))
        if not bool((y[:, skipped] == SENTINEL).all()):
            failures.append((pattern, "Y: a column of a fully masked tile was written"))
        if not bool((feat[:, skipped] == SENTINEL).all()):
            failures.append((pattern, "feat: a column of a fully masked tile was written"))
        live = ~skipped
        if not bool(live.any()):
            print("fused %r masked/%s: nothing live" % (case, pattern))
            continue
        if not torch.equal(feat[:, live].view(torch.int32), ref["unfused"][:, live].view(torch.int32)):
            failures.append((pattern, "feat of a live tile differs from psdf_encode_forward"))
        _hold_y("%r masked/%s" % (case, pattern), y, ref, failures, only=live)
        # without feat: the same bits of Y, the same columns left alone
        y2_flat, y2 = _guarded(dims[-1], N, dev)
        assert _entry(s, dims, N, ref["pts"], ref["packed"], skip, None, y2) == OK
        if not (torch.equal(y2.view(torch.int32), y.view(torch.int32)) and _untouched(y2_flat)):
            failures.append((pattern, "Y of the call without feat differs"))
    assert not failures, (case, failures)


def _plain_setup(dev, levels, mode, N=97):
    case = F.FusedCase(F.BASE_ROW, N, levels=levels, mode=mode, window="open", points="uniform")
    s = F.make_setup(dev, case)
    return s, s.points("uniform", N)


@pytest.mark.parametrize("levels,mode,dims", F.NO_LAUNCH, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_shapes_without_a_launch_are_declined_with_nothing_written(dev, levels, mode, dims):
    from permuto_sdf_amd._lib import PsdfError
    from permuto_sdf_amd.fused import encode_mlp_forward_raw
    from permuto_sdf_amd.mlp import packed_size
    N, dims = 97, list(dims)
    s, pts = _plain_setup(dev, levels, mode)
    assert s.C == dims[0]
    packed = torch.zeros(packed_size(dims), dtype=torch.float32, device=dev)
    feat_flat, feat = _guarded(dims[0], N, dev)
    y_flat, y = _guarded(dims[-1], N, dev)
    assert _entry(s, dims, N, pts, packed, None, feat, y) == ERR_UNSUPPORTED
    assert bool((feat_flat == SENTINEL).all()) and bool((y_flat == SENTINEL).all())
    with pytest.raises(PsdfError):
        encode_mlp_forward_raw(s.cfg, pts, s.lat, s.sf, s.sh, s.win, dims, packed, want_feat=True, out=y)
    torch.cuda.synchronize()
    assert bool((y_flat == SENTINEL).all())


@pytest.mark.parametrize("mode", [F.NONE, F.PADDED, F.APPENDED], ids=lambda m: F.MODE_NAMES[m])
def test_argument_errors(dev, mode):
    """dims[0] != C is an argument error in every concat mode (the widths of the two other modes, and one channel off); N = 0
    with NULL pointers is OK"""
    from permuto_sdf_amd import _lib as L
    from permuto_sdf_amd.mlp import _dims_array, packed_size
    N, levels = 97, 16
    s, pts = _plain_setup(dev, levels, mode)
    C = F.channels(levels, mode)
    assert s.C == C
    for K0 in sorted({F.channels(levels, m) for m in (F.NONE, F.PADDED, F.APPENDED)} | {C - 1, C + 1}):
        dims = [K0, 64, 64, 64, 3]
        packed = torch.zeros(packed_size(dims), dtype=torch.float32, device=dev)
        feat_flat, feat = _guarded(max(K0, C), N, dev)
        y_flat, y = _guarded(3, N, dev)
        rc = _entry(s, dims, N, pts, packed, None, feat, y)
        if K0 == C:
            assert rc == OK and _untouched(y_flat) and bool((y != SENTINEL).all())
        else:
            assert rc == ERR_ARG, (K0, rc)
            assert bool((feat_flat == SENTINEL).all()) and bool((y_flat == SENTINEL).all())
    fn = L.lib().psdf_encode_mlp_forward
    fn.restype = ctypes.c_int
    rc = fn(L.c_l(0), L.c_i(levels), L.c_i(s.cfg.capacity), None, None, None, None, None, L.c_i(mode), L.c_f(1e-3), L.c_i(4),
            _dims_array([C, 64, 64, 64, 3]), None, None, None, None, L.stream())
    assert rc == OK
