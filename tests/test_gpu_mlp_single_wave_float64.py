"""GPU: the single-wave fp32-MFMA kernels -- mlp_bwd_kernel (csrc/mlp_bwd.hip) on every row of PSDF_MLP16_ROWS in every launch
form it has, and mlp_fwd_kernel (csrc/mlp.hip) on the PSDF_MLP32_ROWS rows without a split image -- entry by entry against float64.

Forms of the backward, each through its C entry, psdf_last_path(1) == 1 asserted after every call (a reroute to the wide or
split kernels fails the test):
  dwdx    psdf_mlp_backward(dX, dW)      four waves; eight for 32-wide nets from 2^17 samples on
  dw      psdf_mlp_backward(NULL, dW)
  dx      psdf_mlp_backward(dX, NULL)    no accumulators, up to 512 workgroups
  masked  psdf_mlp_backward_data_masked  the dx launch with a sample mask
The forward: psdf_mlp_forward on packed parameters, psdf_last_path(2) asserted per net against the table (fwd_path).
The cases, their batch sizes and what each does to the launch: tests/mlp_float64.py (SW_*), asserted on the host by
tests/test_mlp_single_wave_cases.py.  One float64 pass and one unmodified torch.nn fp32 pass per case, on the device, serve
all its forms.

What is asserted, for dX, every dW_l and db_l, and Y:
  per entry    |ours - f64| / S <= max(4 t, 5e-6): S the entry's own absolute sum in float64, t the worst figure of torch fp32 for
               the same tensor, inputs, device and metric -- the rule for fp32-accurate kernels of
               tests/test_gpu_mlp_baseline_numerics.py; no constant is fitted to what the kernels return
  zeros        an entry with S == 0 (the dX rows of the samples whose dY is 0, the dW_1 column of the zero pad input) is exactly 0
  bounds       every output lies inside a sentinel-filled buffer; nothing outside [K0, N], the parameter shapes or [out, N] changes
               (for ragged nets: a write into the padded rows of a 16-tile)
  forms agree  dX of (dX, NULL) and dW, db of (NULL, dW) keep their own bars; against the (dX, dW) call they are bit-equal where
               FORMS_BIT_EQUAL says that held on the first run, else within the bar of each, the worst difference printed
  mask         dX starts as a sentinel; the columns of fully masked tiles keep it bit for bit, every column of a live tile, masked
               samples included, is held to the per-entry bar
  dY == NULL   the unit gradient of output 0, data-gradient and masked form

The tails case (W_1, b_1 times 20): see test_tails_case.  Every case prints `tensor ours/torch fp32/bar`; the worst figures are
in LABNOTES.md."""
import ctypes
import functools

import pytest
import torch

from tests import mlp_float64 as M
from tests.mlp_float64 import _f64_trace, _per_entry

pytestmark = pytest.mark.gpu

SENTINEL, PAD = 1234.5, 4096
FLOOR = 5e-6
# whether the (dX, NULL) / (NULL, dW) calls returned the bits of the (dX, dW) call on the first run on the MI355X: they did, in all
# 41 / 45 comparisons (the same tile walk and MFMA order; the workgroup images are summed in a fixed order).  Asserted where True;
# where False the worst difference (in S) would be printed and held to the two bars
FORMS_BIT_EQUAL = {"dX": True, "dW": True}


def _guarded(rows, N, dev):
    """a [rows, N] view in the middle of a sentinel-filled buffer -> (the whole buffer, the view)"""
    flat = torch.full((2 * PAD + rows * N,), SENTINEL, dtype=torch.float32, device=dev)
    return flat, flat[PAD:PAD + rows * N].view(rows, N)


def _untouched(flat):
    return bool((flat[:PAD] == SENTINEL).all()) and bool((flat[-PAD:] == SENTINEL).all())


class _GuardedGrads:
    """zero-filled dW_l [d_{l+1}, d_l] and db_l [d_{l+1}] (the kernels accumulate), each with PAD sentinel floats on either
    side; every view starts on a 16-byte boundary"""

    def __init__(self, dims, dev):
        nl = len(dims) - 1
        shapes = [(dims[l + 1], dims[l]) for l in range(nl)] + [(dims[l + 1],) for l in range(nl)]
        offs, tot = [], PAD
        for s in shapes:
            n = s[0] * (s[1] if len(s) == 2 else 1)
            offs.append((tot, n))
            tot += ((n + 3) & ~3) + PAD
        self.flat = torch.full((tot,), SENTINEL, dtype=torch.float32, device=dev)
        self.inside = torch.zeros(tot, dtype=torch.bool, device=dev)
        views = []
        for (o, n), s in zip(offs, shapes):
            self.inside[o:o + n] = True
            views.append(self.flat[o:o + n].view(*s))
            views[-1].zero_()
        self.dWs, self.dbs = views[:nl], views[nl:]

    def untouched(self):
        return bool((self.flat[~self.inside] == SENTINEL).all())


def _last_path(family):
    from permuto_sdf_amd import _lib as L
    fn = L.lib().psdf_last_path
    fn.restype = ctypes.c_int
    return int(fn(L.c_i(family)))


@functools.lru_cache(maxsize=2)
def _reference(dims, N, tails=False, unit_dy=False):
    """the case on the device, its float64 pass (Y, SY, gradients, S), and the figures t of unmodified torch.nn in fp32; shared
    by every form of the case and never written to.  unit_dy: the upstream gradient is 1 for output 0 and 0 elsewhere"""
    dev = torch.device("cuda:0")
    lin, x, gy = M.sw_case(dims, N, tails)
    if unit_dy:
        gy = torch.zeros_like(gy)
        gy[:, 0] = 1.0
    lin = [l.to(dev) for l in lin]
    xd, gyd = x.to(dev), gy.to(dev)
    y64, SY, g64, s64, _, _ = _f64_trace(lin, xd, gyd)
    x32 = xd.clone().requires_grad_(True)
    h = x32
    for i, l in enumerate(lin):
        h = l(h)
        if i < len(lin) - 1:
            h = torch.nn.functional.gelu(h)
    h.backward(gyd)
    t32 = {"dX": x32.grad}
    for i, l in enumerate(lin):
        t32["dW%d" % (i + 1)], t32["db%d" % (i + 1)] = l.weight.grad, l.bias.grad
    t = {k: _per_entry(t32[k], g64[k], s64[k])[0] for k in g64}
    t["Y"] = _per_entry(h.detach(), y64, SY)[0]
    return {"dims": list(dims), "N": N, "x_fm": xd.t().contiguous(), "gy_fm": gyd.t().contiguous(),
            "ws": [l.weight.detach().contiguous() for l in lin], "bs": [l.bias.detach().contiguous() for l in lin],
            "y64": y64, "SY": SY, "g64": g64, "s64": s64, "t": t}


def _arr(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _backward(ref, form, dx, grads, monkeypatch, skip=None, dy_null=False):
    """one call of the C entry of `form`; rc 0 and the fp32-MFMA kernel (path 1) asserted"""
    from permuto_sdf_amd import _lib as L
    from permuto_sdf_amd.mlp import _dims_array
    dims, N = ref["dims"], ref["N"]
    nl = len(dims) - 1
    gy = None if dy_null else L.ptr(ref["gy_fm"])
    # the colour head's dW+dX call is the split-fp16 workgroup kernel's unless PSDF_MLP_WIDE_SPLIT=f32 (read at every call)
    if form == "dwdx" and tuple(dims) == M.SW_HEAD:
        monkeypatch.setenv("PSDF_MLP_WIDE_SPLIT", "f32")
    else:
        monkeypatch.delenv("PSDF_MLP_WIDE_SPLIT", raising=False)
    if form == "masked":
        fn = L.lib().psdf_mlp_backward_data_masked
        fn.restype = ctypes.c_int
        rc = fn(L.c_i(nl), _dims_array(dims), L.c_l(N), L.ptr(ref["x_fm"]), _arr(ref["ws"]), _arr(ref["bs"]), gy, L.ptr(skip),
                L.ptr(dx), L.stream())
    else:
        fn = L.lib().psdf_mlp_backward
        fn.restype = ctypes.c_int
        rc = fn(L.c_i(nl), _dims_array(dims), L.c_l(N), L.ptr(ref["x_fm"]), _arr(ref["ws"]), _arr(ref["bs"]), gy,
                L.ptr(dx) if form in ("dwdx", "dx") else None, _arr(grads.dWs) if grads else None,
                _arr(grads.dbs) if grads else None, L.stream())
    assert rc == 0, (dims, N, form, rc)
    assert _last_path(1) == 1, (dims, N, form, _last_path(1))
    torch.cuda.synchronize()


def _hold(label, form, got, ref, failures, only=None):
    """every tensor of `got` per entry against the float64 pass; only: a [N] mask of the samples (rows of dX) to hold"""
    rows = []
    for k, v in got.items():
        g64, S = ref["g64"][k], ref["s64"][k]
        assert v.shape == g64.shape, (label, form, k)
        if only is not None:
            v, g64, S = v[only], g64[only], S[only]
        if not bool(torch.isfinite(v).all()):
            failures.append((form, k, "not finite"))
            continue
        e, bad = _per_entry(v, g64, S)
        bar = max(4 * ref["t"][k], FLOOR)
        rows.append("%s %.1e/%.1e/%.1e" % (k, e, ref["t"][k], bar))
        if bad:
            failures.append((form, k, "an entry without terms is not zero"))
        if not e <= bar:
            failures.append((form, k, e, bar))
    print("single wave %s %s, per entry (ours/torch fp32/bar): %s" % (label, form, " ".join(rows)))


def _agree(label, form, got, full, ref, failures):
    """the results of a (dX, NULL) / (NULL, dW) call against those of the (dX, dW) call"""
    worst, equal = 0.0, True
    for k, v in got.items():
        if torch.equal(v, full[k]):
            continue
        equal = False
        S = ref["s64"][k]
        d = (v.double() - full[k].double()).abs()
        e = float(torch.where(S > 0, d / S.clamp_min(1e-300), torch.zeros_like(d)).max())
        worst = max(worst, e)
        # each holds its own bar against float64, so the two differ by at most both bars
        if not e <= 2 * max(4 * ref["t"][k], FLOOR) or bool(((S == 0) & (d != 0)).any()):
            failures.append((form, k, "differs from the dW+dX call", e))
    kind = "dX" if form == "dx" else "dW"
    print("single wave %s %s against dW+dX: %s" % (label, form, "bit-equal" if equal else "worst difference %.1e S" % worst))
    if FORMS_BIT_EQUAL[kind] and not equal:
        failures.append((form, "not the bits of the dW+dX call", worst))


def _grads_dict(grads):
    got = {}
    for i in range(len(grads.dWs)):
        got["dW%d" % (i + 1)], got["db%d" % (i + 1)] = grads.dWs[i], grads.dbs[i]
    return got


def _masked(label, ref, patterns, failures, monkeypatch, dy_null=False):
    dev, dims, N = ref["x_fm"].device, ref["dims"], ref["N"]
    stride = M.sw_launch(dims, N, "masked")["stride"]
    for pattern in patterns:
        skip, skipped = M.sw_mask(N, pattern, stride=stride)
        skip, skipped = skip.to(dev), skipped.to(dev)
        flat, dx = _guarded(dims[0], N, dev)
        _backward(ref, "masked", dx, None, monkeypatch, skip=skip, dy_null=dy_null)
        if not _untouched(flat):
            failures.append(("masked", pattern, "dX: written beyond [K0, N]"))
        if not bool((dx[:, skipped] == SENTINEL).all()):
            failures.append(("masked", pattern, "a column of a fully masked tile was written"))
        if bool((~skipped).any()):
            _hold(label, "masked/" + pattern, {"dX": dx.t()}, ref, failures, only=~skipped)
        else:
            print("single wave %s masked/%s: nothing live" % (label, pattern))


def _run_case(case, monkeypatch):
    ref = _reference(case.dims, case.N, case.tails)
    dev, dims, N = ref["x_fm"].device, ref["dims"], ref["N"]
    label, failures, full = repr(case), [], None
    for form in [f for f in M.SW_FORMS if f in case.forms]:            # dW+dX first: the others are compared with it
        if form == "masked":
            # (the tile patterns need three tiles and a partial last one)
            patterns = M.SW_MASKS if N in (65, M.SW_N_DW) else ("none", "all")
            if N == M.SW_N_DX:
                patterns = tuple(dict.fromkeys(M.SW_MASKS + M.SW_MASKS_TWO_TILES))
            _masked(label, ref, patterns, failures, monkeypatch)
            continue
        flat, dx = _guarded(dims[0], N, dev) if form != "dw" else (None, None)
        grads = _GuardedGrads(dims, dev) if form != "dx" else None
        _backward(ref, form, dx, grads, monkeypatch)
        got = {}
        if dx is not None:
            if not _untouched(flat):
                failures.append((form, "dX: written beyond [K0, N]"))
            got["dX"] = dx.t()
        if grads is not None:
            if not grads.untouched():
                failures.append((form, "dW / db: written beyond the parameter shapes"))
            got.update(_grads_dict(grads))
        _hold(label, form, got, ref, failures)
        if form == "dwdx":
            full = got
        elif full is not None:
            _agree(label, form, got, full, ref, failures)
    return failures


@pytest.mark.parametrize("case", M.SW_CASES, ids=repr)
def test_backward_per_entry_in_every_form(dev, case, monkeypatch):
    """every form the case is listed with (tests/mlp_float64.py: SW_NETS and the batch lists)"""
    failures = _run_case(case, monkeypatch)
    assert not failures, (case, failures)


def test_tails_case(dev, monkeypatch):
    """52-32-32-32-33 at N = 16 423 with W_1, b_1 times 20: pre-activations out to |z_1| > 6, where gelu' = cdf + z pdf cancels.
    Held to the plain rule like every other case."""
    failures = _run_case(M.SW_TAILS_CASE, monkeypatch)
    assert not failures, (M.SW_TAILS_CASE, failures)


@pytest.mark.parametrize("dims,form", [((35, 64, 64, 64, 3), "dx"), ((35, 64, 64, 64, 3), "masked"), (M.SW_REF, "dx")],
                         ids=lambda v: v if isinstance(v, str) else "-".join(map(str, v)))
def test_null_dy_is_the_unit_gradient_of_output_0(dev, dims, form, monkeypatch):
    """dY == NULL on a final-dot net with three outputs and on the 33-output net (MFMA output layer; its row has no masked form),
    against the float64 pass with dY = (1, 0, .., 0) per sample"""
    N = M.SW_N_DW
    ref = _reference(tuple(dims), N, False, True)
    label, failures = "%s N=%d dY=NULL" % ("-".join(map(str, dims)), N), []
    if form == "masked":
        _masked(label, ref, ("none", "every_second_tile", "last_tile"), failures, monkeypatch, dy_null=True)
    else:
        flat, dx = _guarded(dims[0], N, dev)
        _backward(ref, "dx", dx, None, monkeypatch, dy_null=True)
        assert _untouched(flat), (label, "dX: written beyond [K0, N]")
        _hold(label, "dx", {"dX": dx.t()}, ref, failures)
    assert not failures, (label, failures)


@pytest.mark.parametrize("N", M.SW_N_FWD)
@pytest.mark.parametrize("dims", M.SW_FWD_NETS, ids=lambda d: "-".join(map(str, d)))
def test_forward_per_entry(dev, dims, N):
    """psdf_mlp_forward: the fp32-MFMA kernel (path 1) on the rows without a split image -- at 131 111 samples past its cap of 1024
    workgroups, two waves on a second 32-sample tile -- and the split-bf16 kernel (path 2) on the others, to the same rule"""
    from permuto_sdf_amd.mlp import mlp_forward_raw, pack_params
    ref = _reference(tuple(dims), N)
    d = ref["dims"]
    flat, y = _guarded(d[-1], N, dev)
    mlp_forward_raw(d, ref["x_fm"], pack_params(d, ref["ws"], ref["bs"]), out=y)
    torch.cuda.synchronize()
    assert _last_path(2) == M.fwd_path(dims), (dims, _last_path(2))
    assert _untouched(flat), (dims, N, "Y: written beyond [out, N]")
    assert bool(torch.isfinite(y).all()), (dims, N)
    e, bad = _per_entry(y.t(), ref["y64"], ref["SY"])
    bar = max(4 * ref["t"]["Y"], FLOOR)
    print("single wave %s N=%d forward (path %d), per entry (ours/torch fp32/bar): Y %.1e/%.1e/%.1e"
          % ("-".join(map(str, dims)), N, _last_path(2), e, ref["t"]["Y"], bar))
    assert not bad, (dims, N, "an entry without terms is not zero")
    assert e <= bar, (dims, N, e, bar)
