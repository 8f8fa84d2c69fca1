"""The loss tails (second block of csrc/neus.hip: l1_loss, eikonal_loss, normalize3, curvature_shift, curvature_loss,
offsurface_loss, sigmoid_rows, both directions) against the float64 evaluators of oracle/tails_float64.py, ENTRY BY ENTRY, on
the families of oracle/tails_cases.py: where training runs (second normal 1e-4 away, |grad sdf| ~ 1) and where the formulas are
ill conditioned.  Bars are derived (the evaluator's docstring); tests/test_oracle_tails_float64.py shows on the CPU that they
admit plain fp32 and that they bite.  Exclusions are conditions: a curvature row whose float64 dot lies within its own E(dot) of
a clamp edge may take either arm -- inside the bar of the open arm, or exactly 0.  Nothing else.

Loss checks start from a zero accumulator (the pre-filled one is test_abi_options).  Sizes: every N of tails_cases.SIZES through
the raw ABI; L1 past one pass of its 256-workgroup grid (R C = 65 538) and several
passes with a ragged end (R = 50 001); every `stream_grid` kernel at N = 4096 * 256 + 257 (second pass of the grid-stride loop),
elementwise outputs on the first 1000, last 1000 and 1000 seeded random rows, the loss against the full float64 sum; the loss
kernels once more at three full passes (N = 3 * 4096 * 256 + 257).
Every comparison prints (-s) worst error / bar and the bites / saturated shares."""
import pytest
import torch

from oracle import tails_cases as tc
from oracle import tails_float64 as t64
from tests.float64_check import check, show

pytestmark = pytest.mark.gpu

LOSS0 = 0.0            # the loss checks start from a zero accumulator: the bar is ((m + r) u sum|t| + sum E(t)), nothing else
PREFILL = 0.75         # test_abi_options: the kernels ADD to what the accumulator holds (contributions far above ulp(0.75))
EPS_SHIFT = 1e-4


def _L():
    from permuto_sdf_amd import _lib as L
    return L


def _acc(dev, value=LOSS0):
    return torch.full((1,), value, dtype=torch.float32, device=dev)


def scalar(out, name, got, val, bar, loss0=0.0):
    """the loss against its float64 value; prints error / bar and the bar against what the KERNEL added (loss - loss0)"""
    got = float(got.detach().cpu().double().reshape(-1)[0])
    ratio = abs(got - val) / max(bar, 1e-300)
    out.append("%s %.3f (bar / |loss - loss0| %.1e)" % (name, ratio, bar / max(abs(val - loss0), 1e-300)))
    assert abs(got - val) <= bar, "%s: kernel %r, float64 %r, bar %r" % (name, got, val, bar)


# ---------------------------------------------------------------------------------------------------------- raw ABI
def raw_l1(pred, gt, mask, scale, loss, want_grad=True):
    L = _L()
    R, C = pred.shape
    g = torch.full_like(pred, 7.0) if want_grad else None
    m = None if mask is None else mask.to(torch.uint8).contiguous()
    L.call("psdf_l1_loss", L.c_l(R), L.c_i(C), L.ptr(pred), L.ptr(gt), L.ptr(m), L.c_f(scale), L.ptr(loss), L.ptr(g), L.stream())
    return g


def raw_eikonal(x, scale, loss, want_grad=True):
    L = _L()
    g = torch.full_like(x, 7.0) if want_grad else None
    L.call("psdf_eikonal_loss", L.c_l(x.shape[0]), L.ptr(x), L.c_f(scale), L.ptr(loss), L.ptr(g), L.stream())
    return g


def raw_normalize(x, gy=None):
    L = _L()
    out = torch.full_like(x, 7.0)
    L.call("psdf_normalize3", L.c_l(x.shape[0]), L.ptr(x), L.ptr(gy), L.ptr(out), L.stream())
    return out


def raw_shift(p, g, r, eps, gs=None):
    L = _L()
    out = torch.full_like(g, 7.0)
    L.call("psdf_curvature_shift", L.c_l(g.shape[0]), L.ptr(p), L.ptr(g), L.ptr(r), L.c_f(eps), L.ptr(gs), L.ptr(out), L.stream())
    return out


def raw_curvature(a, b, scale, loss, want_grad=True):
    L = _L()
    ga, gb = (torch.full_like(a, 7.0), torch.full_like(b, 7.0)) if want_grad else (None, None)
    L.call("psdf_curvature_loss", L.c_l(a.shape[0]), L.ptr(a), L.ptr(b), L.c_f(scale), L.ptr(loss), L.ptr(ga), L.ptr(gb), L.stream())
    return ga, gb


def raw_offsurface(s, sharp, scale, loss, want_grad=True):
    L = _L()
    g = torch.full_like(s, 7.0) if want_grad else None
    L.call("psdf_offsurface_loss", L.c_l(s.shape[0]), L.ptr(s), L.c_f(sharp), L.c_f(scale), L.ptr(loss), L.ptr(g), L.stream())
    return g


def check_curvature(out, name, got, ev, which, rows=None):
    """non-edge rows: inside the bar (clamped rows: bar 0, exactly 0); edge rows: the whole row inside the open arm's bar or the whole
    row exactly 0"""
    sel = (lambda t: t) if rows is None else (lambda t: t[rows])
    edge = sel(ev["edge"])
    check(out, name, got, sel(ev[which]), sel(ev[which + "_bar"]), ~edge)
    if bool(edge.any()):                                            # the arm is a decision of the ROW: all of it open, or all of it 0
        g = got.detach().cpu().double()[edge]
        is_open = ((g - sel(ev[which + "_open"])[edge]).abs() <= sel(ev[which + "_open_bar"])[edge]).all(dim=1)
        is_zero = (g == 0).all(dim=1)
        ok = is_open | is_zero
        assert bool(ok.all()), "%s: %d clamp-edge rows are neither arm as a whole" % (name, int((~ok).sum()))


# ================================================================================================================= L1
L1_CASES = [(n, c, m) for n in tc.SIZES for c, m in ((1, "random"), (3, "none"), (4, "false"))] + \
           [(5001, 3, "random"), (21846, 3, "random"), (50001, 1, "none"), (50001, 3, "random"), (50001, 4, "random")]


@pytest.mark.parametrize("R,C,mask", L1_CASES)
def test_l1_loss(dev, R, C, mask):
    pred, gt, m = tc.l1(R, C, mask)
    scale = 0.9 / (R * C)
    ev = t64.l1_loss(pred, gt, m, scale, loss0=LOSS0)
    loss = _acc(dev)
    g = raw_l1(pred.to(dev), gt.to(dev), None if m is None else m.to(dev), scale, loss)
    out = []
    scalar(out, "loss", loss, ev["loss"], ev["loss_bar"])
    assert torch.equal(g.cpu().double(), ev["grad"]), "gradient entries are exactly +-scale or 0"
    if mask == "false":
        assert float(loss) == LOSS0
    show("l1 R=%d C=%d mask=%s" % (R, C, mask), out)


# ============================================================================================================ eikonal
@pytest.mark.parametrize("N", tc.SIZES)
def test_eikonal_loss(dev, N):
    x = tc.eikonal(N)
    scale = 0.1 / N
    ev = t64.eikonal_loss(x, scale, loss0=LOSS0)
    loss = _acc(dev)
    g = raw_eikonal(x.to(dev), scale, loss)
    out = []
    scalar(out, "loss", loss, ev["loss"], ev["loss_bar"])
    check(out, "g_gradients", g, ev["grad"], ev["grad_bar"])
    show("eikonal N=%d" % N, out)


# ========================================================================================================== normalize
@pytest.mark.parametrize("N", tc.SIZES)
def test_normalize3(dev, N):
    x, gy = tc.normalize(N)
    y, Ey = t64.normalize3(x)
    gx, Egx = t64.normalize3_backward(x, gy)
    out = []
    check(out, "y", raw_normalize(x.to(dev)), y, Ey)
    check(out, "g_x", raw_normalize(x.to(dev), gy.to(dev)), gx, Egx)
    show("normalize3 N=%d" % N, out)


@pytest.mark.parametrize("N", tc.SIZES)
def test_curvature_shift(dev, N):
    p, g, r, gs = tc.shift(N)
    o, Eo = t64.curvature_shift(p, g, r, EPS_SHIFT)
    gg, Egg = t64.curvature_shift_backward(g, r, EPS_SHIFT, gs)
    out = []
    check(out, "shifted", raw_shift(p.to(dev), g.to(dev), r.to(dev), EPS_SHIFT), o, Eo)
    check(out, "g_gradients", raw_shift(None, g.to(dev), r.to(dev), EPS_SHIFT, gs.to(dev)), gg, Egg)
    show("curvature_shift N=%d" % N, out)


# ========================================================================================================== curvature
@pytest.mark.parametrize("family", ["parallel", "training", "straddle"])
@pytest.mark.parametrize("N", tc.SIZES)
def test_curvature_loss(dev, N, family):
    a, b = tc.curvature(family, N)
    scale = 0.65 / N
    ev = t64.curvature_loss(a, b, scale, loss0=LOSS0)
    share = float(ev["edge"].double().mean())
    if family in tc.EDGE_CAP and N >= 5001:
        assert share <= tc.EDGE_CAP[family]
    loss = _acc(dev)
    ga, gb = raw_curvature(a.to(dev), b.to(dev), scale, loss)
    out = ["clamp-edge rows %.1f%%, clamped %.1f%%" % (100 * share, 100 * float(ev["clamped"].double().mean()))]
    scalar(out, "loss", loss, ev["loss"], ev["loss_bar"])
    check_curvature(out, "g_a", ga, ev, "ga")
    check_curvature(out, "g_b", gb, ev, "gb")
    if family == "parallel" and N >= 64:
        rows = (torch.arange(N) >= 7) & ev["clamped"] & ~ev["edge"]
        assert float(rows[7:].double().mean()) >= 0.98               # delta <= 2e-4: 1 - dot <= 4e-7, inside the clamp
        assert not bool(ga.cpu()[rows].any()) and not bool(gb.cpu()[rows].any()), "clamped rows are exactly 0"
    show("curvature %s N=%d" % (family, N), out)


# ============================================================================================ offsurface and sigmoid
@pytest.mark.parametrize("N", tc.SIZES)
def test_offsurface_loss(dev, N):
    s = tc.offsurface(N)
    scale = 0.3 / N
    ev = t64.offsurface_loss(s, 100.0, scale, loss0=LOSS0)
    loss = _acc(dev)
    g = raw_offsurface(s.to(dev), 100.0, scale, loss)
    out = []
    scalar(out, "loss", loss, ev["loss"], ev["loss_bar"])
    check(out, "g_sdf", g, ev["grad"], ev["grad_bar"])
    show("offsurface N=%d" % N, out)


@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("N", tc.SIZES)
def test_sigmoid_rows(dev, N, C):
    from permuto_sdf_amd.neus import sigmoid_rows_backward_raw, sigmoid_rows_raw
    x, gy = tc.sigmoid(N, C)
    y64, Ey = t64.sigmoid_rows(x)
    y = sigmoid_rows_raw(x.to(dev))
    out = []
    check(out, "y", y, y64, Ey)
    gx64, Egx = t64.sigmoid_rows_backward(gy, y)                   # from the fp32 y the forward kernel returned
    check(out, "g_x", sigmoid_rows_backward_raw(gy.to(dev), y), gx64, Egx)
    show("sigmoid_rows N=%d C=%d" % (N, C), out)


# ==================================================================================== second pass of the grid-stride loop
def _rows(x, rows):
    return x[rows].contiguous()


def test_large_eikonal(dev):
    N = tc.LARGE_N
    x = tc.eikonal(N)
    scale = 0.1 / N
    ev = t64.eikonal_loss(x, scale, loss0=LOSS0)
    loss = _acc(dev)
    g = raw_eikonal(x.to(dev), scale, loss)
    rows, out = tc.sample_rows(N), []
    scalar(out, "loss", loss, ev["loss"], ev["loss_bar"])
    check(out, "g_gradients", g.cpu()[rows], ev["grad"][rows], ev["grad_bar"][rows])
    show("eikonal N=%d" % N, out)


def test_large_normalize3(dev):
    N = tc.LARGE_N
    x, gy = tc.normalize(N)
    rows, out = tc.sample_rows(N), []
    y, Ey = t64.normalize3(_rows(x, rows))
    gx, Egx = t64.normalize3_backward(_rows(x, rows), _rows(gy, rows))
    check(out, "y", raw_normalize(x.to(dev)).cpu()[rows], y, Ey)
    check(out, "g_x", raw_normalize(x.to(dev), gy.to(dev)).cpu()[rows], gx, Egx)
    show("normalize3 N=%d" % N, out)


def test_large_curvature_shift(dev):
    N = tc.LARGE_N
    p, g, r, gs = tc.shift(N)
    rows, out = tc.sample_rows(N), []
    o, Eo = t64.curvature_shift(_rows(p, rows), _rows(g, rows), _rows(r, rows), EPS_SHIFT)
    gg, Egg = t64.curvature_shift_backward(_rows(g, rows), _rows(r, rows), EPS_SHIFT, _rows(gs, rows))
    check(out, "shifted", raw_shift(p.to(dev), g.to(dev), r.to(dev), EPS_SHIFT).cpu()[rows], o, Eo)
    check(out, "g_gradients", raw_shift(None, g.to(dev), r.to(dev), EPS_SHIFT, gs.to(dev)).cpu()[rows], gg, Egg)
    show("curvature_shift N=%d" % N, out)


def test_large_curvature_loss(dev):
    N = tc.LARGE_N
    a, b = tc.curvature("training", N)
    scale = 0.65 / N
    ev = t64.curvature_loss(a, b, scale, loss0=LOSS0)
    assert float(ev["edge"].double().mean()) <= tc.EDGE_CAP["training"]
    loss = _acc(dev)
    ga, gb = raw_curvature(a.to(dev), b.to(dev), scale, loss)
    rows, out = tc.sample_rows(N), []
    scalar(out, "loss", loss, ev["loss"], ev["loss_bar"])
    check_curvature(out, "g_a", ga.cpu()[rows], ev, "ga", rows)
    check_curvature(out, "g_b", gb.cpu()[rows], ev, "gb", rows)
    show("curvature training N=%d" % N, out)


def test_large_offsurface(dev):
    N = tc.LARGE_N
    s = tc.offsurface(N)
    scale = 0.3 / N
    ev = t64.offsurface_loss(s, 100.0, scale, loss0=LOSS0)
    loss = _acc(dev)
    g = raw_offsurface(s.to(dev), 100.0, scale, loss)
    rows, out = tc.sample_rows(N), []
    scalar(out, "loss", loss, ev["loss"], ev["loss_bar"])
    check(out, "g_sdf", g.cpu()[rows], ev["grad"][rows], ev["grad_bar"][rows])
    show("offsurface N=%d" % N, out)


@pytest.mark.parametrize("kernel", ["eikonal", "curvature", "offsurface"])
def test_three_full_passes_loss(dev, kernel):
    """N = 3 * 4096 * 256 + 257: at N = 4096 * 256 + 257 the second pass holds 257 rows, 2e-4 of the sum and about the loss bar, so
    a kernel that lost it from `acc` would pass the scalar check there; here every thread accumulates three terms and a lost pass
    is a third of the loss"""
    N = tc.LARGE_N3
    out = []
    loss = _acc(dev)
    if kernel == "eikonal":
        x = tc.eikonal(N)
        ev = t64.eikonal_loss(x, 0.1 / N)
        raw_eikonal(x.to(dev), 0.1 / N, loss, False)
    elif kernel == "curvature":
        a, b = tc.curvature("training", N)
        ev = t64.curvature_loss(a, b, 0.65 / N)
        raw_curvature(a.to(dev), b.to(dev), 0.65 / N, loss, False)
    else:
        s = tc.offsurface(N)
        ev = t64.offsurface_loss(s, 100.0, 0.3 / N)
        raw_offsurface(s.to(dev), 100.0, 0.3 / N, loss, False)
    assert ev["loss_bar"] < 1e-3 * ev["loss"]
    scalar(out, "loss", loss, ev["loss"], ev["loss_bar"])
    show("%s N=%d" % (kernel, N), out)


def test_large_sigmoid_rows(dev):
    from permuto_sdf_amd.neus import sigmoid_rows_backward_raw, sigmoid_rows_raw
    N, C = tc.LARGE_N, 3
    x, gy = tc.sigmoid(N, C)
    rows, out = tc.sample_rows(N), []
    y = sigmoid_rows_raw(x.to(dev))
    y64, Ey = t64.sigmoid_rows(x[:, rows].contiguous())
    check(out, "y", y.cpu()[rows], y64, Ey)
    gx64, Egx = t64.sigmoid_rows_backward(_rows(gy, rows), _rows(y.cpu(), rows))
    check(out, "g_x", sigmoid_rows_backward_raw(gy.to(dev), y).cpu()[:, rows], gx64, Egx)
    show("sigmoid_rows N=%d C=%d" % (N, C), out)


# ======================================================================================================== ABI options
def test_abi_options(dev):
    """loss = NULL with gradients wanted, gradients NULL with the loss wanted, a pre-filled accumulator is added to, N = 0 returns OK
    and touches nothing"""
    N = 257
    d = lambda t: t.to(dev)
    out = []
    # ---- gradients only: the same entries as with a loss
    x = tc.eikonal(N)
    ev = t64.eikonal_loss(x, 0.1 / N)
    check(out, "eikonal g (loss NULL)", raw_eikonal(d(x), 0.1 / N, None), ev["grad"], ev["grad_bar"])
    a, b = tc.curvature("training", N)
    evc = t64.curvature_loss(a, b, 0.65 / N)
    ga, gb = raw_curvature(d(a), d(b), 0.65 / N, None)
    check_curvature(out, "curvature g_a (loss NULL)", ga, evc, "ga")
    check_curvature(out, "curvature g_b (loss NULL)", gb, evc, "gb")
    s = tc.offsurface(N)
    evo = t64.offsurface_loss(s, 100.0, 0.3 / N)
    check(out, "offsurface g (loss NULL)", raw_offsurface(d(s), 100.0, 0.3 / N, None), evo["grad"], evo["grad_bar"])
    pred, gt, m = tc.l1(N, 3, "random")
    evl = t64.l1_loss(pred, gt, m, 0.9 / (3 * N))
    assert torch.equal(raw_l1(d(pred), d(gt), d(m), 0.9 / (3 * N), None).cpu().double(), evl["grad"])
    # ---- loss only, from a zero accumulator
    for name, run, e in (("eikonal", lambda l: raw_eikonal(d(x), 0.1 / N, l, False), ev),
                         ("curvature", lambda l: raw_curvature(d(a), d(b), 0.65 / N, l, False), evc),
                         ("offsurface", lambda l: raw_offsurface(d(s), 100.0, 0.3 / N, l, False), evo),
                         ("l1", lambda l: raw_l1(d(pred), d(gt), d(m), 0.9 / (3 * N), l, False), evl)):
        loss = _acc(dev, 0.0)
        run(loss)
        scalar(out, name + " loss (gradients NULL)", loss, e["loss"], e["loss_bar"])
    # ---- the loss is an ACCUMULATOR: pre-filled with 0.75, scales that make what the kernel adds comparable to it (the bar then
    #      holds the roundings of the `grid` atomic additions onto |loss0| too: grid u |loss0|, oracle/tails_float64.loss_scalar)
    for name, run, e in (("eikonal", lambda l: raw_eikonal(d(x), 0.5, l, False), t64.eikonal_loss(x, 0.5, loss0=PREFILL)),
                         ("curvature", lambda l: raw_curvature(d(a), d(b), 0.05, l, False), t64.curvature_loss(a, b, 0.05, loss0=PREFILL)),
                         ("offsurface", lambda l: raw_offsurface(d(s), 100.0, 0.02, l, False), t64.offsurface_loss(s, 100.0, 0.02, loss0=PREFILL)),
                         ("l1", lambda l: raw_l1(d(pred), d(gt), d(m), 0.01, l, False), t64.l1_loss(pred, gt, m, 0.01, loss0=PREFILL))):
        assert e["loss"] - PREFILL > 0.1 and e["loss_bar"] < 1e-3 * (e["loss"] - PREFILL), name
        loss = _acc(dev, PREFILL)
        run(loss)
        scalar(out, name + " loss (added to 0.75)", loss, e["loss"], e["loss_bar"], PREFILL)
    # ---- N = 0: OK, nothing written (the outputs keep their sentinel 7, the accumulator its value)
    e3, e1 = torch.empty(0, 3, device=dev), torch.empty(0, device=dev)
    L = _L()
    loss = _acc(dev, PREFILL)
    sent = torch.full((4, 3), 7.0, device=dev)
    z = L.c_l(0)
    L.call("psdf_l1_loss", z, L.c_i(3), L.ptr(e3), L.ptr(e3), None, L.c_f(1.0), L.ptr(loss), L.ptr(sent), L.stream())
    L.call("psdf_eikonal_loss", z, L.ptr(e3), L.c_f(1.0), L.ptr(loss), L.ptr(sent), L.stream())
    L.call("psdf_normalize3", z, L.ptr(e3), None, L.ptr(sent), L.stream())
    L.call("psdf_normalize3", z, L.ptr(e3), L.ptr(e3), L.ptr(sent), L.stream())
    L.call("psdf_curvature_shift", z, L.ptr(e3), L.ptr(e3), L.ptr(e3), L.c_f(1e-4), None, L.ptr(sent), L.stream())
    L.call("psdf_curvature_shift", z, None, L.ptr(e3), L.ptr(e3), L.c_f(1e-4), L.ptr(e3), L.ptr(sent), L.stream())
    L.call("psdf_curvature_loss", z, L.ptr(e3), L.ptr(e3), L.c_f(1.0), L.ptr(loss), L.ptr(sent), L.ptr(sent), L.stream())
    L.call("psdf_offsurface_loss", z, L.ptr(e1), L.c_f(100.0), L.c_f(1.0), L.ptr(loss), L.ptr(sent), L.stream())
    L.call("psdf_sigmoid_rows", z, L.c_i(3), L.ptr(e3), L.ptr(sent), L.stream())
    L.call("psdf_sigmoid_rows_backward", z, L.c_i(3), L.ptr(e3), L.ptr(e3), L.ptr(sent), L.stream())
    assert float(loss) == PREFILL and bool((sent == 7.0).all())
    show("ABI options N=%d" % N, out)


# ================================================================================================= autograd wrappers
def test_autograd_wrappers(dev):
    """permuto_sdf_amd/neus.py: the wrappers' own scales (1 / N, 1 / (R C)) and an upstream gradient of 2.5 (one more product:
    bar 2.5 bar + u |value|)"""
    from permuto_sdf_amd import neus
    N, UP = 5001, 2.5
    d = lambda t: t.to(dev)
    out = []

    def scaled(val, bar):
        return UP * val, UP * bar + t64.U * (UP * val).abs()

    pred, gt, m = tc.l1(N, 3, "random")
    evl = t64.l1_loss(pred, gt, m, 1.0 / (3 * N))
    p = d(pred).requires_grad_(True)
    loss = neus.l1_loss(p, d(gt), d(m))
    (loss * UP).backward()
    scalar(out, "l1 loss", loss, evl["loss"], evl["loss_bar"])
    v, bar = scaled(evl["grad"], torch.zeros_like(evl["grad"]))
    check(out, "l1 g_pred", p.grad, v, bar)

    x = tc.eikonal(N)
    ev = t64.eikonal_loss(x, 1.0 / N)
    xg = d(x).requires_grad_(True)
    loss = neus.eikonal_loss(xg)
    (loss * UP).backward()
    scalar(out, "eikonal loss", loss, ev["loss"], ev["loss_bar"])
    check(out, "eikonal g", xg.grad, *scaled(ev["grad"], ev["grad_bar"]))

    a, b = tc.curvature("training", N)
    evc = t64.curvature_loss(a, b, 1.0 / N)
    ag, bg = d(a).requires_grad_(True), d(b).requires_grad_(True)
    loss = neus.curvature_loss(ag, bg)
    (loss * UP).backward()
    scalar(out, "curvature loss", loss, evc["loss"], evc["loss_bar"])
    up = dict(edge=evc["edge"])
    for k in ("ga", "gb", "ga_open", "gb_open"):
        up[k], up[k + "_bar"] = scaled(evc[k], evc[k + "_bar"])
    check_curvature(out, "curvature g_a", ag.grad, up, "ga")
    check_curvature(out, "curvature g_b", bg.grad, up, "gb")

    s = tc.offsurface(N)
    evo = t64.offsurface_loss(s, 100.0, 1.0 / N)
    sg = d(s).view(-1, 1).requires_grad_(True)
    loss = neus.offsurface_loss(sg, 100.0)
    (loss * UP).backward()
    scalar(out, "offsurface loss", loss, evo["loss"], evo["loss_bar"])
    check(out, "offsurface g", sg.grad.view(-1), *scaled(evo["grad"], evo["grad_bar"]))

    xn, gy = tc.normalize(N)
    y64, Ey = t64.normalize3(xn)
    gx64, Egx = t64.normalize3_backward(xn, gy)
    xr = d(xn).requires_grad_(True)
    y = neus.normalize3(xr)
    y.backward(d(gy))
    check(out, "normalize3 y", y, y64, Ey)
    check(out, "normalize3 g_x", xr.grad, gx64, Egx)

    pts, g, r, gs = tc.shift(N)
    o64, Eo = t64.curvature_shift(pts, g, r, EPS_SHIFT)
    gg64, Egg = t64.curvature_shift_backward(g, r, EPS_SHIFT, gs)
    gr = d(g).requires_grad_(True)
    o = neus.curvature_shift(d(pts), gr, d(r), EPS_SHIFT)
    o.backward(d(gs))
    check(out, "curvature_shift", o, o64, Eo)
    check(out, "curvature_shift g", gr.grad, gg64, Egg)
    show("autograd wrappers N=%d, upstream %.1f" % (N, UP), out)
