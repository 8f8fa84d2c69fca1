"""The two kernels of csrc/sdf_fit.hip against their float64 yardsticks, ENTRY BY ENTRY, through the raw ABI.

psdf_sdf_fit_loss against tests/sdf_fit_float64.py (derived bars; tests/test_sdf_fit_host.py shows on the CPU that they admit
plain fp32 and that they bite), for P in {3, 4}, both case families, with and without the eikonal clamp, at
(n_surf, n_off) in {(0, 5), (5, 0), (1, 1), (63, 65), (257, 1000)} and one row past a full pass of the loss kernel's grid
(whatever csrc/sdf_fit_plan.h makes that).  Output buffers are pre-filled with 7.0, so an entry the kernel does not write shows;
the loss is checked from a zero and from a pre-filled accumulator; a second call gives bit-identical terms.  The one exclusion
is the evaluator's: a row whose float64 | |g| - 1 | lies within its own error bound may take either sign arm or 0 (it must fit
one of the three).  psdf_sdf_fit_batch is exact arithmetic and is checked bit for bit in tests/test_gpu_sdf_fit.py.
Every comparison prints (-s) worst error / bar."""
import pytest
import torch

from tests import sdf_fit_float64 as ev64

pytestmark = pytest.mark.gpu

WEIGHTS = ev64.REFERENCE_WEIGHTS
SHARP, SCALE = 1e2, 1.0 / 30000.0
PREFILL = 0.75
SHAPES = [(0, 5), (5, 0), (1, 1), (63, 65), (257, 1000)]


def _L():
    from permuto_sdf_amd import _lib as L
    return L


def _plan(n_surf, n_off):
    from permuto_sdf_amd import sdf_fit
    return sdf_fit.plan(n_surf, n_off)


def raw_loss(dev, P, n_surf, s, G, n, clamp, loss0, want_grad=True, want_loss=True):
    """one call of psdf_sdf_fit_loss on pre-filled outputs -> (terms [4], loss [1] or None, grad_sdf, grad_gradients)"""
    L = _L()
    N = G.shape[0]
    s, G = s.to(dev).contiguous(), G.to(dev).contiguous()
    n = n.to(dev).contiguous() if n_surf else None
    ws = torch.full((max(1, _plan(n_surf, N - n_surf)[1] // 8),), 7.0, dtype=torch.float64, device=dev)
    terms = torch.full((4,), 7.0, dtype=torch.float32, device=dev)
    loss = torch.full((1,), loss0, dtype=torch.float32, device=dev) if want_loss else None
    gs = torch.full((N,), 7.0, dtype=torch.float32, device=dev) if want_grad else None
    gg = torch.full((N, P), 7.0, dtype=torch.float32, device=dev) if want_grad else None
    L.call("psdf_sdf_fit_loss", L.c_i(P), L.c_l(n_surf), L.c_l(N - n_surf), L.ptr(s), L.ptr(G), L.ptr(n), (L.c_f * 4)(*WEIGHTS),
           L.c_f(SHARP), L.c_f(0.0 if clamp is None else clamp), L.c_f(SCALE), L.ptr(ws), L.ptr(terms), L.ptr(loss), L.ptr(gs),
           L.ptr(gg), L.stream())
    return terms, loss, gs, gg


def compare(label, dev, P, n_surf, n_off, family, clamp, seed):
    s, G, n = ev64.cases(P, n_surf, n_off, family, seed=seed)
    out = []
    for loss0 in (0.0, PREFILL):
        ev = ev64.evaluate(s, G, n, n_surf, WEIGHTS, SHARP, clamp, SCALE, loss0=loss0)
        terms, loss, gs, gg = raw_loss(dev, P, n_surf, s, G, n, clamp, loss0)
        t = terms.cpu().double()
        assert bool(torch.isfinite(t).all())
        r_terms = float(((t - ev["terms"]).abs() / ev["terms_bar"]).max())
        assert bool(((t - ev["terms"]).abs() <= ev["terms_bar"]).all()), (label, t, ev["terms"], ev["terms_bar"])
        got = float(loss.cpu().double())
        r_loss = abs(got - ev["loss"]) / ev["loss_bar"]
        assert abs(got - ev["loss"]) <= ev["loss_bar"], (label, loss0, got, ev["loss"], ev["loss_bar"])
        out.append("from %.2f: terms %.3f loss %.3f" % (loss0, r_terms, r_loss))
    # gradients (they do not depend on the accumulator): every entry written, every entry inside its bar
    g1 = gs.cpu().double()
    assert bool(torch.isfinite(g1).all()) and bool(torch.isfinite(gg).all())
    err = (g1 - ev["grad_sdf"]).abs()
    assert bool((err <= ev["grad_sdf_bar"]).all()), (label, "grad_sdf", float((err / ev["grad_sdf_bar"].clamp_min(1e-300)).max()))
    nz = ev["grad_sdf_bar"] > 0
    r_gs = float((err[nz] / ev["grad_sdf_bar"][nz]).max()) if bool(nz.any()) else 0.0
    worst, bad = ev64.check_gradients(gg, ev)
    assert not bad, (label, "grad_gradients rows outside their bars", bad[:10], gg[bad[0]].tolist(), ev["grad_gradients"][bad[0]].tolist())
    if P == 4:
        assert not bool(gg[:, 3].any()), "the time column of grad_gradients is written as 0"
    # the same call again, and without loss and gradients: the same bits
    again, _, _, _ = raw_loss(dev, P, n_surf, s, G, n, clamp, 0.0)
    bare, _, _, _ = raw_loss(dev, P, n_surf, s, G, n, clamp, 0.0, want_grad=False, want_loss=False)
    assert torch.equal(again, terms) and torch.equal(bare, terms)
    print("%s: worst error / bar: %s, grad_sdf %.3f, grad_gradients %.3f (%d of %d rows ambiguous)"
          % (label, "; ".join(out), r_gs, worst, int(ev["ambiguous"].sum()), n_surf + n_off))


@pytest.mark.parametrize("P", [3, 4])
@pytest.mark.parametrize("family", ev64.FAMILIES)
@pytest.mark.parametrize("clamp", ev64.CLAMPS)
def test_loss_kernel_entry_by_entry(dev, P, family, clamp):
    for n_surf, n_off in SHAPES:
        compare("P %d %s clamp %s %d + %d" % (P, family, clamp, n_surf, n_off), dev, P, n_surf, n_off, family, clamp, seed=5)


@pytest.mark.parametrize("P, family, clamp", [(3, "training", None), (4, "ill", 0.05)])
def test_one_row_past_a_full_pass_of_the_grid(dev, P, family, clamp):
    cap, _, pass_rows, _ = _plan(1, 10 ** 7)
    assert _plan(300, pass_rows - 300)[0] == cap and _plan(300, pass_rows + 1 - 300)[0] == cap
    compare("P %d %s clamp %s 300 + %d (one row past %d workgroups x 256)" % (P, family, clamp, pass_rows + 1 - 300, cap), dev, P, 300,
            pass_rows + 1 - 300, family, clamp, seed=6)


def test_empty_segments_and_the_wrapper(dev):
    from permuto_sdf_amd import sdf_fit
    # a mean over no rows is 0, not NaN, and the other rows' gradients do not feel it
    for n_surf, n_off in ((0, 5), (5, 0)):
        s, G, n = ev64.cases(3, n_surf, n_off, "training", seed=7)
        terms, _, gs, gg = raw_loss(dev, 3, n_surf, s, G, n, None, 0.0)
        t = terms.tolist()
        assert (t[1] == 0.0 and t[2] == 0.0) if n_surf == 0 else t[3] == 0.0
        assert bool(torch.isfinite(gs).all()) and bool(torch.isfinite(gg).all())
    # N = 0 through the wrapper: zeros, no launch; the Function's gradients are the raw call's
    loss, terms, gs, gg = sdf_fit.sdf_fit_loss_raw(torch.zeros(0, device=dev), torch.zeros(0, 3, device=dev), torch.zeros(0, 3, device=dev), 0)
    assert float(loss) == 0.0 and terms.tolist() == [0.0] * 4 and gs.numel() == 0 and gg.shape == (0, 3)
    s, G, n = (t.to(dev) for t in ev64.cases(4, 63, 65, "training", seed=8))
    raw = sdf_fit.sdf_fit_loss_raw(s, G, n, 63, eik_clamp=0.05)
    sr, Gr = s.clone().requires_grad_(True), G.clone().requires_grad_(True)
    loss, terms = sdf_fit.sdf_fit_loss(sr.view(-1, 1), Gr, n, 63, eik_clamp=0.05)
    (2.0 * loss).backward()
    assert torch.equal(loss.detach().view(1), raw[0]) and torch.equal(terms, raw[1])
    assert torch.equal(sr.grad, 2.0 * raw[2]) and torch.equal(Gr.grad, 2.0 * raw[3])
    # and the torch form of the same loss agrees to fp32 accuracy
    lt, tt = sdf_fit.sdf_fit_loss_torch(s, G, n, 63, eik_clamp=0.05)
    assert abs(float(lt) - float(loss.detach())) <= 1e-5 * abs(float(loss.detach())) and float((tt - terms).abs().max()) <= 1e-5
