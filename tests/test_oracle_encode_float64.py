"""CPU: the float64 evaluator of the encoding's five linear maps (oracle/encode_float64.py) is pinned against the fp32
restatement's own autograd (oracle/permuto_oracle.py), which every older encoding test trusts:

  * the closed-form Jacobian d bary / d pos against float64 autograd of ``po.simplex`` on the points whose float64 simplex IS
    the fp32 one (elsewhere float64 describes another simplex and is no reference);
  * forward, lattice gradient, position gradient, double backward (gathered, scattered, scattered with a direct gradient
    riding along) against ``po.encode`` + autograd (``create_graph=True`` for the double backward), for the four kernel
    instantiations, both concatenation layouts, a closed level and a fractional window.

Bar: the evaluator's own per-entry bound ``(m + r) u sum|t| + m 2^-126`` (oracle/encode_float64.error_bar) with r = the
roundings autograd spends on one term: 2 for the forward and the lattice scatter (``bary * w``, ``* lat`` or ``* g``), 6 on
the Jacobian chain (``fv * g``, ``* w``, the difference of two barycentric slots is a sum, ``* 1/(P+1)`` rounded once in the
forward's mixed float64 expression and once on the way back, ``* i``, ``* sf``).  Nothing here is tuned to a measured figure;
the measured worst error / bar is printed.
"""
import numpy as np
import pytest
import torch

from oracle import encode_float64 as e64
from oracle import permuto_oracle as po

CASES = [(3, 2), (4, 2), (2, 2), (3, 4)]
R_SCATTER, R_JACOBIAN = 2, 6


def setup(P, F, layout, L=6, T=5000, N=1500, seed=1):
    torch.manual_seed(seed + 10 * P + F)
    sl = np.geomspace(1.0, 1e-3, L)
    lat, sh = po.make_params(P, T, L, F, seed=seed, init_scale=1.0)
    win = torch.tensor([1.0, 1.0, 0.5, 1.0, 0.0, 0.25][:L])          # all kinds: open, fractional, closed (level 4)
    pts = torch.rand(N, P) - 0.5
    sf = po.scale_factors(sl, P)
    mode = po.concat_layout(layout != 0, layout if layout else None)
    ev = e64.Encoding64(pts, lat, sf, sh, win, mode, 1e-3)
    return sl, lat, sh, win, pts, sf, ev


def ratio(got, ref, r):
    val, mag, cnt = ref
    bar = e64.error_bar(mag, cnt, r)
    err = (got.double() - val).abs()
    assert bool((err <= bar).all()), "worst error / bar %.3g at %s" % (
        float((err / bar.clamp_min(1e-300)).max()), np.unravel_index(int((err / bar.clamp_min(1e-300)).argmax()), err.shape))
    return float((err / bar.clamp_min(1e-300)).max())


@pytest.mark.parametrize("P,F", CASES)
def test_jacobian_equals_float64_autograd_where_the_simplex_agrees(P, F):
    sl, lat, sh, win, pts, sf, ev = setup(P, F, 0)
    agree_total = 0
    for l in (0, 3, 5):
        p64 = pts.double().requires_grad_(True)
        rem64, rank64, b64 = po.simplex(p64, sh[l].double(), sf[l].double())
        rem32, rank32, _ = po.simplex(pts, sh[l], sf[l])
        same = ((rem64 == rem32) & (rank64 == rank32)).all(1)
        agree_total += int(same.sum())
        J, A, Cn = e64.jacobian(rank32, sf[l])
        assert bool((A >= J.abs() - 1e-12 * A).all()) and bool((Cn >= 1).any())
        for r in range(P + 1):
            (g,) = torch.autograd.grad(b64[:, r].sum(), p64, retain_graph=True)
            assert float((g - J[:, r])[same].abs().max()) <= 1e-12 * float(J.abs().max())
    assert agree_total > len(pts)            # the comparison is not vacuous


@pytest.mark.parametrize("layout", [0, 1, 2])
@pytest.mark.parametrize("P,F", CASES)
def test_five_maps_equal_restatement_autograd(P, F, layout):
    sl, lat, sh, win, pts, sf, ev = setup(P, F, layout)
    N, C = len(pts), ev.C
    assert C == po.output_dims(P, len(sl), F, layout != 0, layout if layout else None)
    g, g2, u = torch.randn(N, C), torch.randn(N, C), torch.randn(N, P)
    pr = pts.clone().requires_grad_(True)
    latr = lat.clone().requires_grad_(True)
    gr = g.clone().requires_grad_(True)
    out = po.encode(pr, latr, sl, sh, win, layout != 0, 1e-3, layout if layout else None)
    worst = {"forward": ratio(out.detach(), ev.forward(), R_SCATTER)}
    gp, gl = torch.autograd.grad(out, [pr, latr], gr, create_graph=True)
    worst["lattice"] = ratio(gl.detach(), ev.lattice_grad(g), R_SCATTER)
    worst["position"] = ratio(gp.detach(), ev.position_grad(g), R_JACOBIAN)
    gg, gls = torch.autograd.grad((gp * u).sum(), [gr, latr], retain_graph=True)
    worst["dbl gathered"] = ratio(gg, ev.double_backward_gathered(u), R_JACOBIAN)
    worst["dbl scattered"] = ratio(gls, ev.double_backward_scattered(u, g), R_JACOBIAN)
    (glm,) = torch.autograd.grad((gp * u).sum() + (out * g2).sum(), [latr])
    worst["dbl scattered + direct"] = ratio(glm, ev.double_backward_scattered(u, g, g2), R_JACOBIAN)
    print("P %d F %d layout %d: worst error / bar " % (P, F, layout) + ", ".join("%s %.3f" % kv for kv in worst.items()))
    # the closed level: nothing comes out of it, exactly
    fwd = ev.forward()[0]
    assert float(fwd[:, 4 * F:5 * F].abs().max()) == 0.0 and float(ev.lattice_grad(g)[0][4].abs().max()) == 0.0
    assert float(ev.double_backward_gathered(u)[2][:, 4 * F:5 * F].max()) == 0.0


def test_scatter_rows_equals_index_add():
    torch.manual_seed(0)
    rows = torch.randint(0, 50, (4000,))
    rows[:1500] = 7                                   # one crowded row
    vals = torch.randn(4000, 3, dtype=torch.float64)
    ref = torch.zeros(64, 3, dtype=torch.float64).index_add_(0, rows, vals)
    got = e64.scatter_rows(rows, vals, 64)
    assert float((got - ref).abs().max()) <= 1e-12
    assert float(got[50:].abs().max()) == 0.0
    # a row's error is relative to its own terms: one tiny contribution behind a large prefix comes out exactly
    rows2 = torch.cat([rows, torch.tensor([60])])
    vals2 = torch.cat([vals * 1e3, torch.full((1, 3), 1.2345e-10, dtype=torch.float64)])
    assert torch.equal(e64.scatter_rows(rows2, vals2, 64)[60], vals2[-1])
    assert e64.scatter_rows(rows[:0], vals[:0], 8).shape == (8, 3)
