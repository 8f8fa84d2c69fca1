"""The float64 evaluator of the Lipschitz weight normalisation (oracle/lipshitz_float64.py) WITHOUT any kernel:

  * its values equal torch float64 autograd of the reference's expression (clamp(softplus(c) / sum |W_row|, max=1), the tie
    included), to a millionth of the bar;
  * the cap on exclusions holds on the committed families (oracle/lipshitz_cases.py): no `edge` row anywhere but the planted rows of
    `near_edge`, every other row at least 1e-3 from the branch (`ties`: exact sums instead, no edge row, the tie row active);
  * the bars admit an fp32 numpy emulation of the kernels' summation order (lane loop, six butterfly steps, one atomic per active
    row) and CPU fp32 torch autograd of the reference's expression, entry by entry;
  * the bars BITE: per family, the share of non-zero entries whose bar is below 1e-3 of the entry stays above a floor taken from what
    the evaluator gives on these inputs (printed with -s, recorded in LABNOTES.md);
  * the check can fail: six mutants of the emulation are rejected.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import lipshitz_cases as lc
from oracle import lipshitz_float64 as l64

PREFILL_SHARE = 0.75       # the pre-filled dc0 is this share of what the rows add (comparable, as the GPU test's)
ALL = [(f, o, i) for f in lc.FAMILIES for (o, i) in lc.SHAPES]
f32 = np.float32


def all_cases(family, o, i):
    return lc.cases(family, o, i)


# ------------------------------------------------------------------------------------------- the reference's expression
def reference(W, c, G, dtype, rows=None):
    """torch autograd of permuto_sdf_py/models/models.py:94-100 -> Wn, dW, dc (of the rows given)"""
    w = W.to(dtype).clone().requires_grad_(True)
    cc = c.to(dtype).clone().requires_grad_(True)
    ws = w if rows is None else w[rows]
    scale = torch.clamp(F.softplus(cc) / ws.abs().sum(dim=1), max=1.0)
    wn = ws * scale[:, None]
    wn.backward(G.to(dtype) if rows is None else G.to(dtype)[rows])
    dW = w.grad if rows is None else w.grad[rows]
    return wn.detach(), dW, cc.grad


# -------------------------------------------------------------------------------- fp32 emulation of the kernels' order
def _wave_sum(x):
    """per-lane accumulation over j = lane, lane + 64, .. then the xor butterfly 32, 16, .. 1, every addition rounded to fp32"""
    acc = np.zeros(64, f32)
    for s in range(0, len(x), 64):
        ch = x[s:s + 64]
        acc[:len(ch)] = acc[:len(ch)] + ch
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = (acc + acc[lanes ^ o]).astype(f32)
    assert (acc == acc[0]).all() or np.isnan(acc[0])
    return acc[0]


def emulate(W, c, G, dc0=0.0, mutant=None):
    """lipshitz_norm_fwd_kernel and lipshitz_norm_bwd_kernel in numpy fp32 (expf, log1pf as correctly rounded functions).
    mutant: no_sgn | strict_lt | no_sigma | dc_overwrite | drop_tail | sgn0_one"""
    W, G = W.numpy().astype(f32), G.numpy().astype(f32)
    x = f32(c.reshape(-1)[0].item())
    n_out, n_in = W.shape
    sp = x if x > f32(20) else f32(math.log1p(float(f32(math.exp(float(x))))))
    sig = f32(1) if x > f32(20) else f32(1) / (f32(1) + f32(min(math.exp(-float(x)), 3.0e38)))
    if mutant == "no_sigma":
        sig = f32(1)
    Wn, dW, dc = np.empty_like(W), np.empty_like(W), f32(dc0)
    with np.errstate(all="ignore"):
        for r in range(n_out):
            w, g = W[r], G[r]
            aw = np.abs(w)
            a = _wave_sum(aw[:n_in - n_in % 64] if mutant == "drop_tail" else aw)
            gw = _wave_sum((g * w).astype(f32))
            ratio = f32(sp) / a
            Wn[r] = w * np.fmin(ratio, f32(1))                        # fminf: a nan ratio gives 1
            active = ratio < f32(1) if mutant == "strict_lt" else ratio <= f32(1)
            sgn = np.sign(w).astype(f32)
            if mutant == "sgn0_one":
                sgn = np.where(w == 0, f32(1), sgn)
            if not active:
                dW[r] = g
                continue
            if mutant == "no_sgn":
                dW[r] = g * ratio
            else:
                dW[r] = g * ratio - (gw * f32(sp)) / (a * a) * sgn
            term = gw / a * sig
            dc = term if mutant == "dc_overwrite" else f32(dc + term)
    return torch.from_numpy(Wn), torch.from_numpy(dW), float(dc)


# ------------------------------------------------------------------------------------------------------ the verdicts
def rows_ok(got, G, ev):
    """[out] bool: the row is inside its bars; an `edge` row as a whole inside the active arm's bars, or as a whole exactly G"""
    got = got.double()
    ok = ((got - ev["dW"]).abs() <= ev["dW_bar"]).all(dim=1)
    opened = ((got - ev["dW_open"]).abs() <= ev["dW_open_bar"]).all(dim=1)
    closed = (got == G.double()).all(dim=1)
    return torch.where(ev["edge"], opened | closed, ok)


def accepted(case, kind, fwd, ev, Wn, dW, dc):
    G = case.G[kind]
    return bool(((Wn.double() - fwd["Wn"]).abs() <= fwd["Wn_bar"]).all()) and bool(rows_ok(dW, G, ev).all()) \
        and abs(dc - ev["dc"]) <= ev["dc_bar"]


def prefill(ev):
    return float(torch.tensor(PREFILL_SHARE * float(ev["terms"][ev["active"]].abs().sum()), dtype=torch.float32))


def ratio_of(err, bar):
    k = bar > 0
    return float((err[k] / bar[k]).max()) if bool(k.any()) else 0.0


# ================================================================================================== the issue's example
def test_the_tie_is_differentiated():
    W, c, G = torch.tensor([[8.0, -8.0, 16.0]]), torch.tensor([32.0]), torch.tensor([[1.0, 2.0, 3.0]])
    fwd, ev = l64.forward(W, c), l64.backward(W, c, G)
    assert float(fwd["ratio"][0]) == 1.0 and float(fwd["E_ratio"][0]) == 0.0 and not bool(fwd["edge"].any()) and bool(ev["active"][0])
    assert torch.equal(fwd["Wn"], W.double()) and not bool(fwd["Wn_bar"].any())
    assert torch.equal(ev["dW"], torch.tensor([[-0.25, 3.25, 1.75]], dtype=torch.float64)) and ev["dc"] == 1.25
    _, dW, dc = reference(W, c, G, torch.float64)
    assert torch.equal(dW, ev["dW"]) and float(dc) == 1.25
    _, dW, dc = emulate(W, c, G)
    assert torch.equal(dW.double(), ev["dW"]) and dc == 1.25
    _, dW, dc = emulate(W, c, G, mutant="strict_lt")
    assert torch.equal(dW, G) and dc == 0.0                          # what the kernels returned before `<=`


# ============================================================================================================ values
@pytest.mark.parametrize("family,o,i", ALL)
def test_values_equal_float64_autograd(family, o, i):
    for case in all_cases(family, o, i):
        fwd = l64.forward(case.W, case.c)
        some = ~(case.W == 0).all(dim=1)           # torch differentiates 0 / 0 on an all-zero row (nan in dW AND in dc): left out
        for kind in lc.GRADS:
            G = case.G[kind]
            ev = l64.backward(case.W, case.c, G)
            if not bool(some.any()):
                assert torch.equal(ev["dW"], G.double()) and ev["dc"] == 0.0 and ev["dc_bar"] == 0.0
                continue
            wn, dW, dc = reference(case.W, case.c, G, torch.float64, None if bool(some.all()) else some)
            for name, got, ref, bar in (("Wn", wn, fwd["Wn"][some], fwd["Wn_bar"][some]), ("dW", dW, ev["dW"][some], ev["dW_bar"][some])):
                tol = 1e-6 * bar
                assert bool(((got - ref).abs() <= tol).all()), "%s %s %s: %g" % (case.label, kind, name, float(((got - ref).abs() - tol).max()))
            assert abs(float(dc) - ev["dc"]) <= 1e-6 * ev["dc_bar"], (case.label, kind, float(dc), ev["dc"], ev["dc_bar"])
        zero = ~some
        if bool(zero.any()):                                       # the contract of the all-zero row
            assert not bool(fwd["Wn"][zero].any()) and not bool(fwd["Wn_bar"][zero].any())
            assert torch.equal(ev["dW"][zero], G.double()[zero]) and not bool(ev["dW_bar"][zero].any()) and not bool(ev["active"][zero].any())


# ============================================================================================================ the cap
def _check_cap(case):
    fwd = l64.forward(case.W, case.c)
    assert not bool((fwd["edge"] & ~case.planted).any()), case.label + ": an edge row that was not planted"
    if case.family == "ties":
        assert not bool(fwd["edge"].any())
        tie = torch.arange(case.W.shape[0]) % 3 == 0
        assert bool((fwd["ratio"][tie] == 1.0).all()) and bool(fwd["active"][tie].all()) and bool((fwd["E_ratio"][tie] == 0).all())
        A = case.W.double().abs().sum(1)
        assert set((A - 32.0).tolist()) <= {0.0, 2.0 ** -15, -2.0 ** -15}
        assert bool((fwd["ratio"] <= 1.0).eq(fwd["active"]).all())
    else:
        rest = ~case.planted
        assert bool(((fwd["ratio"][rest] - 1.0).abs() >= lc.MARGIN).all()), case.label
    return int(fwd["edge"].sum()), int(fwd["active"].sum())


@pytest.mark.parametrize("family,o,i", ALL)
def test_edge_cap(family, o, i):
    for case in all_cases(family, o, i):
        edges, active = _check_cap(case)
        n = case.W.shape[0]
        if family == "near_edge":
            assert edges <= int(case.planted.sum())
            print("%s: %d of %d planted rows are edge rows" % (case.label, edges, int(case.planted.sum())))
        else:
            assert edges == 0
        if family == "inactive":
            assert active == 0 and bool((l64.forward(case.W, case.c)["ratio"] >= 2.0 * (1 - 1e-6)).all())
        if family == "all_active":
            assert active == n
        if family in ("mixed", "soft", "zeros") and n >= 2:
            assert 0 < active < n
        if family == "mixed" and n >= 64:
            assert 0.3 <= active / n <= 0.7
            A = case.W.double().abs().sum(1)
            assert float(A.max() / A.min()) >= 30.0                  # row sums over (nearly) two decades


@pytest.mark.parametrize("name", sorted(lc.NETS))
def test_edge_cap_of_the_nets(name):
    layers = lc.net(name)
    assert len(layers) == len(lc.NETS[name]) <= l64.MAX_LAYERS
    for case in layers:
        _check_cap(case)


# ============================================================================================= correct arithmetic passes
@pytest.mark.parametrize("family,o,i", ALL)
def test_bars_admit_fp32(family, o, i):
    out = []
    for case in all_cases(family, o, i):
        fwd = l64.forward(case.W, case.c)
        some = ~(case.W == 0).all(dim=1)
        worst = {}
        for kind in lc.GRADS:
            G = case.G[kind]
            for dc0 in (0.0, None):
                ev = l64.backward(case.W, case.c, G)
                d0 = prefill(ev) if dc0 is None else 0.0
                ev = l64.backward(case.W, case.c, G, dc0=d0)
                Wn, dW, dc = emulate(case.W, case.c, G, d0)
                assert accepted(case, kind, fwd, ev, Wn, dW, dc), "%s %s dc0=%r: the emulation is outside a bar" % (case.label, kind, d0)
                keep = ~ev["edge"]
                worst["Wn"] = max(worst.get("Wn", 0.0), ratio_of((Wn.double() - fwd["Wn"]).abs(), fwd["Wn_bar"]))
                worst["dW " + kind] = max(worst.get("dW " + kind, 0.0), ratio_of((dW.double() - ev["dW"]).abs()[keep], ev["dW_bar"][keep]))
                worst["dc " + kind] = max(worst.get("dc " + kind, 0.0), abs(dc - ev["dc"]) / max(ev["dc_bar"], 1e-300))
            # CPU fp32 torch of the reference's expression (rows that are not all zero: torch returns nan there)
            if bool(some.any()):
                ev = l64.backward(case.W, case.c, G)
                wn, dW, dc = reference(case.W, case.c, G, torch.float32, None if bool(some.all()) else some)
                assert bool(((wn.double() - fwd["Wn"][some]).abs() <= fwd["Wn_bar"][some]).all()), case.label + " torch fp32 Wn"
                sub = {k: (v[some] if torch.is_tensor(v) else v) for k, v in ev.items()}
                assert bool(rows_ok(dW, G[some], sub).all()), "%s %s: torch fp32 dW" % (case.label, kind)
                assert abs(float(dc) - ev["dc"]) <= ev["dc_bar"], "%s %s: torch fp32 dc %r, float64 %r, bar %r" % (
                    case.label, kind, float(dc), ev["dc"], ev["dc_bar"])
        out.append("%s: " % case.label + ", ".join("%s %.3f" % kv for kv in sorted(worst.items())))
    print("emulation, worst error / bar\n  " + "\n  ".join(out))


# ============================================================================================================= bites
# Floors from what the evaluator gives on the committed inputs (LABNOTES.md has the figures).  Wn and every dW: 0.999 or more in every
# family (a row's bar is a few u of its entries; the orthogonal G cancels in gw, not in dW = g ratio - ..).  dc is ONE number per
# case, seven or 56 per family: a case whose sum of row terms cancels to below 1e-3 of sum |t| costs 1 / 7 (mixed, ties: 0.857).
# No floor where the value is ill conditioned by construction: dc under the orthogonal G (gw ~ 0: 86-100 % saturated), dc of
# `near_edge` (the planted rows' terms widen the bar) and of `inactive` (nothing is added: dc = 0, bar 0).
_DW = {"Wn": 0.99, "dW ordinary": 0.99, "dW small": 0.99, "dW orthogonal": 0.99}
BITE_FLOOR = {
    "inactive": dict(_DW),
    "mixed": dict(_DW, **{"dc ordinary": 0.85, "dc small": 0.85}),
    "all_active": dict(_DW, **{"dc ordinary": 0.99, "dc small": 0.99}),
    "soft": dict(_DW, **{"dc ordinary": 0.95, "dc small": 0.95}),
    "zeros": dict(_DW, **{"dc ordinary": 0.99, "dc small": 0.99}),
    "ties": dict(_DW, **{"dc ordinary": 0.85, "dc small": 0.85}),
    "near_edge": dict(_DW),
}


@pytest.mark.parametrize("family", lc.FAMILIES)
def test_bars_bite(family):
    refs, bars = {}, {}

    def put(key, ref, bar):
        refs.setdefault(key, []).append(ref.reshape(-1))
        bars.setdefault(key, []).append(bar.reshape(-1))
    for (o, i) in lc.SHAPES:
        for case in all_cases(family, o, i):
            fwd = l64.forward(case.W, case.c)
            put("Wn", fwd["Wn"], fwd["Wn_bar"])
            for kind in lc.GRADS:
                ev = l64.backward(case.W, case.c, case.G[kind])
                keep = ~ev["edge"]
                put("dW " + kind, ev["dW"][keep], ev["dW_bar"][keep])
                put("dc " + kind, torch.tensor([ev["dc"]], dtype=torch.float64), torch.tensor([ev["dc_bar"]], dtype=torch.float64))
    got = {}
    for key in sorted(refs):
        b, s = l64.bites(torch.cat(refs[key]), torch.cat(bars[key]))
        got[key] = b
        print("%s %s: bites %.3f, saturated %.3f" % (family, key, b, s))
    for key, floor in BITE_FLOOR.get(family, {}).items():
        assert got[key] >= floor, (family, key, got[key], floor)


# ================================================================================================ the check can fail
def _rejected(mutant, case, kind, prefilled=False):
    G = case.G[kind]
    fwd = l64.forward(case.W, case.c)
    ev = l64.backward(case.W, case.c, G)
    d0 = prefill(ev) if prefilled else 0.0
    ev = l64.backward(case.W, case.c, G, dc0=d0)
    assert accepted(case, kind, fwd, ev, *emulate(case.W, case.c, G, d0)), "the unchanged emulation must pass"
    return not accepted(case, kind, fwd, ev, *emulate(case.W, case.c, G, d0, mutant=mutant))


SOFT_BELOW = [k for k, c in enumerate(lc.SOFT_C) if c <= 5.0]       # sigma(c) <= 0.9933: leaving it out moves dc by >= 0.7 %


@pytest.mark.parametrize("o,i", lc.SHAPES)
def test_mutants_are_rejected(o, i):
    one = lambda family: lc.cases(family, o, i)[0]
    soft = lc.cases("soft", o, i)
    for kind in ("ordinary", "small"):
        for family in ("mixed", "all_active", "ties", "zeros") if o > 1 else ("mixed", "all_active", "ties"):
            assert _rejected("no_sgn", one(family), kind), (family, kind)
        assert _rejected("strict_lt", one("ties"), kind), kind
        for k in SOFT_BELOW:
            assert _rejected("no_sigma", soft[k], kind), (lc.SOFT_C[k], kind)
        for family in ("mixed", "all_active", "ties"):
            assert _rejected("dc_overwrite", one(family), kind, prefilled=True), (family, kind)
        if i % 64:
            for family in ("mixed", "all_active"):
                assert _rejected("drop_tail", one(family), kind), (family, kind)
        if o > 1 and i > 1:
            assert _rejected("sgn0_one", one("zeros"), kind), kind
    # the orthogonal gradient: gw ~ 0, so only what does not hang on gw can show
    if i % 64 and i > 1:
        assert _rejected("drop_tail", one("all_active"), "orthogonal")
