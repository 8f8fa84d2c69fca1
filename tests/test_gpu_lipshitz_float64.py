"""The Lipschitz weight normalisation of the colour network (lipshitz_norm_fwd_kernel, lipshitz_norm_bwd_kernel and
lipshitz_norm_multi_kernel of csrc/mlp_wide.hip, through psdf_lipshitz_normalize_forward, _backward, _forward_multi and
_backward_multi) against the float64 evaluator of oracle/lipshitz_float64.py, ENTRY BY ENTRY, on the shapes and families of
oracle/lipshitz_cases.py.  Bars are derived (the evaluator's docstring); tests/test_oracle_lipshitz_float64.py shows on the CPU that
they admit correct fp32 arithmetic, that they bite and that six wrong kernels are rejected.  Exclusions are conditions: a row whose
float64 ratio lies within its own E(ratio) of 1 may take either arm AS A WHOLE -- inside the bars of the active arm, or exactly G.
Only the planted rows of `near_edge` can be such rows.  The `ties` family has none: a row whose sum is exactly softplus(c) is
differentiated, as torch's clamp(max=1) does it (the kernels decided `ratio < 1` before and returned G there).

dc is checked from zero, and once per entry from a pre-filled value comparable to what the rows add.  Every output is followed by
canaries.  Every comparison prints (-s) worst error / bar and the bites / saturated shares."""
import ctypes
import functools
import math

import pytest
import torch

from oracle import lipshitz_cases as lc
from oracle import lipshitz_float64 as l64
from tests.float64_check import check, show

pytestmark = pytest.mark.gpu

PAD, CANARY = 64, -7.25
PREFILL_SHARE = 0.75
ALL = [(f, o, i) for f in lc.FAMILIES for (o, i) in lc.SHAPES]
OK, ERR_ARG = 0, -1


def _L():
    from permuto_sdf_amd import _lib as L
    return L


def _raw(name):
    fn = getattr(_L().lib(), name)
    fn.restype = ctypes.c_int
    return fn


def _arr(ts):
    return (ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def _ints(v):
    return (ctypes.c_int * len(v))(*[int(x) for x in v])


class Guarded:
    """an output tensor followed by PAD canaries"""

    def __init__(self, shape, dev, fill=None):
        self.shape, self.n = tuple(shape), math.prod(shape)
        self.buf = torch.full((self.n + PAD,), CANARY, dtype=torch.float32, device=dev)
        if fill is not None:
            self.buf[:self.n] = fill

    @property
    def t(self):
        return self.buf[:self.n].view(self.shape)

    def cpu(self):
        assert bool((self.buf[self.n:] == CANARY).all()), "canaries after an output of shape %r were overwritten" % (self.shape,)
        return self.t.cpu()

    def untouched(self):
        return bool((self.buf == CANARY).all())


# ---------------------------------------------------------------------------------------------------------- raw ABI
def single_forward(W, c):
    L = _L()
    wn = Guarded(W.shape, W.device)
    L.call("psdf_lipshitz_normalize_forward", L.c_i(W.shape[0]), L.c_i(W.shape[1]), L.ptr(W), L.ptr(c), L.ptr(wn.buf), L.stream())
    return wn.cpu()


def single_backward(W, c, G, dc0=0.0):
    L = _L()
    dw, dc = Guarded(W.shape, W.device), Guarded((1,), W.device, dc0)
    L.call("psdf_lipshitz_normalize_backward", L.c_i(W.shape[0]), L.c_i(W.shape[1]), L.ptr(W), L.ptr(c), L.ptr(G), L.ptr(dw.buf),
           L.ptr(dc.buf), L.stream())
    return dw.cpu(), float(dc.cpu().double())


def multi_forward(Ws, cs):
    L = _L()
    n = len(Ws)
    wn = [Guarded(W.shape, W.device) for W in Ws]
    L.call("psdf_lipshitz_normalize_forward_multi", L.c_i(n), _ints([W.shape[0] for W in Ws]), _ints([W.shape[1] for W in Ws]), _arr(Ws),
           _arr(cs), _arr([o.buf for o in wn]), L.stream())
    return [o.cpu() for o in wn]


def multi_backward(Ws, cs, Gs, dc0s=None):
    L = _L()
    n = len(Ws)
    dc0s = [0.0] * n if dc0s is None else dc0s
    dw, dc = [Guarded(W.shape, W.device) for W in Ws], [Guarded((1,), W.device, d) for W, d in zip(Ws, dc0s)]
    L.call("psdf_lipshitz_normalize_backward_multi", L.c_i(n), _ints([W.shape[0] for W in Ws]), _ints([W.shape[1] for W in Ws]), _arr(Ws),
           _arr(cs), _arr(Gs), _arr([o.buf for o in dw]), _arr([o.buf for o in dc]), L.stream())
    return [o.cpu() for o in dw], [float(o.cpu().double()) for o in dc]


# ------------------------------------------------------------------------------------------------------ the verdicts
@functools.lru_cache(maxsize=None)
def evaluated(family, o, i):
    """the float64 values of every case of a family and shape, computed once and shared"""
    return tuple((case, l64.forward(case.W, case.c), {k: l64.backward(case.W, case.c, case.G[k]) for k in lc.GRADS})
                 for case in lc.cases(family, o, i))


@functools.lru_cache(maxsize=None)
def evaluated_net(name):
    return tuple((case, l64.forward(case.W, case.c), {k: l64.backward(case.W, case.c, case.G[k]) for k in lc.GRADS}) for case in lc.net(name))


def bits(t):
    return t.contiguous().view(torch.int32)


def check_Wn(out, name, got, case, fwd):
    check(out, name, got, fwd["Wn"], fwd["Wn_bar"])
    one = fwd["one"]
    assert torch.equal(bits(got)[one], bits(case.W)[one]), name + ": rows with scale 1 equal W bit for bit"


def check_dW(out, name, got, G, ev):
    edge = ev["edge"]
    check(out, name, got, ev["dW"], ev["dW_bar"], None if not bool(edge.any()) else ~edge)
    closed = ~ev["active"] & ~edge
    assert torch.equal(bits(got)[closed], bits(G)[closed]), name + ": inactive rows return G bit for bit"
    if bool(edge.any()):                                            # the arm is a decision of the ROW
        g = got.double()[edge]
        is_open = ((g - ev["dW_open"][edge]).abs() <= ev["dW_open_bar"][edge]).all(dim=1)
        is_g = (g == G.double()[edge]).all(dim=1)
        assert bool((is_open | is_g).all()), "%s: %d edge rows are neither arm as a whole" % (name, int((~(is_open | is_g)).sum()))


def check_dc(out, name, got, ev):
    ratio = abs(got - ev["dc"]) / max(ev["dc_bar"], 1e-300)
    out.append("%s %.3f (bar / |added| %.1e)" % (name, ratio if ev["dc_bar"] > 0 else 0.0, ev["dc_bar"] / max(abs(ev["dc"]), 1e-300)))
    assert math.isfinite(got) and abs(got - ev["dc"]) <= ev["dc_bar"], "%s: kernel %r, float64 %r, bar %r" % (name, got, ev["dc"], ev["dc_bar"])


def prefill(ev):
    return float(torch.tensor(PREFILL_SHARE * float(ev["terms"][ev["active"]].abs().sum()), dtype=torch.float32))


# ================================================================================ all four entries, every shape and family
@pytest.mark.parametrize("family,o,i", ALL)
def test_raw_entries(dev, family, o, i):
    for case, fwd, evs in evaluated(family, o, i):
        if family != "near_edge":
            assert not bool(fwd["edge"].any())
        W, c = case.W.to(dev), case.c.to(dev)
        out = []
        wn1, (wnm,) = single_forward(W, c), multi_forward([W], [c])
        check_Wn(out, "Wn", wn1, case, fwd)
        check_Wn(out, "Wn multi", wnm, case, fwd)
        assert torch.equal(bits(wn1), bits(wnm)), "single and multi forward differ"
        for kind in lc.GRADS:
            G, ev = case.G[kind], evs[kind]
            dw1, dc1 = single_backward(W, c, G.to(dev))
            (dwm,), (dcm,) = multi_backward([W], [c], [G.to(dev)])
            check_dW(out, "dW " + kind, dw1, G, ev)
            check_dW(out, "dW multi " + kind, dwm, G, ev)
            check_dc(out, "dc " + kind, dc1, ev)
            check_dc(out, "dc multi " + kind, dcm, ev)
            assert torch.equal(bits(dw1), bits(dwm)), "single and multi backward differ (%s)" % kind
        show(case.label, out)


# ================================================================================================================ ties
@pytest.mark.parametrize("o,i", lc.SHAPES)
def test_ties_take_the_active_arm(dev, o, i):
    """sum |W_r| = softplus(c) = 32 exactly, in every summation order: torch's clamp(max=1) differentiates the row, and so must both
    backward kernels.  No either-arm allowance: the family has no edge row."""
    ((case, fwd, evs),) = evaluated("ties", o, i)
    tie = torch.arange(o) % 3 == 0
    assert not bool(fwd["edge"].any()) and bool((fwd["ratio"][tie] == 1.0).all()) and bool(evs["ordinary"]["active"][tie].all())
    W, c = case.W.to(dev), case.c.to(dev)
    out = []
    for kind in ("ordinary", "small"):
        G, ev = case.G[kind], evs[kind]
        assert bool((ev["dW"][tie] != G.double()[tie]).any()), "the tie rows' gradient is not G"
        dw1, dc1 = single_backward(W, c, G.to(dev))
        (dwm,), (dcm,) = multi_backward([W], [c], [G.to(dev)])
        for name, dw, dc in (("single", dw1, dc1), ("multi", dwm, dcm)):
            check(out, "dW %s %s" % (name, kind), dw, ev["dW"], ev["dW_bar"])
            check(out, "dW tie rows %s %s" % (name, kind), dw[tie], ev["dW"][tie], ev["dW_bar"][tie])
            check_dc(out, "dc %s %s" % (name, kind), dc, ev)
    check_Wn(out, "Wn", single_forward(W, c), case, fwd)
    assert bool(fwd["one"][tie].all())                              # the forward is unaffected: scale 1, W bit for bit
    show(case.label, out)


# ====================================================================================================== pre-filled dc
@pytest.mark.parametrize("entry", ["single", "multi"])
def test_dc_is_accumulated(dev, entry):
    out = []
    for family, o, i in (("mixed", 64, 128), ("all_active", 7, 200), ("ties", 5, 63), ("soft", 128, 111)):
        case, fwd, evs = evaluated(family, o, i)[0]
        for kind in ("ordinary", "small"):
            G = case.G[kind]
            d0 = prefill(evs[kind])
            ev = l64.backward(case.W, case.c, G, dc0=d0)
            assert d0 != 0.0 and 0.1 < abs(d0) / float(ev["terms"][ev["active"]].abs().sum()) < 10 and ev["dc_bar"] < 1e-3 * abs(d0)
            W, c, Gd = case.W.to(dev), case.c.to(dev), G.to(dev)
            if entry == "single":
                dw, dc = single_backward(W, c, Gd, d0)
            else:
                (dw,), (dc,) = multi_backward([W], [c], [Gd], [d0])
            check_dW(out, "%s dW %s" % (case.label, kind), dw, G, ev)
            check_dc(out, "%s dc %s from %.3g" % (case.label, kind, d0), dc, ev)
    show("pre-filled dc, " + entry, out)


# =============================================================================================== the multi-layer lists
@pytest.mark.parametrize("name", sorted(lc.NETS))
def test_multi_against_single(dev, name):
    layers = evaluated_net(name)
    Ws, cs = [l[0].W.to(dev) for l in layers], [l[0].c.to(dev) for l in layers]
    out = []
    wns = multi_forward(Ws, cs)
    for l, (case, fwd, _) in enumerate(layers):
        check_Wn(out, "Wn[%d]" % l, wns[l], case, fwd)
        assert torch.equal(bits(wns[l]), bits(single_forward(Ws[l], cs[l]))), "layer %d: multi and single forward differ" % l
    for k, kind in enumerate(lc.GRADS):
        Gs = [l[0].G[kind] for l in layers]
        Gd = [g.to(dev) for g in Gs]
        d0s = [0.0] * len(layers) if k == 0 else [prefill(l[2][kind]) for l in layers]
        dws, dcs = multi_backward(Ws, cs, Gd, d0s)
        for l, (case, _, evs) in enumerate(layers):
            ev = evs[kind] if k == 0 else l64.backward(case.W, case.c, Gs[l], dc0=d0s[l])
            check_dW(out, "dW[%d] %s" % (l, kind), dws[l], Gs[l], ev)
            check_dc(out, "dc[%d] %s" % (l, kind), dcs[l], ev)
            dw1, dc1 = single_backward(Ws[l], cs[l], Gd[l], d0s[l])
            assert torch.equal(bits(dws[l]), bits(dw1)), "layer %d: multi and single backward differ (%s)" % (l, kind)
            check_dc(out, "dc[%d] single %s" % (l, kind), dc1, ev)
            # both are inside the bar around the float64 value, so they differ by two bars at the most
            assert abs(dcs[l] - dc1) <= 2 * ev["dc_bar"]
    show("net %s %s" % (name, [tuple(w.shape) for w in Ws]), out)


# ============================================================================================== arguments and empties
def test_arguments_and_empties(dev):
    L = _L()
    (case, _, _), = evaluated("mixed", 3, 64)
    W, c, G = case.W.to(dev), case.c.to(dev), case.G["ordinary"].to(dev)
    p, i_, st = L.ptr, L.c_i, L.stream()
    fwd, bwd = _raw("psdf_lipshitz_normalize_forward"), _raw("psdf_lipshitz_normalize_backward")
    fwdm, bwdm = _raw("psdf_lipshitz_normalize_forward_multi"), _raw("psdf_lipshitz_normalize_backward_multi")
    wn, dw, dc = Guarded(W.shape, dev), Guarded(W.shape, dev), Guarded((1,), dev)
    # ---- nothing to do: OK, nothing touched
    for o, i in ((0, 64), (3, 0), (0, 0), (-1, 64), (3, -5)):
        assert fwd(i_(o), i_(i), p(W), p(c), p(wn.buf), st) == OK
        assert bwd(i_(o), i_(i), p(W), p(c), p(G), p(dw.buf), p(dc.buf), st) == OK
    # ---- a NULL pointer: argument error, nothing touched
    for args in ((None, p(c), p(wn.buf)), (p(W), None, p(wn.buf)), (p(W), p(c), None)):
        assert fwd(i_(3), i_(64), *args, st) == ERR_ARG
    full = (p(W), p(c), p(G), p(dw.buf), p(dc.buf))
    for k in range(5):
        assert bwd(i_(3), i_(64), *[None if j == k else a for j, a in enumerate(full)], st) == ERR_ARG
    # ---- the multi entries
    o1, i1, Wa, ca, Ga = _ints([3]), _ints([64]), _arr([W]), _arr([c]), _arr([G])
    wna, dwa, dca = _arr([wn.buf]), _arr([dw.buf]), _arr([dc.buf])
    assert fwdm(i_(0), o1, i1, Wa, ca, wna, st) == OK and bwdm(i_(0), o1, i1, Wa, ca, Ga, dwa, dca, st) == OK
    assert fwdm(i_(0), None, None, None, None, None, st) == OK
    nine = [W] * 9
    assert fwdm(i_(9), _ints([3] * 9), _ints([64] * 9), _arr(nine), _arr([c] * 9), _arr([wn.buf] * 9), st) == ERR_ARG
    assert bwdm(i_(9), _ints([3] * 9), _ints([64] * 9), _arr(nine), _arr([c] * 9), _arr([G] * 9), _arr([dw.buf] * 9), _arr([dc.buf] * 9),
                st) == ERR_ARG
    fargs = (o1, i1, Wa, ca, wna)
    for k in range(5):
        assert fwdm(i_(1), *[None if j == k else a for j, a in enumerate(fargs)], st) == ERR_ARG
    bargs = (o1, i1, Wa, ca, Ga, dwa, dca)
    for k in range(7):
        assert bwdm(i_(1), *[None if j == k else a for j, a in enumerate(bargs)], st) == ERR_ARG
    none = _arr([None])
    for k in (2, 3, 4):                                               # a NULL entry of a pointer list
        assert fwdm(i_(1), *[none if j == k else a for j, a in enumerate(fargs)], st) == ERR_ARG
    for k in (2, 3, 4, 5, 6):
        assert bwdm(i_(1), *[none if j == k else a for j, a in enumerate(bargs)], st) == ERR_ARG
    torch.cuda.synchronize()
    assert wn.untouched() and dw.untouched() and dc.untouched()


# ======================================================================================================= Python layer
def test_single_layer_function(dev):
    """_LipshitzNormFunc under autograd, loss sum <Wn, G>: the raw entry's dW bit for bit, dc within the bar; one weight is the
    transpose of a contiguous tensor"""
    from permuto_sdf_amd.mlp import _LipshitzNormFunc
    out = []
    for family, o, i, transposed in (("mixed", 7, 200, False), ("ties", 3, 64, False), ("zeros", 5, 63, True), ("soft", 2, 65, True)):
        case, fwd, evs = evaluated(family, o, i)[0]
        G, ev = case.G["ordinary"], evs["ordinary"]
        Wd, cd, Gd = case.W.to(dev), case.c.to(dev), G.to(dev)
        if transposed:
            base = Wd.t().contiguous().requires_grad_(True)
            w = base.t()
            assert not w.is_contiguous()
        else:
            base = w = Wd.clone().requires_grad_(True)
        cc = cd.clone().requires_grad_(True)
        wn = _LipshitzNormFunc.apply(w, cc)
        (wn * Gd).sum().backward()
        got = base.grad.t() if transposed else base.grad
        dw_raw, _ = single_backward(Wd, cd, Gd)
        assert torch.equal(bits(wn.detach().cpu()), bits(single_forward(Wd, cd)))
        assert torch.equal(bits(got.cpu()), bits(dw_raw)), case.label
        check_Wn(out, case.label + " Wn", wn.detach().cpu(), case, fwd)
        check_dW(out, case.label + " dW", got.cpu(), G, ev)
        check_dc(out, case.label + " dc", float(cc.grad.cpu().double()), ev)
    show("_LipshitzNormFunc", out)


def test_all_layers_function(dev):
    """_LipshitzNormAllFunc on the colour net's shapes: layer 2 is left out of the loss (its gradient arrives as None and becomes
    zeros), layer 0 is non-contiguous"""
    from permuto_sdf_amd.mlp import _LipshitzNormAllFunc
    layers = evaluated_net("colour")
    n, skip = len(layers), 2
    Wd, cd = [l[0].W.to(dev) for l in layers], [l[0].c.to(dev) for l in layers]
    Gs = [l[0].G["ordinary"] if k != skip else torch.zeros_like(l[0].W) for k, l in enumerate(layers)]
    Gd = [g.to(dev) for g in Gs]
    base0 = Wd[0].t().contiguous().requires_grad_(True)
    ws = [base0.t()] + [w.clone().requires_grad_(True) for w in Wd[1:]]
    assert not ws[0].is_contiguous()
    cs = [c.clone().requires_grad_(True) for c in cd]
    wns = _LipshitzNormAllFunc.apply(n, *ws, *cs)
    sum((wn * g).sum() for k, (wn, g) in enumerate(zip(wns, Gd)) if k != skip).backward()
    raw_wn = multi_forward(Wd, cd)
    raw_dw, _ = multi_backward(Wd, cd, Gd)
    out = []
    for k, (case, fwd, evs) in enumerate(layers):
        got = base0.grad.t() if k == 0 else ws[k].grad
        assert torch.equal(bits(wns[k].detach().cpu()), bits(raw_wn[k])), k
        assert torch.equal(bits(got.cpu()), bits(raw_dw[k])), k
        ev = evs["ordinary"] if k != skip else l64.backward(case.W, case.c, Gs[k])
        check_dW(out, "dW[%d]" % k, got.cpu(), Gs[k], ev)
        assert cs[k].grad.shape == cs[k].shape
        check_dc(out, "dc[%d]" % k, float(cs[k].grad.cpu().double()), ev)
    assert not bool(ws[skip].grad.any()) and float(cs[skip].grad) == 0.0     # G = 0: nothing flows
    show("_LipshitzNormAllFunc", out)


def test_dc_arena(dev):
    """a caller's zero-filled dc_flat: dc_l lands at element 4 l, every other element stays zero"""
    from permuto_sdf_amd.mlp import lipshitz_normalize_all_backward_raw
    layers = evaluated_net("colour")
    n = len(layers)
    Wd, cd = [l[0].W.to(dev) for l in layers], [l[0].c.to(dev) for l in layers]
    Gd = [l[0].G["ordinary"].to(dev) for l in layers]
    arena = torch.zeros(4 * n, dtype=torch.float32, device=dev)
    dws, dcs = lipshitz_normalize_all_backward_raw(Wd, cd, Gd, dc_flat=arena)
    raw_dw, _ = multi_backward(Wd, cd, Gd)
    flat = arena.cpu()
    out = []
    for l, (case, _, evs) in enumerate(layers):
        assert dcs[l].data_ptr() == arena.data_ptr() + 16 * l and dcs[l].shape == (1,)
        assert torch.equal(bits(dws[l].cpu()), bits(raw_dw[l]))
        assert float(flat[4 * l]) != 0.0
        check_dc(out, "dc[%d]" % l, float(flat[4 * l].double()), evs["ordinary"])
    rest = torch.ones(4 * n, dtype=torch.bool)
    rest[::4] = False
    assert not bool(flat[rest].any())
    show("dc arena", out)


def test_module_forward_uses_the_normalised_weights(dev, monkeypatch):
    from permuto_sdf_amd import LipshitzMLP, mlp
    torch.manual_seed(11)
    m = LipshitzMLP(111, [128, 128, 64, 3], True).to(dev)
    with torch.no_grad():
        for c in m.lipshitz_bound_per_layer:
            c.mul_(0.35)                                              # some rows active
    seen = []
    real = mlp._FusedMLPFunc.apply

    def spy(module, x, *params):
        seen.append([p.detach().clone() for p in params[:module.n_layers]])
        return real(module, x, *params)
    monkeypatch.setattr(mlp._FusedMLPFunc, "apply", spy)
    y = m(torch.randn(256, 111, device=dev))
    assert bool(torch.isfinite(y).all()) and len(seen) == 1
    want = mlp.lipshitz_normalize_all_raw(list(m.weights_per_layer), list(m.lipshitz_bound_per_layer))
    some_active = False
    for l, (a, b) in enumerate(zip(seen[0], want)):
        assert torch.equal(bits(a.cpu()), bits(b.cpu())), l
        fwd = l64.forward(m.weights_per_layer[l].detach().cpu(), m.lipshitz_bound_per_layer[l].detach().cpu())
        out = []
        check(out, "Wn[%d]" % l, a, fwd["Wn"], fwd["Wn_bar"])
        some_active |= bool(fwd["active"].any())
        show("LipshitzMLP.forward", out)
    assert some_active
