"""AdamW (csrc/optim.hip: adamw_kernel, adamw_multi_kernel, adamw_blocks_kernel, adamw_blocks_multi_kernel) against the float64
evaluator oracle/tails_float64.adamw, ENTRY BY ENTRY and STEP BY STEP, on every launch form.

Adam (eps 1e-15) rescales every entry by its own magnitude, lattice values are ~1e-4 and lattice gradients span many decades:
the bar of an entry is derived from the roundings of the update rule (about 1e-6 of the update itself at the median,
tests/test_oracle_tails_float64.py), three orders of magnitude below the max-norm bar of tests/test_gpu_optim.py.

Every step is checked from the kernel's OWN fp32 state: the evaluator takes the fp32 p, m, v that went into the step and returns
the expected state out, p, m and v are compared per entry; five consecutive steps per case, so the moments a kernel produced feed
its next step.  Inputs: oracle/tails_cases.adam (|g|, moments log-uniform over 1e-30 ... 1e3, exact zeros).  Argument checks that
return an error without launching are asserted as error returns only.  Every comparison prints (-s) worst error / bar and the
bites / saturated shares."""
import ctypes

import pytest
import torch

from oracle import tails_cases as tc
from oracle import tails_float64 as t64
from tests.float64_check import check, show

pytestmark = pytest.mark.gpu

LR, B1, B2 = tc.ADAM_LR, tc.ADAM_BETAS[0], tc.ADAM_BETAS[1]
STEPS = 5


def _L():
    from permuto_sdf_amd import _lib as L
    return L


def raw_dense(p, g, m, v, hyper, step, lr=LR, b1=B1, b2=B2):
    L = _L()
    eps, wd, gs = hyper
    L.call("psdf_adamw_step", L.c_l(p.numel()), L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), L.c_f(lr), L.c_f(b1), L.c_f(b2), L.c_f(eps),
           L.c_f(wd), L.c_i(step), L.c_f(gs), L.stream())


def _voidp(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def raw_multi(ps, gs_, ms, vs, hyper, step, sizes=None):
    L = _L()
    eps, wd, gs = hyper
    n = len(ps)
    sizes = (ctypes.c_int64 * n)(*(sizes if sizes is not None else [p.numel() for p in ps]))
    L.call("psdf_adamw_step_multi", L.c_i(n), sizes, _voidp(ps), _voidp(gs_), _voidp(ms), _voidp(vs), L.c_f(LR), L.c_f(B1), L.c_f(B2),
           L.c_f(eps), L.c_f(wd), L.c_i(step), L.c_f(gs), L.stream())


def raw_blocks(nb, be, p, g, m, v, touched, active, lr, b1, b2, eps, step, gs, zero_grad):
    L = _L()
    L.call("psdf_adamw_step_blocks", L.c_l(nb), L.c_i(be), L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), L.ptr(touched), L.ptr(active),
           L.c_f(lr), L.c_f(b1), L.c_f(b2), L.c_f(eps), L.c_i(step), L.c_f(gs), L.c_i(zero_grad), L.stream())


def raw_blocks_multi(nbs, bes, ps, gs_, ms, vs, ts, acts, lrs, b1s, b2s, epss, steps, gs, zero_grad):
    L = _L()
    n = len(ps)
    fl = lambda xs: (ctypes.c_float * n)(*[float(x) for x in xs])
    L.call("psdf_adamw_step_blocks_multi", L.c_i(n), (ctypes.c_int64 * n)(*nbs), (ctypes.c_int * n)(*bes), _voidp(ps), _voidp(gs_),
           _voidp(ms), _voidp(vs), _voidp(ts), _voidp(acts), fl(lrs), fl(b1s), fl(b2s), fl(epss), (ctypes.c_int * n)(*steps),
           L.c_f(gs), L.c_i(zero_grad), L.stream())


def check_step(out, tag, before, g, after, hyper, step, idx=None, lr=LR, b1=B1, b2=B2):
    """before / after: (p, m, v) fp32 CPU tensors around one step with gradient g; idx: the entries to compare"""
    eps, wd, gs = hyper
    sel = (lambda t: t) if idx is None else (lambda t: t[idx])
    ev = t64.adamw(sel(before[0]), sel(g), sel(before[1]), sel(before[2]), lr, b1, b2, eps, wd, step, gs)
    for k, got in zip("pmv", after):
        check(out, "%s %s" % (tag, k), sel(got), ev[k], ev[k + "_bar"])


class Launches:
    """records the C entry points FusedAdamW.step() calls (permuto_sdf_amd.optim resolves `L.call` at call time)"""

    def __init__(self, monkeypatch):
        L = _L()
        self.names, real = [], L.call
        monkeypatch.setattr(L, "call", lambda name, *a: (self.names.append(name), real(name, *a))[1])

    def take(self):
        names, self.names[:] = [n for n in self.names if n.startswith("psdf_adamw")], []
        return names


def fresh_grad(n, family, seed):
    return tc.adam(n, family, seed)[1]


# ============================================================================================================== dense
DENSE = [(n, h, ("lattice", "randn")[(i + h) % 2], tc.ADAM_STEPS[(i + 3 * h) % 6])
         for i, n in enumerate((1, 2, 3, 4, 5, 7, 8, 1023, 1025)) for h in (0, 1)]


@pytest.mark.parametrize("n,h,family,start", DENSE)
def test_dense_every_step(dev, n, h, family, start):
    hyper = tc.ADAM_HYPER[h]
    p0, g0, m0, v0 = tc.adam(n, family, seed=start)
    p, m, v = p0.to(dev), m0.to(dev), v0.to(dev)
    out = []
    for k in range(STEPS):
        g = g0 if k == 0 else fresh_grad(n, family, 100 + k)
        before = (p.cpu(), m.cpu(), v.cpu())
        raw_dense(p, g.to(dev), m, v, hyper, start + k)
        check_step(out, "step %d" % (start + k), before, g, (p.cpu(), m.cpu(), v.cpu()), hyper, start + k)
    show("adamw dense n=%d %s eps=%g wd=%g gs=%g" % ((n, family) + hyper), out)


@pytest.mark.parametrize("h", [0, 1])
def test_dense_grid_stride_and_scalar_tail(dev, h):
    """n = 4096 * 256 * 4 + 5: the capped grid (4096 workgroups) covers 4096 * 256 * 4 entries per pass, so the second pass of
    thread 0 is one more float4 and the second pass of thread 1 is the scalar tail of 1 entry; the first 1000, the last 1000 (the
    tail and the last float4 among them) and 1000 seeded random entries are compared"""
    n = 4096 * 256 * 4 + 5
    hyper = tc.ADAM_HYPER[h]
    start = (1000, 2)[h]
    idx = tc.sample_rows(n)
    assert bool((idx >= n - 9).sum() == 9)                        # the last two float4 and the scalar tail
    p0, g0, m0, v0 = tc.adam(n, ("lattice", "randn")[h], seed=5)
    p, m, v = p0.to(dev), m0.to(dev), v0.to(dev)
    out = []
    for k in range(STEPS):
        g = g0 if k == 0 else torch.roll(g0, 7919 * k)
        before = (p.cpu(), m.cpu(), v.cpu())
        raw_dense(p, g.to(dev), m, v, hyper, start + k)
        check_step(out, "step %d" % (start + k), before, g, (p.cpu(), m.cpu(), v.cpu()), hyper, start + k, idx)
    show("adamw dense n=%d eps=%g wd=%g gs=%g" % ((n,) + hyper), out)


# ============================================================================================================== multi
MULTI_SIZES = (0, 1, 2, 3, 5, 64, 1000, 4099, 65535, 70001)


def _flat_layout(sizes):
    """16-byte aligned offsets of the tensors in one flat buffer, with a 4-float gap after each (and for a size of 0)"""
    offs, at = [], 4
    for s in sizes:
        offs.append(at)
        at += (s + 3) // 4 * 4 + 4
    return offs, at


@pytest.mark.parametrize("n_tensors,h", [(1, 0), (64, 0), (64, 1)])
def test_multi_raw(dev, n_tensors, h):
    hyper = tc.ADAM_HYPER[h]
    gen = tc.gen(77 + n_tensors)
    if n_tensors == 1:
        sizes = [4099]
    else:
        sizes = list(MULTI_SIZES) * 6 + [1, 3, 64, 0]
        sizes = [sizes[i] for i in torch.randperm(64, generator=gen).tolist()]
    offs, total = _flat_layout(sizes)
    owned = torch.zeros(total, dtype=torch.bool)
    for o, s in zip(offs, sizes):
        owned[o:o + s] = True
    start = (3, 10)[h]
    p0, g0, m0, v0 = tc.adam(total, ("lattice", "randn")[h], seed=11)
    P, M, V = p0.to(dev), m0.to(dev), v0.to(dev)
    views = lambda T: [T[o:o + max(s, 1)] for o, s in zip(offs, sizes)]     # a size of 0 still gets a valid pointer
    out = []
    for k in range(STEPS):
        g = g0 if k == 0 else torch.roll(g0, 7919 * k)
        G = g.to(dev)
        before = (P.cpu(), M.cpu(), V.cpu())
        raw_multi(views(P), views(G), views(M), views(V), hyper, start + k, sizes)
        after = (P.cpu(), M.cpu(), V.cpu())
        check_step(out, "step %d" % (start + k), before, g, after, hyper, start + k, owned)
        for a, b in zip(before, after):                             # the gaps and the tensor of size 0: bit-unchanged
            assert torch.equal(a[~owned].view(torch.int32), b[~owned].view(torch.int32))
    show("adamw multi %d tensors eps=%g wd=%g gs=%g" % ((n_tensors,) + hyper), out)


def test_multi_through_fused_adamw(dev, monkeypatch):
    """65 small parameters: two launches (64 + 1); then parameters whose step counts differ, one having skipped a step"""
    from permuto_sdf_amd.optim import FusedAdamW
    eps, wd, gs = tc.ADAM_HYPER[1]
    sizes = [(1, 2, 3, 5, 64, 257, 1000)[i % 7] for i in range(65)]
    state = [tc.adam(s, "lattice", seed=300 + i) for i, s in enumerate(sizes)]
    params = [torch.nn.Parameter(st[0].to(dev)) for st in state]
    opt = FusedAdamW(params, lr=LR, betas=(B1, B2), eps=eps, weight_decay=wd)
    launches = Launches(monkeypatch)
    out = []
    steps = [0] * 65
    for k in range(STEPS):
        grads = [fresh_grad(s, "lattice", 400 + 65 * k + i) for i, s in enumerate(sizes)]
        skip = {7} if k == 1 else set()                             # parameter 7 sits out the second step
        before = []
        for i, p in enumerate(params):
            st = opt.state.get(p) or {}
            z = torch.zeros(sizes[i])
            before.append((p.detach().cpu(), st["exp_avg"].cpu() if "exp_avg" in st else z, st["exp_avg_sq"].cpu() if "exp_avg" in st else z))
            p.grad = None if i in skip else grads[i].to(dev)
        launches.take()
        opt.step(grad_scale=gs)
        # first call: 65 parameters at one step count, 64 + 1; second: 64 (parameter 7 sits out); then parameter 7 is a step
        # behind the other 64 and gets a launch of its own.  Never the dense per-tensor entry point.
        assert launches.take() == ["psdf_adamw_step_multi"] * (1 if k == 1 else 2), "the small parameters did not take the multi launch"
        cat = lambda ts: torch.cat([t.reshape(-1) for t in ts])
        for want_step in sorted({steps[i] + 1 for i in range(65) if i not in skip}):
            ids = [i for i in range(65) if i not in skip and steps[i] + 1 == want_step]
            after = [(params[i].detach().cpu(), opt.state[params[i]]["exp_avg"].cpu(), opt.state[params[i]]["exp_avg_sq"].cpu()) for i in ids]
            check_step(out, "call %d step %d" % (k + 1, want_step), tuple(cat([before[i][j] for i in ids]) for j in range(3)),
                       cat([grads[i] for i in ids]), tuple(cat([a[j] for a in after]) for j in range(3)), (eps, wd, gs), want_step)
        for i in skip:
            assert torch.equal(before[i][0], params[i].detach().cpu())
        for i in range(65):
            steps[i] += 0 if i in skip else 1
            assert opt.state[params[i]]["step"] == steps[i]
    assert steps[7] == STEPS - 1
    show("adamw multi through FusedAdamW, 65 parameters", out)


# ============================================================================================================= blocks
def _flags(nb, seed):
    """(touched, active) per block: all four combinations, in a seeded order"""
    combos = torch.tensor([[1, 0], [0, 1], [1, 1], [0, 0]], dtype=torch.uint8)
    order = (torch.arange(nb) + seed) % 4
    return combos[order, 0].contiguous(), combos[order, 1].contiguous()


def _blocks_steps(dev, out, tag, nb, be, zero_grad, seed, launch, lr=LR, b1=B1, b2=B2, eps=1e-15, gs=1.0, start=1, state=None):
    """five steps of one blocks tensor; `launch(step, tensors)` runs the kernel over (p, g, m, v, touched, active)"""
    n = nb * be
    p0, g0, m0, v0 = tc.adam(max(n, 4), "lattice", seed=seed)
    touched0, active = _flags(max(nb, 1), seed)
    P, M, V, A = p0.to(dev), m0.to(dev), v0.to(dev), active.to(dev)
    for k in range(STEPS):
        g = torch.roll(g0, 131 * k)
        g[g == 0] = 1e-3                                            # a skipped block keeps a NON-ZERO sentinel gradient
        touched = torch.roll(touched0, k)
        G, T = g.to(dev), touched.to(dev)
        before = (P.cpu(), M.cpu(), V.cpu())
        act_before = A.cpu()
        launch(start + k, (P, G, M, V, T, A))
        after = (P.cpu(), M.cpu(), V.cpu())
        done = ((touched | act_before) != 0)[:nb]
        ent = done.repeat_interleave(be)
        ent = torch.cat([ent, torch.zeros(max(n, 4) - n, dtype=torch.bool)])
        if bool(ent.any()):
            check_step(out, "%s step %d" % (tag, start + k), before, g, after, (eps, 0.0, gs), start + k, ent, lr, b1, b2)
        bits = lambda t: t.view(torch.int32)
        for a, b in zip(before, after):                             # skipped blocks: p, m, v bit-unchanged ...
            assert torch.equal(bits(a)[~ent], bits(b)[~ent]), tag
        g_after = G.cpu()
        assert torch.equal(bits(g_after)[~ent], bits(g)[~ent]), tag + ": gradient of a skipped block"      # ... and g
        if zero_grad:
            assert not bool(g_after[ent].any()), tag + ": gradient of a processed block is cleared"
        else:
            assert torch.equal(bits(g_after)[ent], bits(g)[ent]), tag
        t_after, a_after = T.cpu()[:nb], A.cpu()[:nb]
        assert not bool(t_after[done].any()) and bool((a_after[done] == 1).all()), tag + ": flags of processed blocks"
        assert not bool(t_after[~done].any()) and not bool(a_after[~done].any()), tag + ": flags of skipped blocks"


BLOCKS = [(be, nb) for be in (4, 8, 252, 256, 260, 1024) for nb in (1, 3, 4, 5)] + [(4, 8192 * 4 + 3), (8, 8192 * 4 + 3)]


@pytest.mark.parametrize("zero_grad", [0, 1])
@pytest.mark.parametrize("be,nb", BLOCKS)
def test_blocks_raw(dev, be, nb, zero_grad):
    out = []
    eps, _, gs = tc.ADAM_HYPER[(be // 4 + nb) % 2]
    start = tc.ADAM_STEPS[(be + nb) % 6]
    _blocks_steps(dev, out, "", nb, be, zero_grad, be + nb + zero_grad, eps=eps, gs=gs, start=start,
                  launch=lambda step, t: raw_blocks(nb, be, *t, LR, B1, B2, eps, step, gs, zero_grad))
    show("adamw blocks block_elems=%d n_blocks=%d zero_grad=%d eps=%g gs=%g from step %d" % (be, nb, zero_grad, eps, gs, start), out)


@pytest.mark.parametrize("n_tensors", [1, 8])
@pytest.mark.parametrize("zero_grad", [0, 1])
def test_blocks_multi_raw(dev, n_tensors, zero_grad):
    """every tensor with its own n_blocks (one of them 0), block_elems, lr, betas, eps and step"""
    nbs = [5, 0, 1, 37, 4, 3, 300, 8][:n_tensors]
    bes = [256, 8, 4, 260, 1024, 252, 8, 4][:n_tensors]
    lrs = [1e-3, 2e-3, 5e-4, 1e-2, 3e-3, 1e-4, 7e-3, 1e-3][:n_tensors]
    b1s = [0.9, 0.8, 0.95, 0.5, 0.9, 0.85, 0.99, 0.0][:n_tensors]
    b2s = [0.99, 0.999, 0.9, 0.95, 0.99, 0.98, 0.999, 0.5][:n_tensors]
    epss = [1e-15, 1e-8, 1e-12, 1e-15, 1e-6, 1e-10, 1e-15, 1e-8][:n_tensors]
    starts = [1, 7, 1000, 2, 3, 100000, 10, 50][:n_tensors]
    gs = 0.125
    n = [max(a * b, 4) for a, b in zip(nbs, bes)]
    st = [tc.adam(n[t], "lattice", seed=900 + t) for t in range(n_tensors)]
    flags = [_flags(max(nbs[t], 1), t) for t in range(n_tensors)]
    P, M, V = ([s[j].to(dev) for s in st] for j in (0, 2, 3))
    A = [f[1].to(dev) for f in flags]
    out = []
    for k in range(STEPS):
        gsrc = [torch.roll(s[1], 131 * k) for s in st]
        for g in gsrc:
            g[g == 0] = 1e-3
        touched = [torch.roll(f[0], k) for f in flags]
        G, T = [g.to(dev) for g in gsrc], [t.to(dev) for t in touched]
        before = [(P[t].cpu(), M[t].cpu(), V[t].cpu(), A[t].cpu()) for t in range(n_tensors)]
        raw_blocks_multi(nbs, bes, P, G, M, V, T, A, lrs, b1s, b2s, epss, [s + k for s in starts], gs, zero_grad)
        for t in range(n_tensors):
            nb, be = nbs[t], bes[t]
            done = ((touched[t] | before[t][3]) != 0)[:nb]
            ent = torch.cat([done.repeat_interleave(be), torch.zeros(n[t] - nb * be, dtype=torch.bool)])
            after = (P[t].cpu(), M[t].cpu(), V[t].cpu())
            if bool(ent.any()):
                check_step(out, "t%d step %d" % (t, starts[t] + k), before[t][:3], gsrc[t], after, (epss[t], 0.0, gs), starts[t] + k, ent,
                           lrs[t], b1s[t], b2s[t])
            bits = lambda x: x.view(torch.int32)
            for a, b in zip(before[t][:3], after):
                assert torch.equal(bits(a)[~ent], bits(b)[~ent])
            ga = G[t].cpu()
            assert torch.equal(bits(ga)[~ent], bits(gsrc[t])[~ent])
            assert (not bool(ga[ent].any())) if zero_grad else torch.equal(bits(ga)[ent], bits(gsrc[t])[ent])
            ta, aa = T[t].cpu()[:nb], A[t].cpu()[:nb]
            assert not bool(ta[done].any()) and bool((aa[done] == 1).all())
            assert not bool(ta[~done].any()) and not bool(aa[~done].any())
    show("adamw blocks multi %d tensors zero_grad=%d" % (n_tensors, zero_grad), out)


def test_blocks_through_fused_adamw(dev, monkeypatch):
    """nine attached parameters, each in a group of its own: two launches (8 + 1)"""
    from permuto_sdf_amd.encoding import TouchedRows
    from permuto_sdf_amd.optim import FusedAdamW
    shape, log2 = (2, 256, 2), 6                                    # 4 blocks of 128 floats per level
    n = shape[0] * shape[1] * shape[2]
    st = [tc.adam(n, "lattice", seed=1200 + t) for t in range(9)]
    params = [torch.nn.Parameter(s[0].view(shape).to(dev)) for s in st]
    lrs = [1e-3 * (t + 1) for t in range(9)]
    epss = [(1e-15, 1e-8, 1e-12)[t % 3] for t in range(9)]
    opt = FusedAdamW([dict(params=[p], lr=lrs[t], eps=epss[t], betas=(0.9 - 0.05 * t, 0.99)) for t, p in enumerate(params)])
    trs = [TouchedRows(p.data, block_rows_log2=log2) for p in params]
    for p, tr in zip(params, trs):
        opt.attach(p, tr)
    launches = Launches(monkeypatch)
    out = []
    for k in range(STEPS):
        before, gsrc, done = [], [], []
        for t, (p, tr) in enumerate(zip(params, trs)):
            g = fresh_grad(n, "lattice", 1300 + 9 * k + t)
            touched = ((torch.arange(8) + t + k) % 3 == 0).to(torch.uint8)
            g = g * touched.bool().repeat_interleave(128)               # a gradient exists only where the forward marked rows
            tr.grad.copy_(g.view(shape))
            tr.touched.copy_(touched.view(2, 4))
            s = opt.state.get(p) or {}
            z = torch.zeros(n)
            before.append((p.detach().cpu().view(-1), s["exp_avg"].cpu().view(-1) if "exp_avg" in s else z,
                           s["exp_avg_sq"].cpu().view(-1) if "exp_avg" in s else z))
            gsrc.append(g)
            done.append(((touched | tr.active.cpu().view(-1)) != 0).repeat_interleave(128))
        launches.take()
        opt.step()
        assert launches.take() == ["psdf_adamw_step_blocks_multi", "psdf_adamw_step_blocks"], "eight tensors in one launch, the ninth alone"
        for t, (p, tr) in enumerate(zip(params, trs)):
            s = opt.state[p]
            after = (p.detach().cpu().view(-1), s["exp_avg"].cpu().view(-1), s["exp_avg_sq"].cpu().view(-1))
            if bool(done[t].any()):
                check_step(out, "p%d step %d" % (t, k + 1), before[t], gsrc[t], after, (epss[t], 0.0, 1.0), k + 1, done[t], lrs[t],
                           0.9 - 0.05 * t, 0.99)
            for a, b in zip(before[t], after):
                assert torch.equal(a[~done[t]].view(torch.int32), b[~done[t]].view(torch.int32))
            assert not bool(tr.grad.any()) and not bool(tr.touched.any())
    show("adamw blocks through FusedAdamW, 9 attached parameters", out)


# ============================================================================================================== owned
def test_owned_ranges_of_a_dense_parameter(dev):
    from permuto_sdf_amd.optim import FusedAdamW
    n, ranges = 64, [(4, 12), (20, 40)]
    eps, wd, gs = tc.ADAM_HYPER[1]
    p0 = tc.adam(n, "randn", seed=21)[0]
    p = torch.nn.Parameter(p0.to(dev))
    opt = FusedAdamW([p], lr=LR, betas=(B1, B2), eps=eps, weight_decay=wd)
    inside = torch.zeros(n, dtype=torch.bool)
    for lo, hi in ranges:
        inside[lo:hi] = True
    out = []
    for k in range(STEPS):
        g = fresh_grad(n, "randn", 30 + k)
        s = opt.state.get(p) or {}
        z = torch.zeros(n)
        before = (p.detach().cpu(), s["exp_avg"].cpu() if "exp_avg" in s else z, s["exp_avg_sq"].cpu() if "exp_avg" in s else z)
        p.grad = g.to(dev)
        opt.step(grad_scale=gs, owned={p: ranges})
        s = opt.state[p]
        after = (p.detach().cpu(), s["exp_avg"].cpu(), s["exp_avg_sq"].cpu())
        check_step(out, "step %d" % (k + 1), before, g, after, (eps, wd, gs), k + 1, inside)
        for a, b in zip(before, after):
            assert torch.equal(a[~inside].view(torch.int32), b[~inside].view(torch.int32)), "outside the owned ranges"
    show("adamw step(owned=...) n=%d ranges %s" % (n, ranges), out)


# ===================================================================================================== argument checks
def test_argument_checks_return_errors(dev):
    L = _L()
    t = lambda k=64: torch.zeros(k, device=dev)
    p, g, m, v = t(), t(), t(), t()
    by = lambda k=4: torch.zeros(k, dtype=torch.uint8, device=dev)
    hyper = tc.ADAM_HYPER[0]

    def refused(fn):
        with pytest.raises(L.PsdfError, match="status -1"):
            fn()
    refused(lambda: raw_dense(p[1:5], g[:4], m[:4], v[:4], hyper, 1))                       # misaligned pointer
    refused(lambda: raw_dense(p, g, m, v, hyper, 0))                                         # step < 1
    refused(lambda: raw_multi([p[1:5]], [g[:4]], [m[:4]], [v[:4]], hyper, 1))
    refused(lambda: raw_multi([p], [g], [m], [v], hyper, 0))
    refused(lambda: raw_multi([p] * 65, [g] * 65, [m] * 65, [v] * 65, hyper, 1))             # more than 64 tensors
    refused(lambda: raw_blocks(4, 6, p, g, m, v, by(), by(), LR, B1, B2, 1e-15, 1, 1.0, 1))  # block_elems not a multiple of 4
    refused(lambda: raw_blocks(4, 4, p[1:17], g[:16], m[:16], v[:16], by(), by(), LR, B1, B2, 1e-15, 1, 1.0, 1))
    refused(lambda: raw_blocks(4, 4, p, g, m, v, by(), by(), LR, B1, B2, 1e-15, 0, 1.0, 1))
    one = lambda x: [x]
    refused(lambda: raw_blocks_multi([4], [6], one(p), one(g), one(m), one(v), one(by()), one(by()), [LR], [B1], [B2], [1e-15], [1], 1.0, 1))
    refused(lambda: raw_blocks_multi([4], [4], one(p), one(g), one(m), one(v), one(by()), one(by()), [LR], [B1], [B2], [1e-15], [0], 1.0, 1))
    refused(lambda: raw_blocks_multi([4] * 9, [4] * 9, [p] * 9, [g] * 9, [m] * 9, [v] * 9, [by()] * 9, [by()] * 9, [LR] * 9, [B1] * 9,
                                     [B2] * 9, [1e-15] * 9, [1] * 9, 1.0, 1))                # more than 8 tensors
    assert not bool(p.any()) and not bool(m.any()) and not bool(v.any())
