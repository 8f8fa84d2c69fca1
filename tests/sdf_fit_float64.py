"""FLOAT64 EVALUATOR of the SDF-fitting loss tail (csrc/sdf_fit.hip) and the cases it is checked on.  TEST INFRASTRUCTURE ONLY.

Plain torch float64 on the CPU, no autograd, no HIP.  Inputs are fp32 tensors taken exactly; weights, sharpness, eik_clamp and
scale are taken as the fp32 numbers the C ABI receives.  `evaluate` returns the four terms, the loss and both gradients together
with a PER-ENTRY BAR on |fp32 kernel - float64|, in the manner of oracle/tails_float64.py, whose running-error primitives
(_mul, _add, _div, _dot3, _sqrt; U = 2^-24, TINY = 2^-126, SLACK, ULP_EXPF) are reused.

THE FORMULA (sdf_loss of the reference, permuto_sdf_py/utils/sdf_utils.py:16-57, in the project's words).  Row i has the SDF
value s, the gradient g (the first three columns of its row of `gradients`) and, on the surface (i < n_surf), the normal n:
    term 0 = mean over all rows       w | |g| - 1 |,  w = exp(-s^2 / (2 c^2)) under an eikonal clamp c, else 1; w is a constant
    term 1 = mean over surface rows   1 - (g / max(|g|, 1e-8)) . (n / max(|n|, 1e-8))
    term 2 = mean over surface rows   |s|
    term 3 = mean over the others     exp(-sharpness |s|)
    loss   = loss0 + scale sum_k weights[k] term k
sign(0) = 0 in both absolute values, d|g|/dg = 0 at g = 0, a mean over no rows is 0.  The clamps of term 1 act on the VALUES of
the norms only: the installed torch's F.cosine_similarity clamps them in place outside the graph, so the derivative of a clamped
norm stays that of the norm (tests/test_sdf_fit_host.py holds the evaluator to torch autograd at |g| = 1e-9 and at g = 0).  With a = max(|g|, 1e-8), u = n / max(|n|, 1e-8), cos = (g / a) . u
and C_k = scale weights[k] / rows of mean k:
    d loss / d g = C_0 w sign(|g| - 1) g / |g|  -  C_1 (u / a - [|g| > 0] cos g / (a |g|))            (second part: surface rows)
    d loss / d s = C_2 sign(s) on the surface,  -C_3 sharpness sign(s) exp(-sharpness |s|) off it;  the time column gets 0.

THE BARS: a first-order running error analysis of the expressions as csrc/sdf_fit.hip writes them.  Every intermediate z carries
a bound E(z) of |fp32 z - float64 z|: one rounding u |z| per operation, inherited errors through the partial derivatives, sqrtf
and the divisions correctly rounded, expf within ULP_EXPF ulps (oracle/tails_float64.py states each rule).  The coefficients C_k
are formed in double on the host and rounded once: E(C_k) = u |C_k|; 2 c^2 likewise.  The kernel's 1e-8f differs from 1e-8 by
6e-17, which a clamped norm carries as its error.  Where the FORMULA is ill conditioned the absolute terms dominate by
construction: e = |g| - 1 has E(e) ~ 2.5 u against e -> 0, and u / a - cos g / (a |g|) cancels to 0 for g parallel to n while
both parts carry ~10 u / a.

BRANCHES.  sign(|g| - 1) is decided by the fp32 value of |g| - 1: a row whose float64 | |g| - 1 | lies within E(e) may take
either arm or 0.  Such a row is reported in `ambiguous`; `grad_gradients_arms` [3, N, P] holds the gradient for sign = -1, 0, +1
with bars, and the row passes when all of its entries fit ONE arm.  The terms need no such care (|e| is continuous).  |g| > 0 is
decided alike in both precisions: a sum of squares of fp32 numbers that is 0 in one is 0 in the other unless a square underflows
(|g| < 2^-63: the bar of such a row is infinite through its quotient).

THE MEANS.  Every thread adds its rows in double, the workgroup's tree and the finishing launch add in double: against the fp32
roundings of the rows the 2^-53 of these additions vanishes (covered by SLACK).  term k = (float)(sum / count):
    bar = SLACK sum E(t) / count + u |term k| + TINY;   loss: sum_k |scale weights[k]| bar_k + u |added| + u |loss0 + added| + TINY.

No constant of any bar is fitted to what the kernels produce.
"""
import math

import torch

from oracle.composite_float64 import SLACK, TINY, U, ULP_EXPF, _f32
from oracle.tails_float64 import _add, _d, _div, _dot3, _fin, _mul, _sqrt, _z

EPS = 1e-8                      # torch's F.cosine_similarity default
EPS32 = _f32(1e-8)              # what the kernel holds
REFERENCE_WEIGHTS = (5e1, 1e2, 3e3, 1e2)


def _clamped_norm(x):
    """-> (|x|, E, max(|x|, EPS), E)"""
    dd, Edd = _dot3(x, _z(x), x, _z(x))
    nrm, En = _sqrt(dd, Edd)
    d_eps = abs(EPS - EPS32)
    den = nrm.clamp_min(EPS)
    Eden = torch.where(nrm + En <= min(EPS, EPS32), torch.full_like(nrm, d_eps), En + d_eps)
    return nrm, En, den, Eden


def _col(v, like):
    return v[:, None].expand_as(like)


def evaluate(sdf, gradients, normals, n_surf, weights=REFERENCE_WEIGHTS, sharpness=1e2, eik_clamp=None, scale=1.0 / 30000.0,
             loss0=0.0):
    """-> dict(terms [4], terms_bar [4], loss, loss_bar, grad_sdf [N], grad_sdf_bar, grad_gradients [N, P], grad_gradients_bar,
    ambiguous [N] bool, grad_gradients_arms [3, N, P], grad_gradients_arms_bar [3, N, P])"""
    s, G = _d(sdf).reshape(-1), _d(gradients)
    N, P = G.shape
    n_surf = int(n_surf)
    n_off = N - n_surf
    g = G[:, :3]
    wts = [_f32(w) for w in weights]
    sc, sh = _f32(scale), _f32(sharpness)
    counts = [N, n_surf, n_surf, n_off]
    C = [sc * wts[k] / counts[k] if counts[k] else 0.0 for k in range(4)]
    surf = torch.arange(N) < n_surf

    # ---- term 0 and its gradient
    ln, Eln, ga, Ega = _clamped_norm(g)
    e, Ee = ln - 1.0, Eln + U * (ln - 1.0).abs()
    if eik_clamp is not None and _f32(eik_clamp) > 0:
        c = _f32(eik_clamp)
        two = 2.0 * c * c                      # the kernel holds it rounded once: E = u two
        ss, Ess = _mul(s, _z(s), s, _z(s))
        q, Eq = _div(ss, Ess, torch.full_like(s, two), torch.full_like(s, U * two))
        w = torch.exp(-q)
        Ew = w * (torch.expm1(Eq) + 2 * ULP_EXPF * U) + TINY
    else:
        w, Ew = torch.ones_like(s), _z(s)
    t0 = w * e.abs()
    Et0 = Ew * e.abs() + w * Ee + Ew * Ee + U * t0 + TINY
    ambiguous = e.abs() <= Ee
    cw, Ecw = C[0] * w, abs(C[0]) * Ew + 2 * U * (C[0] * w).abs() + TINY          # the cast of C_0 and the product
    ke, Eke = _div(cw, Ecw, ln, Eln)
    ke, Eke = torch.where(ln > 0, ke, _z(ke)), torch.where(ln > 0, Eke, _z(Eke))   # g = 0: exactly 0
    d0, Ed0 = _mul(_col(ke, g), _col(Eke, g), g, _z(g))
    Ed0 = torch.where(g == 0, _z(Ed0), Ed0)

    # ---- terms 1 and 2 and their gradients (surface rows; computed for the first n_surf rows only)
    gs, lns, gas, Egas = g[:n_surf], ln[:n_surf], ga[:n_surf], Ega[:n_surf]
    n = _d(normals).reshape(-1, 3)[:n_surf] if n_surf else torch.zeros(0, 3, dtype=torch.float64)
    _, _, nb, Enb = _clamped_norm(n)
    u, Eu = _div(n, _z(n), _col(nb, n), _col(Enb, n))
    xg, Exg = _div(gs, _z(gs), _col(gas, gs), _col(Egas, gs))
    cos, Ecos = _dot3(xg, Exg, u, Eu)
    t1 = 1.0 - cos
    Et1 = Ecos + U * t1.abs()
    t2 = s[:n_surf].abs()
    first, Ef = _div(u, Eu, _col(gas, u), _col(Egas, u))
    gl, Egl = _mul(gas, Egas, lns, Eln[:n_surf])
    back, Eback = _div(cos, Ecos, gl, Egl)
    sec, Esec = _mul(_col(back, gs), _col(Eback, gs), gs, _z(gs))
    open_arm, Eopen = _add(first, Ef, sec, Esec, -1.0)
    pos = _col(lns > 0, gs)
    dcos = torch.where(pos, open_arm, first)
    Edcos = torch.where(pos, _fin(Eopen), Ef)
    d1 = C[1] * dcos
    Ed1 = abs(C[1]) * Edcos + 2 * U * d1.abs() + TINY

    # ---- term 3 and its gradient (the other rows)
    so = s[n_surf:]
    y = sh * so.abs()
    ex = torch.exp(-y)
    Eex = ex * (torch.expm1(U * y) + 2 * ULP_EXPF * U) + TINY
    gso = -(C[3] * sh) * torch.sign(so) * ex
    Egso = torch.where(so == 0, _z(so), abs(C[3] * sh) * Eex + 3 * U * gso.abs() + TINY)

    grad_sdf = torch.cat([C[2] * torch.sign(s[:n_surf]), gso])
    grad_sdf_bar = torch.cat([U * (C[2] * torch.sign(s[:n_surf])).abs(), Egso])

    def assemble(sign):
        val, bar = torch.zeros(N, P, dtype=torch.float64), torch.zeros(N, P, dtype=torch.float64)
        a, Ea = _col(sign, g) * d0, torch.where(_col(sign, g) == 0, _z(Ed0), Ed0)
        b, Eb = torch.cat([d1, _z(g[n_surf:])]), torch.cat([Ed1, _z(g[n_surf:])])
        v = a - b
        val[:, :3] = v
        bar[:, :3] = torch.where(_col(surf, g), Ea + Eb + U * v.abs(), Ea)
        return val, _fin(bar)

    arms = [assemble(torch.full_like(e, sgn)) for sgn in (-1.0, 0.0, 1.0)]
    gg, gg_bar = assemble(torch.sign(e))

    # ---- the means and the loss
    sums = [(t0, Et0, N), (t1, Et1, n_surf), (t2, _z(t2), n_surf), (ex, Eex, n_off)]
    terms = torch.tensor([float(t.sum()) / cnt if cnt else 0.0 for t, _, cnt in sums], dtype=torch.float64)
    terms_bar = torch.tensor([(SLACK * float(E.sum()) / cnt if cnt else 0.0) for _, E, cnt in sums], dtype=torch.float64)
    terms_bar = terms_bar + U * terms.abs() + TINY
    added = sum(sc * wts[k] * float(terms[k]) for k in range(4))
    loss = float(loss0) + added
    loss_bar = sum(abs(sc * wts[k]) * float(terms_bar[k]) for k in range(4)) + U * abs(added) + U * abs(loss) + TINY
    return dict(terms=terms, terms_bar=terms_bar, loss=loss, loss_bar=loss_bar, grad_sdf=grad_sdf, grad_sdf_bar=grad_sdf_bar,
                grad_gradients=gg, grad_gradients_bar=gg_bar, ambiguous=ambiguous,
                grad_gradients_arms=torch.stack([a[0] for a in arms]), grad_gradients_arms_bar=torch.stack([a[1] for a in arms]))


def check_gradients(got, ev):
    """got [N, P] against the evaluator: an unambiguous row inside its bars, an ambiguous one inside the bars of ONE of the three
    arms of sign(|g| - 1) -> (worst error / bar over the unambiguous rows, rows outside)"""
    got = got.detach().cpu().double()
    err = (got - ev["grad_gradients"]).abs()
    ok = (err <= ev["grad_gradients_bar"]).all(dim=1)
    arm_ok = ((got[None] - ev["grad_gradients_arms"]).abs() <= ev["grad_gradients_arms_bar"]).all(dim=2).any(dim=0)
    amb = ev["ambiguous"]
    bad = torch.where(amb, ~arm_ok, ~ok)
    ratio = (err / ev["grad_gradients_bar"].clamp_min(1e-300))[~amb]
    return (float(ratio.max()) if ratio.numel() else 0.0), bad.nonzero().view(-1).tolist()


# --------------------------------------------------------------------------------------------------------------------- cases
def _unit(x):
    return x / x.norm(dim=1, keepdim=True).clamp_min(1e-30)


def cases(P, n_surf, n_off, family, seed=0):
    """fp32 CPU tensors sdf [N], gradients [N, P], normals [n_surf, 3] of one of two families.
    "training": where fitting runs -- |g| = 1 +- 0.3, off-surface |s| <= 0.5, surface |s| <= 1e-2, normals within ~30 degrees of g
    for most rows and anywhere for the rest.
    "ill": the same rows with every seventh-row pattern replaced by a place where the formulas are ill conditioned: |g| = 1
    exactly (an axis and a 3-4-5 direction), g = 0, s = 0, g antiparallel to n, |g| = 1e-9, g parallel to n with |g| within one ulp of 1."""
    gen = torch.Generator().manual_seed(1000 * seed + 10 * P + (0 if family == "training" else 1))
    N = n_surf + n_off
    d = _unit(torch.randn(N, 3, generator=gen, dtype=torch.float64))
    g = d * (1.0 + 0.3 * (2 * torch.rand(N, 1, generator=gen, dtype=torch.float64) - 1))
    s = torch.rand(N, generator=gen, dtype=torch.float64) - 0.5
    s[:n_surf] = (2 * torch.rand(n_surf, generator=gen, dtype=torch.float64) - 1) * 1e-2
    n = _unit(d[:n_surf] + 0.3 * torch.randn(n_surf, 3, generator=gen, dtype=torch.float64))
    wild = torch.rand(n_surf, generator=gen) < 0.1
    n[wild] = _unit(torch.randn(int(wild.sum()), 3, generator=gen, dtype=torch.float64))
    n = n * (1.0 + 1e-3 * torch.randn(n_surf, 1, generator=gen, dtype=torch.float64))     # normals of a mesh are unit up to rounding
    if family == "ill":
        k = torch.arange(N) % 8
        on_surf = torch.arange(N) < n_surf
        g[k == 0] = torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64)
        g[k == 1] = torch.tensor([0.6, 0.0, 0.8], dtype=torch.float64)
        g[k == 2] = 0.0
        s[k == 3] = 0.0
        g[:n_surf][k[:n_surf] == 4] = -1.2 * n[k[:n_surf] == 4]
        g[k == 5] = torch.tensor([1e-9, 0.0, 0.0], dtype=torch.float64)
        m6 = (k == 6) & on_surf
        g[m6] = _unit(n[m6[:n_surf]]) * (1.0 + 2.0 ** -23)
    elif family != "training":
        raise ValueError(family)
    G = torch.cat([g, torch.randn(N, P - 3, generator=gen, dtype=torch.float64)], 1) if P > 3 else g
    return s.float(), G.float().contiguous(), n.float().contiguous()


FAMILIES = ("training", "ill")
CLAMPS = (None, 0.05)


def torch_formula(sdf, gradients, normals, n_surf, weights=REFERENCE_WEIGHTS, sharpness=1e2, eik_clamp=None, scale=1.0 / 30000.0,
                  detach_weight=True, abs_fn=torch.abs):
    """the formula above in torch operators of the tensors' own dtype, for autograd -> (loss, terms [4]).  detach_weight and abs_fn
    exist for the tests that show the bars bite."""
    import torch.nn.functional as F
    s = sdf.reshape(-1)
    g = gradients[:, :3]
    eik = abs_fn(g.norm(dim=-1) - 1.0)
    if eik_clamp is not None:
        x = abs_fn(s)
        x = x.detach() if detach_weight else x
        eik = eik * torch.exp(-(x * x) / (2.0 * eik_clamp * eik_clamp))
    zero = s.new_zeros(())
    off = s[n_surf:]
    terms = [eik.mean() if eik.numel() else zero,
             (1.0 - F.cosine_similarity(g[:n_surf], normals, dim=-1)).mean() if n_surf else zero,
             abs_fn(s[:n_surf]).mean() if n_surf else zero,
             torch.exp(-sharpness * abs_fn(off)).mean() if off.numel() else zero]
    loss = sum(t * w for t, w in zip(terms, weights)) * scale
    return loss, torch.stack(terms)


assert math.isclose(EPS32, 1e-8, rel_tol=1e-7)
