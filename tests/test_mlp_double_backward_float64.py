"""Host: the float64 evaluator of the MLP double backward (tests/mlp_float64.py: f64_double_backward), which the GPU test
tests/test_gpu_mlp_double_backward_float64.py holds mlp_dbl_bwd_kernel to, entry by entry.  No kernel runs here.

  the pin        the hand-written evaluator equals torch float64 autograd of <d y / d x . dY, V> + <Y, dY2> (create_graph=True) on
                 every family of the GPU test: |delta| / S <= 1e-12 with S the entry's own absolute sum
  zero entries   every family has the entries with S == 0 that it claims (the dW_1 columns of closed levels and of the pad column,
                 the dX2 rows of missed samples, db_4 without dY2, the dW_4 rows of outputs without an upstream gradient), and the
                 evaluator returns exactly 0 there
  tails          the "tails" family really reaches max |z_1| >= 6 and has at least 1 % of its z_1 within 0.05 of +-sqrt 2
  mutations      each deliberate defect of DBL_MUTATIONS moves at least one tensor by 10 x 2e-5 under the same metric on N = 4 099:
                 2e-5 is the loosest bar a GPU case is expected to get (4 x the largest figure of torch fp32 seen, 5.4e-6)

Prints the pin, the zero-entry shares and the mutation table (also in LABNOTES.md)."""
import pytest
import torch

from tests import mlp_float64 as M
from tests.mlp_float64 import _per_entry, f64_double_backward, double_backward_autograd

PIN = 1e-12
LOOSEST_BAR = 2e-5
N_HOST = 259                 # 16 tiles + 3: every family at a batch the host evaluates in float64 at once
N_MUTATIONS = 4_099          # 256 tiles + 3


def _families():
    """every distinct family of the GPU cases (the geometry cases differ from the row cases only in N)"""
    seen, out = set(), []
    for c in M.DBL_ROW_CASES + M.DBL_NUMERICS_CASES + M.DBL_GEOMETRY_CASES:
        f = c.at(N_HOST)
        if f.key() not in seen:
            seen.add(f.key())
            out.append(f)
    return out


FAMILIES = _families()


def _claimed_zeros(case, S):
    """{tensor: mask of the entries the family claims to have S == 0}"""
    K0, out = case.dims[0], case.dims[4]
    claims = {}
    if M.sdf_layout(K0):
        cols = torch.zeros(K0, dtype=torch.bool)
        cols[K0 - 1] = True
        L = M.sdf_levels(K0)
        cols[2 * (L - case.closed()):2 * L] = True
        claims["dW1"] = cols[None, :].expand_as(S["dW1"])
    if case.misses:
        rows = torch.zeros(case.N, dtype=torch.bool)
        rows[5::16] = True
        claims["dX2"] = rows[:, None].expand_as(S["dX2"])
    if not case.plus:
        claims["db4"] = torch.ones(out, dtype=torch.bool)
    if case.dy == "unit" and not case.plus and out > 1:
        rows = torch.ones(out, dtype=torch.bool)
        rows[0] = False
        claims["dW4"] = rows[:, None].expand_as(S["dW4"])
    return claims


@pytest.mark.parametrize("case", FAMILIES, ids=repr)
def test_evaluator_matches_float64_autograd_and_has_its_zero_entries(case):
    lin, x, dy, v, dy2 = case.make()
    g, S, Z = f64_double_backward(lin, x, dy, v, dy2)
    ref = double_backward_autograd(lin, x, dy, v, dy2)
    worst = 0.0
    for k in M.DBL_TENSORS:
        assert g[k].shape == ref[k].shape == S[k].shape, k
        e, bad = _per_entry(g[k], ref[k], S[k])
        assert not bad, (k, "autograd is not exactly 0 where S == 0")
        assert bool(((S[k] == 0) <= (g[k] == 0)).all()), (k, "the evaluator is not exactly 0 where S == 0")
        worst = max(worst, e)
        assert e <= PIN, (k, e)
    claims = _claimed_zeros(case, S)
    shares = []
    for k, mask in claims.items():
        assert bool(mask.any()) and bool((S[k][mask] == 0).all()), (k, "claimed zero entries have terms")
        shares.append("%s %.3f" % (k, float((S[k] == 0).double().mean())))
    if M.sdf_layout(case.dims[0]):
        assert "dW1" in claims
    if case.misses:
        assert "dX2" in claims
    print("double backward %r: pin %.1e; share of entries with S == 0: %s" % (case, worst, " ".join(shares) or "none claimed"))
    if case.tails:
        z1 = Z[0]
        near = float((((z1.abs() - 2 ** 0.5).abs()) <= 0.05).double().mean())
        print("double backward %r: max |z_1| %.2f, share of z_1 within 0.05 of +-sqrt 2: %.4f" % (case, float(z1.abs().max()), near))
        assert float(z1.abs().max()) >= 6.0
        assert near >= 0.01


def test_tails_family_at_the_gpu_batch():
    """the drawn GPU cases themselves (N = 16 423), not only their families at the host batch"""
    for case in M.DBL_NUMERICS_CASES:
        if not case.tails:
            continue
        lin, x, _, _, _ = case.make()
        z1 = x.double() @ lin[0].weight.detach().double().t() + lin[0].bias.detach().double()
        near = float((((z1.abs() - 2 ** 0.5).abs()) <= 0.05).double().mean())
        print("double backward %r: max |z_1| %.2f, share within 0.05 of +-sqrt 2: %.4f" % (case, float(z1.abs().max()), near))
        assert float(z1.abs().max()) >= 6.0 and near >= 0.01, (case, float(z1.abs().max()), near)


@pytest.mark.parametrize("case", [M.DblCase(M.DBL_BASE, N_MUTATIONS, lattice=1e-2),
                                  M.DblCase(M.DBL_REF, N_MUTATIONS, lattice=1e-2, plus=True)], ids=repr)
def test_every_mutation_is_visible_under_the_metric(case):
    lin, x, dy, v, dy2 = case.make()
    g, S, _ = f64_double_backward(lin, x, dy, v, dy2)
    missed = []
    for mut in M.DBL_MUTATIONS:
        if mut[0] in ("drop_dY2H3", "dY2_without_a3") and not case.plus:
            continue
        gm, _, _ = f64_double_backward(lin, x, dy, v, dy2, mutate=mut)
        figs = {k: _per_entry(gm[k], g[k], S[k])[0] for k in M.DBL_TENSORS}
        print("double backward %r mutation %s %d: %s" % (case, mut[0], mut[1],
                                                         " ".join("%s %.1e" % kv for kv in figs.items() if kv[1] > 0)))
        if not max(figs.values()) >= 10 * LOOSEST_BAR:
            missed.append((mut, max(figs.values())))
    assert not missed, missed
