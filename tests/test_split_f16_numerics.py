"""Host-side restatement (numpy) of the arithmetic of the two-piece fp16 MLP kernels (csrc/mlp_bwd_split_f16.hip, the f16 path of
csrc/mlp_device.h, csrc/mlp_wide.hip): every fp32 operand a = a0 + a1 with a0 = fp16(a) (the remainder a - a0 is exact in fp32)
and a1 = fp16(a - a0) rounded to nearest, products a0 b0 + a0 b1 + a1 b0 accumulated in fp32 (the parameter-gradient products
keep a1 b1 too).
Rounding of the high piece: rounds 3-5 rounded it TOWARD ZERO (v_cvt_pkrtz) -- `f16_rtz` / `split2` below, and the tests written
for them, which stay because what they establish (an exact remainder, the need for the third product, for the chain on the
mantissa of dY and for the H pre-scale) holds for either rounding.  Since round 6 NO kernel does: split2 of
mlp_bwd_split_f16.hip, split8h / split1h of mlp_device.h and wsplit2 of mlp_wide.hip all round the high piece to NEAREST
(v_cvt_pk_f16_f32) -- `split2_rtn` below, which `dw1_model` uses.  (The one v_cvt_pkrtz left, transpose_pieces of
mlp_bwd_split_f16.hip, converts values that are fp16 numbers already: exact.)
What the kernels rely on and what their guards are for is checked here without a GPU; the GPU counterparts are
tests/test_gpu_mlp_baseline_numerics.py (per entry; its inputs are first held against `dw1_model` here),
tests/test_gpu_mlp.py::test_split_f16_backward_matches_float64 / ..._forward_against_float64 and
tests/test_gpu_hotpath_parity.py::test_cfg2_full_batch_dense_gradient_against_float64."""
import numpy as np
import pytest
import torch

from tests import mlp_float64 as M


def f16_rtz(x):
    """fp32 -> fp16 rounded toward zero, subnormals kept, overflow saturating at the largest finite number (v_cvt_pkrtz)"""
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore"):
        h = x.astype(np.float16)
    too_big = np.abs(h.astype(np.float64)) > np.abs(x.astype(np.float64))
    h = np.where(too_big, np.nextafter(h, np.float16(0)), h)
    return h.astype(np.float16)


def split2(x):
    """(high, low) fp16 pieces of fp32 values, as the kernels form them"""
    x = np.asarray(x, np.float32)
    hi = f16_rtz(x)
    rem = x - hi.astype(np.float32)                 # exact in fp32 (checked below)
    return hi, rem.astype(np.float16)               # numpy's cast rounds to nearest even, like v_fma_mix


def prod3(a, b):
    """a0 b0 + a0 b1 + a1 b0 in float64 (every piece product is exact in fp32: 11 x 11 significant bits)"""
    a0, a1 = (p.astype(np.float64) for p in split2(a))
    b0, b1 = (p.astype(np.float64) for p in split2(b))
    return a1 * b0 + a0 * b1 + a0 * b0


def test_remainder_is_exact_and_pieces_reconstruct_to_22_bits():
    rng = np.random.default_rng(0)
    x = (rng.standard_normal(200_000) * 10.0 ** rng.uniform(-4, 4, 200_000)).astype(np.float32)
    hi, lo = split2(x)
    rem64 = x.astype(np.float64) - hi.astype(np.float64)
    assert np.array_equal((x - hi.astype(np.float32)).astype(np.float64), rem64)        # the fp32 subtraction lost nothing
    assert np.all(np.abs(hi.astype(np.float64)) <= np.abs(x.astype(np.float64)))         # toward zero
    ok = np.abs(x) > 2.0 ** -3                      # low piece still a NORMAL fp16 number: 11 + 11 bits
    err = np.abs(hi.astype(np.float64) + lo.astype(np.float64) - x) / np.abs(x)
    assert err[ok].max() <= 2.0 ** -22
    # below 2^-3 the low piece is an fp16 SUBNORMAL: absolute precision 2^-25 (half the subnormal spacing), which is what makes
    # the scheme legitimate on gfx950 only because its matrix pipe honours subnormal inputs (attic/prototypes/mlp_fwd_split_f16.hip)
    small = np.abs(x) <= 2.0 ** -3
    assert np.abs(hi.astype(np.float64) + lo.astype(np.float64) - x)[small].max() <= 2.0 ** -25


def test_three_products_reach_fp32_level_two_do_not():
    rng = np.random.default_rng(1)
    a = rng.standard_normal(100_000).astype(np.float32)
    b = rng.standard_normal(100_000).astype(np.float32)
    exact = a.astype(np.float64) * b.astype(np.float64)
    e3 = np.abs(prod3(a, b) - exact) / np.abs(exact).max()
    a0, _ = split2(a)
    b0, b1 = split2(b)
    e2 = np.abs(a0.astype(np.float64) * (b0.astype(np.float64) + b1.astype(np.float64)) - exact) / np.abs(exact).max()
    assert e3.max() <= 2.0 ** -20 and e2.max() >= 2.0 ** -13          # dropping a1 b0 costs a thousand times more than a1 b1


def test_a_chain_on_the_mantissa_of_dy_is_as_accurate_for_small_gradients_as_for_large_ones():
    """dX[n] = W^T (dY[n] g): linear in dY[n].  On dY itself a sample whose gradient is 1e-6 of the batch's largest would have
    fp16-subnormal operands (2^-24 absolute precision: nothing left); on the MANTISSA of its dY, scaled into [2^4, 2^5) and
    multiplied back by 2^(e - 4) at the store (dy_parts in the kernel), every sample keeps 22 bits relative to itself."""
    rng = np.random.default_rng(2)
    w = rng.standard_normal(64).astype(np.float32) * 0.2
    g = rng.uniform(0.0, 1.1, 64).astype(np.float32)                   # gelu'
    for dy in (np.float32(1.0), np.float32(3e-7), np.float32(2e4)):
        exact = w.astype(np.float64) * (np.float64(dy) * g.astype(np.float64))
        naive = prod3(w, (dy * g).astype(np.float32))
        m, e = np.frexp(dy)                                            # dy = m 2^e, m in [0.5, 1)
        mant = np.float32(m * 32.0)                                    # [2^4, 2^5)
        scaled = prod3(w, (mant * g).astype(np.float32)) * 2.0 ** (int(e) - 5)
        rel = lambda v: (np.abs(v - exact) / np.abs(exact).max()).max()
        assert rel(scaled) <= 2.0 ** -20, (dy, rel(scaled))
        if dy < 1e-5:
            assert rel(naive) > 1e-3, (dy, rel(naive))                 # what the guard is for


def test_h_operand_needs_the_prescale_for_small_activations():
    """dW += dZ^T (H[n] 2^(e(n) - e_max)), e_max from the largest |dY| of the launch.  With encoding-like activations (1e-2), dY spread
    over six decades and ONE outlier that sets e_max, the H-side operand of most samples sits at or below fp16's subnormal spacing
    and their contributions lose their bits -- the truncation toward zero makes the loss systematic, not noise.  Round 4 measured
    1.2e-3 .. 1.7e-3 of dW on the GPU (test_cfg2_full_batch_dense_gradient_against_float64); this emulation gives 2.0e-3.
    Pre-scaled by 2^8 (H_PRESCALE_EXP, taken out again by the summing launch) the same sum is good to 1e-5 (here 7e-6, GPU
    <= 1.5e-5).  Same-signed terms, so that nothing cancels and the bias shows."""
    rng = np.random.default_rng(3)
    n = 200_000
    h = np.abs(rng.standard_normal(n) * 1e-2).astype(np.float32)
    dy = (rng.standard_normal(n) * 10.0 ** (-6.0 * rng.uniform(0, 1, n))).astype(np.float32)
    dy[0] = 1e3
    m, e = np.frexp(dy)                                                  # dy = m 2^e
    dz = (np.abs(m) * 32.0 * rng.uniform(0.05, 1.0, n)).astype(np.float32)   # |dZ| as the chain carries it: on mantissas in [16, 32)
    e2 = (e - e.max()).astype(np.int64)                                  # per-sample exponent relative to the launch maximum
    exact = np.sum(dz.astype(np.float64) * h.astype(np.float64) * 2.0 ** e2)

    def emulated(prescale):
        op = (h.astype(np.float64) * 2.0 ** (e2 + prescale)).astype(np.float32)      # exact power-of-two scaling
        a0, a1 = (p.astype(np.float64) for p in split2(dz))
        b0, b1 = (p.astype(np.float64) for p in split2(op))
        return np.sum(a0 * b0 + a0 * b1 + a1 * b0 + a1 * b1) * 2.0 ** -prescale      # the dW products keep all four

    assert abs(emulated(8) - exact) / exact <= 1e-5
    assert abs(emulated(0) - exact) / exact >= 1e-3
    # the limit the header states: an activation above 255 saturates its pre-scaled high piece
    assert float(f16_rtz(np.float32(300.0 * 2.0 ** 8))) == 65504.0


# ---------------------------------------------------------------------------------------------------------------------------
# Round to nearest (the kernels since round 6) and the dW1 product of the BASELINE net's backward, per entry

def split2_rtn(x):
    """(high, low) fp16 pieces of fp32 values with the high piece rounded to NEAREST even (v_cvt_pk_f16_f32), subnormals kept;
    the remainder is exact in fp32 and the low piece is its fp16 rounded to nearest (v_fma_mixlo/hi_f16)"""
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore"):
        hi = x.astype(np.float16)
    rem = x - hi.astype(np.float32)
    return hi, rem.astype(np.float16)


def test_nearest_split_has_an_exact_remainder_and_half_the_error_of_truncation():
    rng = np.random.default_rng(4)
    x = (rng.standard_normal(200_000) * 10.0 ** rng.uniform(-4, 4, 200_000)).astype(np.float32)
    hi, lo = split2_rtn(x)
    x64, hi64, lo64 = x.astype(np.float64), hi.astype(np.float64), lo.astype(np.float64)
    assert np.array_equal((x - hi.astype(np.float32)).astype(np.float64), x64 - hi64)       # the fp32 subtraction lost nothing
    # from 2^-2 on: a remainder of at most 2^-11 of the binade rounds to 2^-23 of it where the low piece is a normal number, and
    # the 2^-25 of a subnormal low piece is 2^-23 of the value too (truncation: 2^-22); below, the absolute 2^-25 stays
    ok = np.abs(x) >= 2.0 ** -2
    assert (np.abs(hi64 + lo64 - x64) / np.abs(x64))[ok].max() <= 2.0 ** -23
    assert np.abs(hi64 + lo64 - x64)[~ok].max() <= 2.0 ** -25
    assert np.abs(x64 - hi64).max() > 0 and np.any(hi64 > x64) and np.any(hi64 < x64)    # two-sided, unlike f16_rtz


def _pieces(v):
    """fp32 values -> high + low fp16 piece of split2_rtn, summed in float64 (what the four piece products of a dW sum to)"""
    hi = v.half()
    return hi.double() + (v - hi.float()).half().double()


def _dy_exponents(dy):
    """-> (live samples, e(n) = floor(log2 |dy[n]|) of the live ones, e_max)"""
    dy = torch.as_tensor(dy, dtype=torch.float32).reshape(-1)
    live = dy != 0
    e = torch.frexp(dy[live]).exponent.long() - 1          # dy = m 2^e', m in [0.5, 1)
    return live, e, int(e.max())


def dw_db_model(h, dz, dy, h_prescale_exp=8):
    """One layer's parameter-gradient products of mlp_bwd_split_f16_kernel restated: h [N, K] fp32-valued layer input, dz
    [N, 64] float64 gradient at the layer's pre-activation, dy [N] fp32 upstream gradient -> (worst |model - exact| / S of dW
    over the entries with S > 0, S = |dZ|^T |H|; the same for db, S = sum |dZ|).
      H side : h * 2^h_prescale_exp * 2^(e(n) - e_max), e(n) = floor(log2 |dy[n]|), e_max that of the launch's largest |dy|
               (exact scaling, fp32 keeps what it can), split into two fp16 pieces, nearest, subnormals kept;
      dZ side: the chain runs on the mantissa of dy[n] scaled into [16, 32): dz * 2^(4 - e(n)), rounded to fp32, split alike;
      all four piece products kept (summed exactly here: the model carries neither the fp32 accumulation nor the error of the
      device's own dZ); db sums the dZ pieces times 2^h_prescale_exp 2^(e(n) - e_max); the summing launch takes 2^(e_max - 4)
      and the pre-scale out again (exact).
    Samples with dy == 0 contribute nothing."""
    live, e, e_max = _dy_exponents(dy)
    h = torch.as_tensor(h).float().double()[live]
    dz = torch.as_tensor(dz, dtype=torch.float64)[live]
    r = torch.exp2((h_prescale_exp + e - e_max).double())[:, None]
    A = _pieces((dz * torch.exp2((4 - e).double())[:, None]).float())
    B = _pieces((h * r).float())
    back = 2.0 ** (e_max - 4 - h_prescale_exp)
    out = []
    for got, exact, S in ((A.t() @ B * back, dz.t() @ h, dz.abs().t() @ h.abs()), ((A * r).sum(0) * back, dz.sum(0), dz.abs().sum(0))):
        ok = S > 0
        out.append(float(((got - exact).abs()[ok] / S[ok]).max()) if bool(ok.any()) else 0.0)
    return tuple(out)


def dw1_model(x, dz1, dy, h_prescale_exp=8):
    """worst |err| / S over the entries of dW1 with S > 0, from the fp32 inputs x [N, K0], the float64 dZ1 [N, 64] and dy [N]"""
    return dw_db_model(x, dz1, dy, h_prescale_exp)[0]


def parameter_gradient_model(lin, x, gy, h_prescale_exp=8):
    """-> {dW1, db1, dW2, db2, dW3, db3, dW4: model figure} of a BASELINE-net case from its float64 trace.  dW4 = sum dy h3 runs
    in fp32 on the two pieces of h3 as they are (no scaling)."""
    _, _, _, _, H, dZ = M._f64_trace(lin, x, gy)
    out = {}
    for l in range(3):
        out["dW%d" % (l + 1)], out["db%d" % (l + 1)] = dw_db_model(H[l], dZ[l], gy, h_prescale_exp)
    dy, h3 = gy.double().reshape(-1, 1), H[3]
    S = (dy.abs() * h3.abs()).sum(0)
    out["dW4"] = float((((dy * (_pieces(h3.float()) - h3)).sum(0)).abs() / S.clamp_min(1e-300)).max())
    return out


def model_of(lin, x, gy, **kw):
    """dw1_model on the float64 dZ1 of a case"""
    return dw1_model(x, M._f64_pass(lin, x, gy)[4], gy, **kw)


@pytest.mark.parametrize("K0", [36, 52])
def test_f64_pass_equals_float64_autograd(K0):
    """the hand-written float64 pass of tests/mlp_float64.py against torch autograd in float64, 1e-12 of the largest entry of
    each tensor, at N = 257; the S of a column that is exactly zero (the closed levels, the zero column) is exactly 0"""
    N = 257
    gen = torch.Generator().manual_seed(K0)
    lin = M.sdf_net(K0, K0)
    x = M.sdf_inputs(K0, N, 1e-5, 6, gen)
    gy = M.sdf_dy(N, "six_decades", gen)
    y, SY, g, s, dz1 = M._f64_pass(lin, x, gy)
    x64 = x.double().requires_grad_(True)
    l64 = [torch.nn.Linear(l.in_features, l.out_features).double() for l in lin]
    for a, b in zip(l64, lin):
        a.weight.data.copy_(b.weight.data)
        a.bias.data.copy_(b.bias.data)
    h, z1 = x64, None
    for i, l in enumerate(l64):
        h = l(h)
        if i == 0:
            z1 = h
            z1.retain_grad()
        if i < 3:
            h = torch.nn.functional.gelu(h)
    h.backward(gy.double())
    ref = {"dX": x64.grad}
    for i, l in enumerate(l64):
        ref["dW%d" % (i + 1)], ref["db%d" % (i + 1)] = l.weight.grad, l.bias.grad
    rel = lambda a, b: float((a - b).abs().max()) / float(b.abs().max())
    assert rel(y, h.detach()) <= 1e-12 and rel(dz1, z1.grad) <= 1e-12
    assert sorted(g) == sorted(ref)
    for k in ref:
        assert g[k].shape == ref[k].shape == s[k].shape and rel(g[k], ref[k]) <= 1e-12, k
        assert bool((s[k] >= g[k].abs()).all()), k                      # an absolute sum bounds its sum
    L = M.sdf_levels(K0)
    zero_cols = list(range(2 * (L - 6), 2 * L)) + [K0 - 1]
    assert bool((x[:, zero_cols] == 0).all()) and bool((x[:, :2 * (L - 6)] != 0).any(0).all())
    assert bool((s["dW1"][:, zero_cols] == 0).all()) and bool((g["dW1"][:, zero_cols] == 0).all())
    assert bool((s["dW1"][:, :2 * (L - 6)] > 0).all())
    miss = gy.view(-1) == 0
    assert int(miss.sum()) == len(range(5, N, 16)) and bool((s["dX"][miss] == 0).all()) and bool((s["dX"][~miss] > 0).all())


MODEL_BAR = 5e-6          # a quarter of the 2e-5 the device is held to


def test_dw1_model_equals_a_sum_over_the_piece_products_in_numpy():
    """the torch form above against the four piece products written out with numpy's fp16 (split2_rtn)"""
    lin, x, gy = M.geometry_case(36, 65)
    gy = gy * 10.0 ** (-6.0 * torch.rand(65, 1, generator=torch.Generator().manual_seed(1)))
    dz1 = M._f64_pass(lin, x, gy)[4].numpy()
    _, e = np.frexp(gy.numpy().reshape(-1))
    e = e.astype(np.int64) - 1
    a0, a1 = (p.astype(np.float64) for p in split2_rtn((dz1 * 2.0 ** (4 - e)[:, None]).astype(np.float32)))
    b0, b1 = (p.astype(np.float64) for p in split2_rtn((x.numpy().astype(np.float64) * 2.0 ** (8 + e - e.max())[:, None]).astype(np.float32)))
    got = (a1.T @ b1 + a1.T @ b0 + a0.T @ b1 + a0.T @ b0) * 2.0 ** (int(e.max()) - 12)
    S = np.abs(dz1).T @ np.abs(x.numpy().astype(np.float64))
    fig = (np.abs(got - dz1.T @ x.numpy().astype(np.float64))[S > 0] / S[S > 0]).max()
    assert abs(fig - dw1_model(x, dz1, gy)) <= 1e-3 * fig and fig > 0


@pytest.mark.parametrize("K0,lattice,dy", [c for c in M.NUMERICS_CASES if c != M.MODEL_BOUNDED])
def test_dw1_model_holds_the_numerics_cases_with_a_factor_of_four_in_hand(K0, lattice, dy):
    """every numerics case tests/test_gpu_mlp_baseline_numerics.py asserts at 2e-5 per entry: the arithmetic alone, on the same
    seeds and inputs, stays within 5e-6"""
    m = model_of(*M.numerics_case(K0, lattice, dy))
    print("dW1 model K0=%d lattice=%g dy=%s: %.1e" % (K0, lattice, dy, m))
    assert m <= MODEL_BAR, m


def test_dw1_model_holds_the_geometry_cases_with_a_factor_of_four_in_hand():
    """the geometry cases above TINY_BATCH are asserted at 2e-5 and pass the model like the numerics cases; the others take
    max(2e-5, 4 x model) per parameter gradient (an entry is a sum of so few products that one small operand decides it): their
    model figures are printed"""
    worst, tiny = {}, {}
    for K0, N in M.GEOMETRY_CASES:
        case = M.geometry_case(K0, N)
        if N > M.TINY_BATCH:
            worst[(K0, N)] = model_of(*case)
        else:
            tiny[(K0, N)] = parameter_gradient_model(*case)
    print("dW1 model, geometry cases: " + " ".join("%d/%d %.1e" % (k + (v,)) for k, v in worst.items()))
    for k, v in tiny.items():
        print("   model of the tiny batch %d/%d: " % k + " ".join("%s %.1e" % kv for kv in v.items()))
    assert worst and max(worst.values()) <= MODEL_BAR, worst
    assert all(np.isfinite(f) for v in tiny.values() for f in v.values())


def test_dw1_model_documents_the_limit_under_an_outlier_at_initialisation_scale():
    """Lattice features of 1e-5, dY over six decades and one sample at 50x the largest: e_max belongs to the outlier, and the
    H-side operand of every other sample -- 1e-5 * 2^8 * 2^(e(n) - e_max) -- sits at or below fp16's subnormal spacing 2^-24.
    The 2^8 pre-scale (H_PRESCALE_EXP) does not hold 2e-5 per entry of the lattice columns of dW1 there; the GPU test takes its
    bar for this one tensor of this one case from the model.  Whoever raises the pre-scale (a separate, larger one for the
    layer-0 operand, as PRE_X of csrc/mlp_wide.hip) sees here that the limit moved."""
    lin, x, gy = M.numerics_case(*M.MODEL_BOUNDED)
    m8 = model_of(lin, x, gy)
    m0, m14 = model_of(lin, x, gy, h_prescale_exp=0), model_of(lin, x, gy, h_prescale_exp=14)
    print("dW1 model, outlier at lattice 1e-5, N=%d: pre-scale 2^8 %.1e, none %.1e, 2^14 %.1e" % (M.N_NUMERICS, m8, m0, m14))
    assert m8 > 2e-5
    assert m0 > m8 > m14
