"""Layer-0 operand loads and operand split of the split forward kernels (csrc/mlp.hip, mlp_fwd_split_tiles): a load is a scalar
row base plus one 32-bit per-lane byte offset, the partial last k-step reads clamped rows and selects zeros, and the two-piece
split is v_cvt_pk_f16_f32 + v_fma_mixlo/hi_f16.

Nets: [K0, 64, 64, 64, 1] with K0 = 32, 48, 64 (whole k-steps only), 35, 36, 52 (a partial last k-step of 3 or 4 rows: half 0
of the wave alone has rows) and 44 (12 rows: half 0 whole, four rows in half 1 -- the third form of the k-step), with two fp16
pieces and with three bf16 pieces, and [36, 64, 64, 1] (bf16 pieces: the only form that net has).  Batch sizes 1, 31, 32, 33,
95, 4099: ragged tiles, N not a multiple of 4, and 129 tiles = more than the waves of one workgroup.  Every batch is a prefix
of the largest, so one float64 evaluation per net serves all of them.

For every shape the four-wave and the eight-wave form must give the same bytes, and the output must be within the existing
float64 bars: 4e-6 of the largest output with fp16 pieces (what bench.py quotes), max(4 x the error of torch's own fp32
evaluation, 2e-6 of the largest output) with bf16 pieces (tests/test_gpu_mlp.py::test_split_bf16_forward_keeps_fp32_accuracy).
X and Y sit inside larger buffers: the floats around Y hold a sentinel that must survive, everything around X -- the rows
K0.. above all -- holds NaN, so that a load of a padding row shows up in Y (0 x NaN) instead of passing silently, and X is
tried 16-byte aligned and four bytes off."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = 7.0
SIZES = (1, 31, 32, 33, 95, 4099)
NETS = ([([K0, 64, 64, 64, 1], f16) for K0 in (32, 35, 36, 44, 48, 52, 64) for f16 in (True, False)]
        + [([36, 64, 64, 1], False)])


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda")


@pytest.fixture(autouse=True)
def _policy_restored():
    from permuto_sdf_amd.mlp import set_forward_form
    yield
    set_forward_form(0)


def _net(dims, seed):
    torch.manual_seed(seed)
    nl = len(dims) - 1
    mods = []
    for i in range(nl):
        mods.append(torch.nn.Linear(dims[i], dims[i + 1]))
        if i < nl - 1:
            mods.append(torch.nn.GELU())
    return torch.nn.Sequential(*mods)


def _embedded_x(x_fm, lead):
    """x_fm [K0, N] as a view into a NaN-filled buffer: `lead` floats in front, sixteen more rows behind"""
    K0, N = x_fm.shape
    buf = torch.full((lead + (K0 + 16) * N,), float("nan"), dtype=torch.float32, device=x_fm.device)
    view = buf[lead:lead + K0 * N].view(K0, N)
    view.copy_(x_fm)
    assert view.is_contiguous() and (view.data_ptr() % 16 == 0) == (lead % 4 == 0)
    return buf, view


def _forward(dims, x_view, packed, f16, form, skip=None):
    """-> (y [OUT, N], the sentinel floats in front of it, those behind it)"""
    from permuto_sdf_amd import _lib as L
    from permuto_sdf_amd.mlp import _dims_array, last_forward_form, set_forward_form
    N, OUT = x_view.shape[1], dims[-1]
    guard = N + 3
    ybuf = torch.full((guard + OUT * N + guard,), SENTINEL, dtype=torch.float32, device=x_view.device)
    y = ybuf[guard:guard + OUT * N].view(OUT, N)
    lib = L.lib()
    set_forward_form(form)
    try:
        args = [L.c_i(len(dims) - 1), _dims_array(dims), L.c_l(N), L.ptr(x_view), L.ptr(packed)]
        if f16:
            rc = lib.psdf_mlp_forward_f16(*args, L.ptr(y), L.stream())
        elif skip is None:
            rc = lib.psdf_mlp_forward(*args, L.ptr(y), L.stream())
        else:
            rc = lib.psdf_mlp_forward_masked(*args, L.ptr(skip), L.ptr(y), L.stream())
        torch.cuda.synchronize()
        assert int(rc) == 0 and last_forward_form() == form, (rc, form)
    finally:
        set_forward_form(0)
    return y, ybuf[:guard], ybuf[guard + OUT * N:]


@pytest.mark.parametrize("dims,f16", NETS, ids=lambda v: "-".join(map(str, v)) if isinstance(v, list) else ("f16" if v else "bf16"))
def test_operand_loads_stay_inside_the_input_and_forms_agree(dev, dims, f16):
    from permuto_sdf_amd.mlp import pack_params
    K0 = dims[0]
    ref = _net(dims, 300 + K0 + len(dims))
    x = torch.randn(max(SIZES), K0)
    x[:, K0 // 2:] *= 1e-3
    with torch.no_grad():
        y64 = copy.deepcopy(ref).double()(x.double())[:, 0]          # once for every batch size
        err_t32 = float((ref(x)[:, 0].double() - y64).abs().max())   # torch's own fp32 evaluation (the bf16 bar)
    y64 = y64.to(dev)
    lin = [m for m in ref.to(dev) if isinstance(m, torch.nn.Linear)]
    packed = pack_params(dims, [l.weight for l in lin], [l.bias for l in lin], f16=f16)
    x = x.to(dev)
    for N in SIZES:
        x_fm = x[:N].t().contiguous()
        scale = float(y64[:N].abs().max())
        bar = 4e-6 * scale if f16 else max(4.0 * err_t32, 2e-6 * scale)
        for lead in (4, 1):                                          # 16-byte aligned, and four bytes off
            xbuf, xv = _embedded_x(x_fm, lead)
            y4, front4, back4 = _forward(dims, xv, packed, f16, 4)
            y8, front8, back8 = _forward(dims, xv, packed, f16, 8)
            for front, back in ((front4, back4), (front8, back8)):
                assert bool((front == SENTINEL).all()) and bool((back == SENTINEL).all()), (N, lead, "wrote outside Y")
            assert bool(torch.isfinite(y4).all()), (N, lead, "a load outside [X, X + K0 N) reached the output")
            assert torch.equal(y4.view(torch.int32), y8.view(torch.int32)), (N, lead, "forms differ")
            err = float((y4[0].double() - y64[:N]).abs().max())
            print("dims %s %s N=%d lead=%d: error %.2e, bar %.2e" % (dims, "fp16" if f16 else "bf16", N, lead, err, bar))
            assert err <= bar, (N, lead, err, bar)
            assert bool(torch.isnan(xbuf[:lead]).all()) and bool(torch.isnan(xbuf[lead + K0 * N:]).all())


def test_masked_forward_with_embedded_operands(dev):
    """the masked entry point (bf16 pieces; the fp16 form has none) on the partial-k-step net, ragged batch, X four bytes off:
    a tile is evaluated unless every one of its samples is masked"""
    from permuto_sdf_amd.mlp import pack_params
    dims, N = [36, 64, 64, 64, 1], 4099
    ref = _net(dims, 77)
    x = torch.randn(N, 36)
    with torch.no_grad():
        y64 = copy.deepcopy(ref).double()(x.double())[:, 0].to(dev)
        err_t32 = float((ref(x)[:, 0].double().to(dev) - y64).abs().max())
    lin = [m for m in ref.to(dev) if isinstance(m, torch.nn.Linear)]
    packed = pack_params(dims, [l.weight for l in lin], [l.bias for l in lin])
    n = torch.arange(N, device=dev)
    skip = (((n // 32) % 3 == 1) | (n % 7 == 3)).to(torch.uint8)
    skip[(N - 1) // 32 * 32:] = 1                                    # the partial last tile entirely
    skip = skip.contiguous()
    pad = torch.ones((N + 31) // 32 * 32, dtype=torch.int32, device=dev)
    pad[:N] = skip
    written = (pad.view(-1, 32).min(dim=1).values == 0).repeat_interleave(32)[:N]
    xbuf, xv = _embedded_x(x.to(dev).t().contiguous(), 1)
    y4, front4, back4 = _forward(dims, xv, packed, False, 4, skip)
    y8, front8, back8 = _forward(dims, xv, packed, False, 8, skip)
    for t in (front4, back4, front8, back8):
        assert bool((t == SENTINEL).all())
    assert bool((y4[0][~written] == SENTINEL).all()), "a fully masked tile was written"
    assert torch.equal(y4.view(torch.int32), y8.view(torch.int32))
    err = float((y4[0].double() - y64)[written].abs().max())
    bar = max(4.0 * err_t32, 2e-6 * float(y64[written].abs().max()))
    print("masked: error %.2e, bar %.2e" % (err, bar))
    assert err <= bar, (err, bar)
