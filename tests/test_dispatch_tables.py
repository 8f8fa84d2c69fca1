"""Which MLP widths have a fused kernel: psdf_mlp_supported (include/psdf.h), computed from the one dispatch table of
csrc/mlp_dispatch.h, is pinned here against an explicit table (CPU), and on the GPU against what the entry points do for
every shape of the sweep (a kernel where it says 1, -2 without a launch where it says 0)."""
import ctypes
import functools
import itertools
import pytest

from permuto_sdf_amd import mlp as M

# boundary values around every tile edge, and the real nets' 36, 52 and 111, for every layer
VALUES = (1, 16, 17, 32, 33, 36, 48, 49, 52, 64, 65, 80, 81, 111, 112, 113, 128, 129)
OPS = (M.OP_FORWARD, M.OP_FORWARD_F16, M.OP_FORWARD_WIDE_F16, M.OP_BACKWARD, M.OP_BACKWARD_DATA, M.OP_BACKWARD_DATA_MASKED,
       M.OP_DOUBLE_BACKWARD, M.OP_DOUBLE_BACKWARD_PLUS)


def _sweep():
    for n_layers in (3, 4):
        yield from itertools.product(VALUES, repeat=n_layers + 1)


def _sig16(d):
    t = [(x + 15) // 16 for x in d]
    return (t[0], t[1], t[2], t[3] if len(d) == 5 else 0, t[-1], d[-1] <= 4)


def _sig32(d):
    t = [(x + 31) // 32 for x in d]
    return (t[1], t[2], t[3] if len(d) == 5 else 0, t[-1], d[-1] <= 4)


# single-wave instantiations, by tile signature (16-wide tiles: ti0, t1, t2, t3, to, outputs <= 4)
BWD_DW = {(3, 4, 4, 4, 1, True), (4, 4, 4, 4, 1, True), (2, 4, 4, 4, 1, True), (4, 2, 2, 2, 1, True), (3, 2, 2, 2, 1, True),
          (2, 2, 2, 2, 1, True), (4, 2, 2, 2, 3, False), (3, 2, 2, 2, 3, False), (5, 4, 4, 0, 1, True)}
BWD_DX = BWD_DW | {(4, 4, 4, 4, 5, False), (4, 4, 4, 4, 3, False), (3, 4, 4, 4, 3, False)}
BWD_MASKED = {(3, 4, 4, 4, 1, True), (4, 4, 4, 4, 1, True), (2, 4, 4, 4, 1, True), (4, 2, 2, 2, 1, True), (3, 2, 2, 2, 1, True),
              (2, 2, 2, 2, 1, True)}
DBL = {(4, 2, 2, 2, 3, False), (3, 2, 2, 2, 3, False), (4, 2, 2, 2, 1, True), (3, 2, 2, 2, 1, True), (2, 2, 2, 2, 1, True),
       (3, 4, 4, 4, 1, True), (4, 4, 4, 4, 1, True)}
DBL_PLUS = {(4, 2, 2, 2, 3, False), (3, 2, 2, 2, 3, False)}
# 32-wide tiles: t1, t2, t3, to, outputs <= 4
FWD = {(2, 2, 2, 1, True), (1, 1, 1, 1, True), (1, 1, 1, 2, False), (2, 2, 2, 3, False), (2, 2, 2, 2, False), (2, 2, 0, 1, True),
       (4, 4, 2, 1, True)}


# the workgroup-cooperative kernels of mlp_wide.hip, by width
def _colour(d):
    return len(d) == 5 and d[0] <= 112 and d[1] <= 128 and d[2] <= 128 and d[3] <= 64 and d[4] <= 16 and not (d[1] <= 64 and d[2] <= 64)


def _density(d):
    return len(d) == 5 and d[0] <= 64 and all(32 < x <= 64 for x in d[1:4]) and 16 < d[4] <= 80


def _colour_head(d):
    return len(d) == 4 and 64 < d[0] <= 80 and 48 < d[1] <= 64 and 48 < d[2] <= 64 and d[3] <= 4


EXPECTED = {
    M.OP_FORWARD: lambda d: _sig32(d) in FWD,
    M.OP_FORWARD_F16: lambda d: len(d) == 5 and d[0] <= 64 and d[1] == d[2] == d[3] == 64 and d[4] <= 4,
    M.OP_FORWARD_WIDE_F16: lambda d: _colour(d) or _density(d),
    M.OP_BACKWARD: lambda d: _sig16(d) in BWD_DW or _colour(d) or _density(d) or _colour_head(d),
    M.OP_BACKWARD_DATA: lambda d: _sig16(d) in BWD_DX,
    M.OP_BACKWARD_DATA_MASKED: lambda d: _sig16(d) in BWD_MASKED,
    M.OP_DOUBLE_BACKWARD: lambda d: _sig16(d) in DBL,
    M.OP_DOUBLE_BACKWARD_PLUS: lambda d: _sig16(d) in DBL_PLUS,
}
# in the table by signature, declined because the launch would need more than the 160 KB of LDS a launch may use: the fp32
# forward of the colour net's tiles with 128 or more inputs (its weight image), and the double backward of the
# 49..64-input BASELINE net (weight images and staging: built, never launched)
LDS_DECLINED = {M.OP_FORWARD: {d for d in _sweep() if _sig32(d) == (4, 4, 2, 1, True) and d[0] >= 128},
                M.OP_DOUBLE_BACKWARD: {d for d in _sweep() if _sig16(d) == (4, 4, 4, 4, 1, True)}}


@functools.lru_cache(maxsize=None)
def _answers():
    """{op: set of swept widths the library answers 1 for}; every answer is 0 or 1"""
    from permuto_sdf_amd import _lib as L
    q = L.lib().psdf_mlp_supported
    q.restype = ctypes.c_int
    q.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    arr = (ctypes.c_int * 5)()
    yes = {op: set() for op in OPS}
    for d in _sweep():
        arr[:len(d)] = d
        for op in OPS:
            r = q(op, len(d) - 1, arr)
            assert r in (0, 1), (op, d, r)
            if r:
                yes[op].add(d)
    return yes


def test_query_is_the_explicit_table():
    """every operation, every swept width: the compiled library's answer is the table above"""
    wrong = {}
    for op in OPS:
        expected = {d for d in _sweep() if EXPECTED[op](d)}
        declined = LDS_DECLINED.get(op, set())
        assert declined <= expected
        got = _answers()[op]
        if got != expected - declined:
            wrong[op] = (sorted(got - expected)[:8], sorted(expected - declined - got)[:8])
    assert not wrong, wrong


def test_query_argument_errors():
    from permuto_sdf_amd import _lib as L
    q = L.lib().psdf_mlp_supported
    d5 = (ctypes.c_int * 5)(36, 64, 64, 64, 1)
    assert q(M.OP_BACKWARD, 4, d5) == 1
    assert q(8, 4, d5) == -1 and q(-1, 4, d5) == -1 and q(M.OP_BACKWARD, 4, None) == -1
    assert q(M.OP_BACKWARD, 1, d5) == -1 and q(M.OP_BACKWARD, 6, d5) == -1
    assert q(M.OP_FORWARD, 4, (ctypes.c_int * 5)(36, 0, 64, 64, 1)) == -1
    assert q(M.OP_FORWARD, 2, (ctypes.c_int * 3)(36, 64, 1)) == 0          # a valid net without an instantiation


def test_predicates_on_the_nets_of_the_reference():
    from permuto_sdf_amd.mlp import backward_supported, double_backward_supported
    assert backward_supported([52, 32, 32, 32, 33]) and double_backward_supported([52, 32, 32, 32, 33])   # SDF net
    assert backward_supported([36, 64, 64, 64, 1]) and double_backward_supported([36, 64, 64, 64, 1])     # BASELINE net
    assert backward_supported([52, 64, 64, 64, 65]) and backward_supported([80, 64, 64, 3])               # background nets
    from permuto_sdf_amd.mlp import double_backward_plus_supported
    assert double_backward_plus_supported([52, 32, 32, 32, 33]) and double_backward_plus_supported([36, 32, 32, 32, 33])
    assert not double_backward_plus_supported([36, 64, 64, 64, 1]) and not double_backward_plus_supported([52, 32, 32, 32, 1])
    assert backward_supported([112, 128, 128, 64, 3]) and backward_supported([111, 128, 128, 64, 3])     # colour net: mlp_wide.hip
    assert not backward_supported([200, 256, 256, 64, 3]) and not double_backward_supported([112, 128, 128, 64, 3])
    assert not double_backward_supported([80, 64, 64, 3])


def test_routes_of_the_nets_this_project_and_the_reference_build():
    from permuto_sdf_amd.reference_fusion import forward_supported
    for d in ([36, 32, 32, 32, 33], [52, 32, 32, 32, 33], [36, 64, 64, 64, 1], [52, 64, 64, 64, 1], [111, 128, 128, 64, 3],
              [52, 64, 64, 64, 65], [80, 64, 64, 3]):
        assert forward_supported(d) and M.backward_supported(d), d
    assert M.f16_forward_supported([36, 64, 64, 64, 1]) and M.f16_forward_supported([52, 64, 64, 64, 1])
    assert not M.f16_forward_supported([52, 32, 32, 32, 33])
    assert M.supported(M.OP_FORWARD_WIDE_F16, [111, 128, 128, 64, 3]) and M.supported(M.OP_FORWARD_WIDE_F16, [52, 64, 64, 64, 65])
    assert not M.supported(M.OP_FORWARD_WIDE_F16, [52, 32, 32, 32, 33]) and not M.supported(M.OP_FORWARD_WIDE_F16, [80, 64, 64, 3])
    assert not M.supported(M.OP_BACKWARD_DATA, [111, 128, 128, 64, 3])       # its data gradient comes with the dW launch


def _ref64(dims, x, ws, bs):
    """float64 torch evaluation of the Linear/GELU stack, [N, d0] -> [N, dn]"""
    import torch
    h = x
    for i in range(len(ws)):
        h = torch.nn.functional.linear(h, ws[i], bs[i])
        if i < len(ws) - 1:
            h = torch.nn.functional.gelu(h)
    return h


def _close(got, ref, ref32, bar):
    """the bar of tests/test_gpu_mlp.py: within 4x torch's own fp32 error, or `bar` of the largest entry"""
    import torch
    assert bool(torch.isfinite(got).all())
    scale = max(1e-6, ref.abs().max().item())
    err, err32 = ((t.double() - ref).abs().max().item() / scale for t in (got, ref32))
    assert err <= max(4 * err32, bar), (err, err32, bar)


def _torch_results(op, dims, x, ws, bs, gy, v, gy2):
    """what the entry point of `op` computes, by torch autograd in the dtype of the arguments ([N, C] layout)"""
    import torch
    nl = len(ws)
    leaves = [t.clone().requires_grad_(True) for t in [x] + ws + bs]
    y = _ref64(dims, leaves[0], leaves[1:1 + nl], leaves[1 + nl:])
    if op in (M.OP_FORWARD, M.OP_FORWARD_F16, M.OP_FORWARD_WIDE_F16):
        return [y.detach()]
    if op in (M.OP_DOUBLE_BACKWARD, M.OP_DOUBLE_BACKWARD_PLUS):
        (gx,) = torch.autograd.grad(y, leaves[0], gy, create_graph=True)
        r = torch.autograd.grad(gx, leaves, v, retain_graph=True, allow_unused=True)
        r = [a if a is not None else torch.zeros_like(t) for a, t in zip(r, leaves)]     # (the last bias: no term)
        if gy2 is not None:
            r = [a + b for a, b in zip(r, torch.autograd.grad(y, leaves, gy2))]
        return r
    r = torch.autograd.grad(y, leaves, gy)
    return list(r) if op == M.OP_BACKWARD else [r[0]]


def _run_supported(op, dims, N, dev, gen):
    """call the entry point of `op` once on real tensors: rc 0 (else the wrapper raises), finite outputs, float64 agreement"""
    import torch
    from permuto_sdf_amd import _lib as L
    nl = len(dims) - 1
    rnd = lambda *s: (torch.rand(*s, generator=gen, dtype=torch.float64) * 2 - 1).to(dev)
    ws64 = [rnd(dims[i + 1], dims[i]) * (6.0 / (dims[i] + dims[i + 1])) ** 0.5 for i in range(nl)]
    bs64 = [rnd(dims[i + 1]) * 0.1 for i in range(nl)]
    x64, gy64, v64 = rnd(N, dims[0]), rnd(N, dims[-1]), rnd(N, dims[0])
    gy2_64 = rnd(N, dims[-1]) if op == M.OP_DOUBLE_BACKWARD_PLUS else None
    f32 = lambda t: None if t is None else t.float().contiguous()
    ws, bs = [f32(w) for w in ws64], [f32(b) for b in bs64]
    fm = lambda t: None if t is None else t.float().t().contiguous()
    x_fm, gy_fm = fm(x64), fm(gy64)
    if op == M.OP_FORWARD_WIDE_F16:
        got = [M.mlp_forward_wide_f16_raw(dims, x_fm, ws, bs)]
        assert got[0] is not None
    elif op in (M.OP_FORWARD, M.OP_FORWARD_F16):
        f16 = op == M.OP_FORWARD_F16
        got = [M.mlp_forward_raw(dims, x_fm, M.pack_params(dims, ws, bs, f16=f16), f16=f16)]
    elif op in (M.OP_DOUBLE_BACKWARD, M.OP_DOUBLE_BACKWARD_PLUS):
        dx, dWs, dbs = M.mlp_double_backward(dims, x_fm, ws, bs, gy_fm, fm(v64), gy2_fm=fm(gy2_64))
        got = [dx] + list(dWs) + list(dbs)
    elif op == M.OP_BACKWARD:
        dx, dWs, dbs = M.mlp_backward_raw(dims, x_fm, ws, bs, gy_fm)
        got = [dx] + list(dWs) + list(dbs)
    elif op == M.OP_BACKWARD_DATA:
        got = [M.mlp_backward_raw(dims, x_fm, ws, bs, gy_fm, need_dw=False)[0]]
    else:
        dx = torch.empty(dims[0], N, device=dev)
        skip = torch.zeros(N, dtype=torch.uint8, device=dev)
        arr = lambda ts: (ctypes.c_void_p * nl)(*[t.data_ptr() for t in ts])
        L.call("psdf_mlp_backward_data_masked", L.c_i(nl), M._dims_array(dims), L.c_l(N), L.ptr(x_fm), arr(ws), arr(bs),
               L.ptr(gy_fm), L.ptr(skip), L.ptr(dx), L.stream())
        got = [dx]
    got[0] = got[0].t()                 # feature-major -> [N, C]
    r64 = _torch_results(op, dims, x64, ws64, bs64, gy64, v64, gy2_64)
    if op in (M.OP_BACKWARD, M.OP_BACKWARD_DATA, M.OP_BACKWARD_DATA_MASKED):
        # per entry, relative to the sum of the magnitudes of the terms of its last product (tests/test_gpu_mlp_wide_numerics.py):
        # 2e-5 for the fp32 single-wave kernels.  The split-fp16 workgroup kernel of mlp_wide.hip (path 3) holds 2e-5 on the
        # reference's nets and their data (test_gpu_mlp_wide_numerics.py, test_gpu_mlp.py pin that); on arbitrary swept widths and
        # uniform data its two fp16 pieces reach a few 1e-3, and up to 2e-2 on colour-net widths with a one-wide layer (values
        # deep in the pieces' subnormal range).  Held to 5e-2 here -- far from the errors of order 1 of a wrong
        # instantiation, which is what this test is about; the worst errors are printed
        wide = op == M.OP_BACKWARD and L.lib().psdf_last_path(1) == 3
        bar = 5e-2 if wide else 2e-5
        worst = 0.0
        for g, r, S in zip(got, r64, _term_sums(dims, x64, ws64, bs64, gy64)):
            assert bool(torch.isfinite(g).all())
            d = (g.double() - r).abs()
            assert not bool(((S == 0) & (d != 0)).any())
            worst = max(worst, float(torch.where(S > 0, d / S.clamp_min(1e-300), torch.zeros_like(d)).max()))
        assert worst <= bar, (worst, bar)
        return worst if wide else 0.0
    r32 = _torch_results(op, dims, f32(x64), ws, bs, f32(gy64), f32(v64), f32(gy2_64))
    bar = 2e-5 if op in (M.OP_FORWARD, M.OP_FORWARD_F16, M.OP_FORWARD_WIDE_F16) else 2e-4
    for g, r, t in zip(got, r64, r32):
        _close(g, r, t, bar)


def _term_sums(dims, x, ws, bs, gy):
    """[dX, dW_l.., db_l..] of sum |terms| (float64): dX = |dZ_0| |W_0|, dW_l = |dZ_l|^T |H_l|, db_l = sum_n |dZ_l|"""
    import torch
    nl = len(ws)
    H, Z = [x], []
    for i in range(nl):
        Z.append(torch.nn.functional.linear(H[-1], ws[i], bs[i]).requires_grad_(True))
        H.append(torch.nn.functional.gelu(Z[-1]) if i < nl - 1 else Z[-1])
    dZ = torch.autograd.grad(H[-1], Z, gy)
    return ([dZ[0].abs() @ ws[0].abs()] + [dZ[l].abs().t() @ H[l].detach().abs() for l in range(nl)] +
            [dZ[l].abs().sum(0) for l in range(nl)])


@pytest.mark.gpu
def test_query_is_what_the_entry_points_do():
    """For every shape of the sweep and every operation: where the query says 0 the entry point returns -2 and writes nothing (N = 64,
    buffers large enough for any swept width); where it says 1 the entry point runs and agrees with float64 torch -- once per
    kernel configuration (the 16-wide tiles of every layer, outputs <= 4, and for the two table-driven forwards the input width)"""
    import torch
    from permuto_sdf_amd import _lib as L
    dev = torch.device("cuda")
    lib, N, Wmax = L.lib(), 64, max(VALUES)
    sentinel = 7.0
    X = torch.rand(Wmax, N, device=dev)
    dY, V, dY2 = (torch.rand(Wmax, N, device=dev) for _ in range(3))
    packed = torch.zeros(1 << 18, device=dev)
    skip = torch.zeros(N, dtype=torch.uint8, device=dev)
    params = [torch.rand(Wmax * Wmax, device=dev) for _ in range(8)]
    outs = [torch.full((Wmax * Wmax,), sentinel, device=dev) for _ in range(8)]
    Y = torch.full((Wmax, N), sentinel, device=dev)
    P = lambda ts: (ctypes.c_void_p * 4)(*[t.data_ptr() for t in ts])
    Wp, Bp, dWp, dbp = P(params[:4]), P(params[4:]), P(outs[:4]), P(outs[4:])
    x, y, dy, v, dy2, pk, sk = (ctypes.c_void_p(t.data_ptr()) for t in (X, Y, dY, V, dY2, packed, skip))
    n, st = ctypes.c_int64(N), L.stream()
    f = {name: getattr(lib, name) for name in ("psdf_mlp_forward", "psdf_mlp_forward_f16", "psdf_mlp_forward_wide_f16",
                                               "psdf_mlp_backward", "psdf_mlp_backward_data_masked", "psdf_mlp_double_backward",
                                               "psdf_mlp_double_backward_plus")}
    calls = {
        M.OP_FORWARD: lambda nl, d: f["psdf_mlp_forward"](nl, d, n, x, pk, y, st),
        M.OP_FORWARD_F16: lambda nl, d: f["psdf_mlp_forward_f16"](nl, d, n, x, pk, y, st),
        M.OP_FORWARD_WIDE_F16: lambda nl, d: f["psdf_mlp_forward_wide_f16"](nl, d, n, x, Wp, Bp, y, st),
        M.OP_BACKWARD: lambda nl, d: f["psdf_mlp_backward"](nl, d, n, x, Wp, Bp, dy, y, dWp, dbp, st),
        M.OP_BACKWARD_DATA: lambda nl, d: f["psdf_mlp_backward"](nl, d, n, x, Wp, Bp, dy, y, None, None, st),
        M.OP_BACKWARD_DATA_MASKED: lambda nl, d: f["psdf_mlp_backward_data_masked"](nl, d, n, x, Wp, Bp, dy, sk, y, st),
        M.OP_DOUBLE_BACKWARD: lambda nl, d: f["psdf_mlp_double_backward"](nl, d, n, x, Wp, Bp, dy, v, y, dWp, dbp, st),
        M.OP_DOUBLE_BACKWARD_PLUS: lambda nl, d: f["psdf_mlp_double_backward_plus"](nl, d, n, x, Wp, Bp, dy, v, dy2, y, dWp, dbp,
                                                                                     st),
    }
    yes = _answers()
    arr = (ctypes.c_int * 5)()
    declined = 0
    for d in _sweep():
        arr[:len(d)] = d
        for op in OPS:
            if d not in yes[op]:
                rc = calls[op](len(d) - 1, arr)
                assert rc == -2, (op, d, rc)
                declined += 1
    torch.cuda.synchronize()
    assert bool((Y == sentinel).all()) and all(bool((t == sentinel).all()) for t in outs), "a declined call wrote its outputs"
    gen = torch.Generator().manual_seed(0)
    seen, ran, wide_worst = set(), 0, []
    for op in OPS:
        for d in sorted(yes[op]):
            key = (op, tuple((w + 15) // 16 for w in d), d[-1] <= 4, d[0] if op in (M.OP_FORWARD, M.OP_FORWARD_F16) else 0)
            if key in seen:
                continue
            seen.add(key)
            try:
                wide_worst.append((_run_supported(op, list(d), N, dev, gen) or 0.0, d))
            except Exception as e:
                raise AssertionError((op, d, repr(e)))
            ran += 1
    torch.cuda.synchronize()
    print("declined calls %d, launched configurations %d; split-fp16 wide backward, worst per-entry "
          "errors: %s" % (declined, ran, sorted(wide_worst)[-4:]))
