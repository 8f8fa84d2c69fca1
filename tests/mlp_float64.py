"""float64 reference of the Linear / GELU nets with every entry's absolute sum, and the inputs of the BASELINE SDF net
{K0 <= 64, 64, 64, 64, 1} as the encoding hands them over -- shared by the per-entry MLP tests (tests/test_gpu_mlp_wide_numerics.py,
tests/test_gpu_mlp_baseline_numerics.py) and by the host restatement of the split-fp16 arithmetic (tests/test_split_f16_numerics.py).

Per-entry metric: |ours - f64| / S with S the entry's own absolute sum in float64 (the error scale of a dot product; it does not
blow up where a sum cancels): dW_l: |dZ_l|^T |H_{l-1}|, db_l: sum |dZ_l|, dX: |dZ_1| |W_1|, Y: |h_{L-1}| |W_L|^T + |b_L|.  An entry
whose S is 0 has no non-zero term at all and must be exactly 0.

Below the baseline net: the float64 evaluator of the DOUBLE backward (f64_double_backward, with S of the last dot product only),
its input families and its case lists, for tests/test_mlp_double_backward_float64.py and
tests/test_gpu_mlp_double_backward_float64.py.

Last: the nets, batch sizes, launch arithmetic and skip patterns of the single-wave fp32-MFMA kernels in every launch form (SW_*),
for tests/test_mlp_single_wave_cases.py (host) and tests/test_gpu_mlp_single_wave_float64.py.

No test in here; everything is generated on the CPU from seeded generators, so the host tests and the GPU tests see the same
numbers."""
import torch


def _f64_trace(lin, x, gy):
    """float64 forward / backward by hand -> (Y, its absolute sum, the gradients, every entry's absolute sum S, the layer
    inputs [H_0 = X, H_1, ..], the gradients at the pre-activations [dZ_1, dZ_2, ..])"""
    Ws = [l.weight.detach().double() for l in lin]
    bs = [l.bias.detach().double() for l in lin]
    H, Z = [x.double()], []
    for i, (W, b) in enumerate(zip(Ws, bs)):
        z = H[-1] @ W.t() + b
        Z.append(z)
        if i < len(Ws) - 1:
            H.append(torch.nn.functional.gelu(z))
    y = Z[-1]
    SY = H[-1].abs() @ Ws[-1].abs().t() + bs[-1].abs()
    dz = gy.double()
    grads, sums, dZ = {}, {}, [None] * len(Ws)
    for l in range(len(Ws) - 1, -1, -1):
        dZ[l] = dz
        grads["dW%d" % (l + 1)] = dz.t() @ H[l]
        sums["dW%d" % (l + 1)] = dz.abs().t() @ H[l].abs()
        grads["db%d" % (l + 1)] = dz.sum(0)
        sums["db%d" % (l + 1)] = dz.abs().sum(0)
        dh = dz @ Ws[l]
        if l == 0:
            grads["dX"] = dh
            sums["dX"] = dz.abs() @ Ws[l].abs()
        else:
            zz = Z[l - 1]
            gp = 0.5 * (1 + torch.erf(zz / 2 ** 0.5)) + zz * torch.exp(-0.5 * zz * zz) / (2 * torch.pi) ** 0.5
            dz = dh * gp
    return y, SY, grads, sums, H, dZ


def _f64_pass(lin, x, gy):
    """float64 forward / backward by hand: Y, its absolute sum, the gradients, every entry's absolute sum S, and dZ1 (the
    gradient at the first layer's pre-activation, [N, d1])"""
    y, SY, grads, sums, _, dZ = _f64_trace(lin, x, gy)
    return y, SY, grads, sums, dZ[0]


def _per_entry(got, ref, S):
    """-> (worst |got - ref| / S over the entries with S > 0, whether an entry with S == 0 is not exactly 0)"""
    d = (got.double() - ref).abs()
    bad_zero = bool(((S == 0) & (d != 0)).any())
    e = torch.where(S > 0, d / S.clamp_min(1e-300), torch.zeros_like(d))
    return float(e.max()), bad_zero


# ---------------------------------------------------------------------------------------------------------------------------
# the BASELINE SDF net

def sdf_levels(K0):
    """hashed levels of the encoding behind a K0-wide net: 2 features per level + the two pseudo-levels of the points"""
    assert K0 % 2 == 0 and K0 >= 6
    return (K0 - 4) // 2


def sdf_inputs(K0, N, lattice, closed_levels, gen):
    """[N, K0] fp32, the input of the SDF net per layout 1 of csrc/encode_conventions.h (concat_points as zero-padded
    pseudo-levels): 2 L columns of lattice features ~ N(0, lattice) (PSDF_ENC_LATTICE_INIT_SCALE = 1e-5 at initialisation, 1e-2
    trained) with the columns of the last `closed_levels` levels exactly 0 (the coarse-to-fine window at the start of training),
    three point columns U(-1, 1) * 0.7, one column that is exactly 0.  K0 = 36: L = 16; K0 = 52: L = 24."""
    L = sdf_levels(K0)
    lat = torch.randn(N, 2 * L, generator=gen, dtype=torch.float64) * lattice
    if closed_levels:
        lat[:, 2 * (L - closed_levels):] = 0.0
    pts = (torch.rand(N, 3, generator=gen, dtype=torch.float64) * 2 - 1) * 0.7
    x = torch.cat([lat, pts, torch.zeros(N, 1, dtype=torch.float64)], 1)
    assert x.shape == (N, K0)
    return x.float()


def plain_inputs(K0, N, gen):
    """[N, K0] fp32 for the widths no encoding produces: randn, the upper half of the channels scaled by 1e-2"""
    x = torch.randn(N, K0, generator=gen)
    x[:, K0 // 2:] *= 1e-2
    return x


def sdf_net(K0, seed, out=1, hidden=64):
    """the four torch.nn.Linear of K0-64-64-64-1 with biases ~ N(0, 0.1) (as tests/test_gpu_mlp.py makes its split nets);
    out / hidden: the other widths of the double-backward rows (hidden: one width, or the three of a ragged net)"""
    torch.manual_seed(seed)
    hidden = [hidden] * 3 if isinstance(hidden, int) else list(hidden)
    assert len(hidden) == 3
    dims = [K0] + hidden + [out]
    lin = [torch.nn.Linear(dims[i], dims[i + 1]) for i in range(4)]
    for l in lin:
        torch.nn.init.normal_(l.bias, 0.0, 0.1)
    return lin


def sdf_dy(N, kind, gen, misses=True):
    """[N, 1] fp32 upstream gradient of the SDF.  "ordinary": randn; "six_decades": randn * 10^(-6 u) per sample (NeuS weights
    spread over six decades within a batch); "outlier": six decades and ONE sample at 50x the largest of the others (what the
    full-batch float64 test of tests/test_gpu_hotpath_parity.py feeds).  misses: 1 sample in 16 carries exactly 0 (rays that
    miss); the outlier is none of them."""
    gy = torch.randn(N, 1, generator=gen)
    if kind != "ordinary":
        assert kind in ("six_decades", "outlier"), kind
        gy = gy * 10.0 ** (-6.0 * torch.rand(N, 1, generator=gen))
    if misses:
        gy[5::16] = 0.0
    if kind == "outlier":
        gy[(N // 3) // 16 * 16 + 2] = 50.0 * float(gy.abs().max())
    return gy


N_NUMERICS = (1 << 18) + 19          # 262 163: what psdf_mlp_backward routes to the split kernels, ragged
# (K0, lattice scale, dY): through the production dispatch at N_NUMERICS
NUMERICS_CASES = [(K0, lattice, dy) for K0 in (36, 52) for lattice in (1e-5, 1e-2) for dy in ("ordinary", "six_decades")] + \
                 [(36, 1e-5, "outlier"), (36, 1e-2, "outlier")]
# the one numerics case whose dW1 the two-piece fp16 arithmetic cannot hold to 2e-5 per entry: that bar comes from the host model
# (tests/test_split_f16_numerics.py)
MODEL_BOUNDED = (36, 1e-5, "outlier")
# geometry cases of at most this many samples: an entry of a parameter gradient is a sum of so few products that ONE small
# operand (a dZ of 1e-3 on the chain's scale, a lattice feature of 1e-5: fp16 keeps 2^-25 absolute of it) decides its relative
# error; the split-fp16 bars of their parameter gradients come from the host model as well
TINY_BATCH = 65
# (K0, N): launch geometry of the split kernels, min(ceil(ceil(N / 16) / 4), 256) workgroups of 4 waves walking 16-sample tiles.
# 1: a single sample; 17: one tile + 1; 63 / 64 / 65: one workgroup's four tiles -1 / exact (the 16-byte LDS-DMA requests) / +1;
# 16 423 = 256 x 4 x 16 + 39: every wave one tile, two waves a second one, the last tile partial; 16 448: the same point with
# N % 16 == 0; 32 807: every wave two tiles.  K0 = 5: no 16-byte request at all; 27: a partial last k-step; 52: the four-input-
# tile instantiation; 64: no zero-padded staging row (the split-bf16 image ends at 52)
GEOMETRY_CASES = [(36, N) for N in (1, 17, 63, 64, 65, 16_423, 16_448, 32_807)] + \
                 [(K0, N) for N in (65, 16_423) for K0 in (5, 27, 52, 64)]


def numerics_case(K0, lattice, dy):
    """-> (lin, x [N, K0], gy [N, 1]) of a numerics case: closed_levels = 6 at lattice 1e-5 (initialisation), 0 at 1e-2"""
    seed = K0 * 100 + (7 if lattice == 1e-2 else 0) + ("ordinary", "six_decades", "outlier").index(dy)
    gen = torch.Generator().manual_seed(seed)
    lin = sdf_net(K0, seed)
    x = sdf_inputs(K0, N_NUMERICS, lattice, 6 if lattice == 1e-5 else 0, gen)
    return lin, x, sdf_dy(N_NUMERICS, dy, gen)


def geometry_case(K0, N):
    """-> (lin, x [N, K0], gy [N, 1]) of a geometry case: lattice 1e-2 and ordinary dY without zeros; the widths without an
    encoding (5, 27, 64) and 52 get plain_inputs"""
    seed = K0 * 100_000 + N
    gen = torch.Generator().manual_seed(seed)
    lin = sdf_net(K0, seed)
    x = sdf_inputs(K0, N, 1e-2, 0, gen) if K0 == 36 else plain_inputs(K0, N, gen)
    return lin, x, sdf_dy(N, "ordinary", gen, misses=False)


# ---------------------------------------------------------------------------------------------------------------------------
# the DOUBLE backward (mlp_dbl_bwd_kernel of csrc/mlp_bwd.hip: psdf_mlp_double_backward, psdf_mlp_double_backward_plus), shared by
# tests/test_mlp_double_backward_float64.py (host) and tests/test_gpu_mlp_double_backward_float64.py

DBL_TENSORS = ("dX2", "dW1", "db1", "dW2", "db2", "dW3", "db3", "dW4", "db4")
# what a mutation of the evaluator changes (tests/test_mlp_double_backward_float64.py measures each against the unmutated one)
DBL_MUTATIONS = [("drop_c", 1), ("drop_c", 2), ("drop_c", 3), ("a_for_c", 1), ("a_for_c", 2), ("a_for_c", 3), ("drop_u1V", 0),
                 ("drop_dY2H3", 0), ("drop_last_sample", 0), ("dY2_without_a3", 0)]


def _gelu_terms64(z):
    """float64 z -> (gelu, a = gelu', c = gelu'' = phi(z) (2 - z^2))"""
    cdf = 0.5 * (1 + torch.erf(z / 2 ** 0.5))
    pdf = torch.exp(-0.5 * z * z) / (2 * torch.pi) ** 0.5
    return z * cdf, cdf + z * pdf, pdf * (2 - z * z)


def f64_double_backward(lin, x, dy, v, dy2=None, mutate=None):
    """float64, by hand and without autograd, in the notation of the kernel's comment (four layers, three hidden):
        H_0 = X;  Z_l = H_{l-1} W_l^T + b_l;  H_l = gelu(Z_l), a_l = gelu'(Z_l), c_l = gelu''(Z_l)  (l = 1..3);  Y = Z_4
        u_4 = dY;  q_l = u_{l+1} W_{l+1};  u_l = a_l * q_l  (l = 3..1)                                  [dX = u_1 W_1]
        objective <dX, V> + <Y, dY2>
        du_1 = V W_1^T;  da_l = du_l * q_l;  dq_l = du_l * a_l;  du_{l+1} = dq_l W_{l+1}^T
        dz_3 = da_3 * c_3 + (dY2 W_4) * a_3;  dz_l = (dz_{l+1} W_{l+1}) * a_l + da_l * c_l;  dX2 = dz_1 W_1
        dW_1 = u_1^T V + dz_1^T X;  dW_{l+1} = u_{l+1}^T dq_l + dz_{l+1}^T H_l (l = 1, 2);  dW_4 = dY^T dq_3 + dY2^T H_3
        db_l = sum_n dz_l (l = 1..3);  db_4 = sum_n dY2
    dy None: the unit gradient of output 0; dy2 None: absent.  -> (gradients {name: tensor}, absolute sums S {name: tensor}, Z
    [Z_1 .. Z_4]).  S is the absolute sum of the LAST dot product of an entry only, its operands at their float64 values.
    mutate (kind, layer): one deliberate defect, see DBL_MUTATIONS."""
    kind, ml = mutate if mutate else (None, 0)
    W = [None] + [l.weight.detach().double() for l in lin]          # 1-based, as in the comment
    b = [None] + [l.bias.detach().double() for l in lin]
    assert len(W) == 5
    X, V = x.double(), v.double()
    N = X.shape[0]
    if dy is None:
        dY = torch.zeros(N, W[4].shape[0], dtype=torch.float64, device=X.device)
        dY[:, 0] = 1.0
    else:
        dY = dy.double()
    dY2 = torch.zeros_like(dY) if dy2 is None else dy2.double()
    H, Z, a, c = [X], [None], [None], [None]
    for l in (1, 2, 3):
        Z.append(H[l - 1] @ W[l].t() + b[l])
        h, al, cl = _gelu_terms64(Z[l])
        H.append(h)
        a.append(al)
        c.append(al if (kind == "a_for_c" and ml == l) else torch.zeros_like(cl) if (kind == "drop_c" and ml == l) else cl)
    Z.append(H[3] @ W[4].t() + b[4])
    u, q = [None] * 5, [None] * 4
    u[4] = dY
    for l in (3, 2, 1):
        q[l] = u[l + 1] @ W[l + 1]
        u[l] = a[l] * q[l]
    du, da, dq = [None] * 5, [None] * 4, [None] * 4
    du[1] = V @ W[1].t()
    for l in (1, 2, 3):
        da[l] = du[l] * q[l]
        dq[l] = du[l] * a[l]
        if l < 3:
            du[l + 1] = dq[l] @ W[l + 1].t()
    dz = [None] * 4
    dh3 = dY2 @ W[4]
    dz[3] = da[3] * c[3] + (dh3 if kind == "dY2_without_a3" else dh3 * a[3])
    for l in (2, 1):
        dz[l] = (dz[l + 1] @ W[l + 1]) * a[l] + da[l] * c[l]
    # the sums over the samples: m drops the last sample of the (partial) last 16-sample tile from them (its dX2 row stays)
    m = torch.ones(N, 1, dtype=torch.float64, device=X.device)
    if kind == "drop_last_sample":
        m[N - 1] = 0.0
    T = lambda t: (t * m).t()
    A = torch.abs
    g, S = {}, {}
    g["dX2"], S["dX2"] = dz[1] @ W[1], A(dz[1]) @ A(W[1])
    uV = torch.zeros_like(W[1]) if kind == "drop_u1V" else T(u[1]) @ V
    g["dW1"], S["dW1"] = uV + T(dz[1]) @ X, A(u[1]).t() @ A(V) + A(dz[1]).t() @ A(X)
    for l in (1, 2):
        g["dW%d" % (l + 1)] = T(u[l + 1]) @ dq[l] + T(dz[l + 1]) @ H[l]
        S["dW%d" % (l + 1)] = A(u[l + 1]).t() @ A(dq[l]) + A(dz[l + 1]).t() @ A(H[l])
    y2h3 = torch.zeros_like(W[4]) if kind == "drop_dY2H3" else T(dY2) @ H[3]
    g["dW4"], S["dW4"] = T(dY) @ dq[3] + y2h3, A(dY).t() @ A(dq[3]) + A(dY2).t() @ A(H[3])
    for l in (1, 2, 3):
        g["db%d" % l], S["db%d" % l] = (dz[l] * m).sum(0), A(dz[l]).sum(0)
    g["db4"], S["db4"] = (dY2 * m).sum(0), A(dY2).sum(0)
    return g, S, Z[1:]


def double_backward_autograd(lin, x, dy, v, dy2=None, dtype=torch.float64):
    """the same gradients by unmodified torch autograd of <d y / d x . dY, V> + <Y, dY2> with create_graph=True, in `dtype`
    (float64: what pins the evaluator; float32: the figure t of the GPU bars) -> {name: tensor}"""
    Ws = [l.weight.detach().to(dtype).requires_grad_(True) for l in lin]
    bs = [l.bias.detach().to(dtype).requires_grad_(True) for l in lin]
    X = x.detach().to(dtype).requires_grad_(True)
    h = X
    for i in range(4):
        h = torch.nn.functional.linear(h, Ws[i], bs[i])
        if i < 3:
            h = torch.nn.functional.gelu(h)
    if dy is None:
        dY = torch.zeros_like(h)
        dY[:, 0] = 1.0
    else:
        dY = dy.to(dtype)
    (gx,) = torch.autograd.grad(h, X, dY, create_graph=True)
    obj = (gx * v.to(dtype)).sum()
    if dy2 is not None:
        obj = obj + (h * dy2.to(dtype)).sum()
    outs = torch.autograd.grad(obj, [X] + Ws + bs, allow_unused=True)
    outs = [o if o is not None else torch.zeros_like(t) for o, t in zip(outs, [X] + Ws + bs)]
    g = {"dX2": outs[0]}
    for l in range(4):
        g["dW%d" % (l + 1)], g["db%d" % (l + 1)] = outs[1 + l], outs[5 + l]
    return g


def sdf_layout(K0):
    """the widths an encoding of this project produces for the SDF nets (8, 16 and 24 levels); the others get plain_inputs"""
    return K0 in (20, 36, 52)


def dbl_v(K0, N, kind, closed_levels, gen, misses=False, layout=True):
    """[N, K0] fp32, the upstream gradient of dX as the encoding's double backward hands it over.  "ordinary": randn; "decades":
    randn * 10^(-6 u) per sample.  With the encoding's layout the columns of the closed levels and the zero pad column are
    exactly 0; misses: 1 row in 16 is exactly 0 (the rows of sdf_dy and dbl_dy2)."""
    assert kind in ("ordinary", "decades"), kind
    v = torch.randn(N, K0, generator=gen)
    if kind == "decades":
        v = v * 10.0 ** (-6.0 * torch.rand(N, 1, generator=gen))
    if layout:
        L = sdf_levels(K0)
        if closed_levels:
            v[:, 2 * (L - closed_levels):2 * L] = 0.0
        v[:, K0 - 1] = 0.0
    if misses:
        v[5::16] = 0.0
    return v


def dbl_dy2(N, out, gen, misses=False):
    """[N, out] fp32, the upstream gradient of the outputs that the plus form folds in: randn * 0.3, the missed rows exactly 0"""
    g = torch.randn(N, out, generator=gen) * 0.3
    if misses:
        g[5::16] = 0.0
    return g


class DblCase:
    """one case of the double backward.  dims [K0, d1, d2, d3, out]; lattice 1e-5 closes six levels, 1e-2 none (only where
    sdf_layout(K0)); v "ordinary" / "decades"; misses; dy "unit" (None is passed: the production form) / "randn"; plus: with dY2;
    tails: W_1 and b_1 times TAILS_SCALE"""

    def __init__(self, dims, N, lattice=1e-2, v="ordinary", misses=False, dy="unit", plus=False, tails=False):
        self.dims, self.N, self.lattice, self.v, self.misses, self.dy, self.plus, self.tails = \
            list(dims), N, lattice, v, misses, dy, plus, tails

    def key(self):
        return (tuple(self.dims), self.N, self.lattice, self.v, self.misses, self.dy, self.plus, self.tails)

    def __repr__(self):
        return "%s%s N=%d lattice=%g V=%s%s dY=%s%s" % ("-".join(map(str, self.dims)), " plus" if self.plus else "", self.N,
                                                       self.lattice, self.v, "+misses" if self.misses else "", self.dy,
                                                       " tails" if self.tails else "")

    def at(self, N):
        """the same family at another batch"""
        return DblCase(self.dims, N, self.lattice, self.v, self.misses, self.dy, self.plus, self.tails)

    def closed(self):
        return 6 if (self.lattice == 1e-5 and sdf_layout(self.dims[0])) else 0

    def make(self):
        """-> (lin, x [N, K0], dy [N, out] or None, v [N, K0], dy2 [N, out] or None), seeded by the case itself"""
        import zlib
        seed = zlib.crc32(repr(self.key()).encode())
        gen = torch.Generator().manual_seed(seed)
        K0, out, N = self.dims[0], self.dims[4], self.N
        lin = sdf_net(K0, seed, out=out, hidden=self.dims[1:4])
        if self.tails:
            with torch.no_grad():
                lin[0].weight.mul_(TAILS_SCALE)
                lin[0].bias.mul_(TAILS_SCALE)
        layout = sdf_layout(K0)
        x = sdf_inputs(K0, N, self.lattice, self.closed(), gen) if layout else plain_inputs(K0, N, gen)
        v = dbl_v(K0, N, self.v, self.closed(), gen, self.misses, layout)
        dy = None if self.dy == "unit" else torch.randn(N, out, generator=gen)
        dy2 = dbl_dy2(N, out, gen, self.misses) if self.plus else None
        return lin, x, dy, v, dy2


# "tails": pre-activations far out in the GELU tails, where 1 + erf cancels, __expf is at its worst and 2 - z^2 is large and
# negative.  The inputs of the encoding's layout are bounded (|point| <= 0.7, lattice features of 1e-2), so a factor of 4 on W_1
# and b_1 reaches max |z_1| = 1.6 .. 1.9 only (measured on these seeds, 0.04 .. 0.4 % of z_1 near +-sqrt 2); 20 reaches
# 8.0 .. 9.3 with 2.8 .. 3.2 % near +-sqrt 2, which is what the host test asserts of the drawn cases (>= 6, >= 1 %)
TAILS_SCALE = 20.0
DBL_BASE, DBL_REF = [36, 64, 64, 64, 1], [52, 32, 32, 32, 33]      # the two production nets; DBL_REF runs in the plus form
N_DBL = 16_423                       # 256 x 4 x 16 + 39: two waves take a second tile, the last tile is partial
# every DBL row of PSDF_MLP16_ROWS (csrc/mlp_dispatch.h) that the library launches, the PLUS rows with and without dY2; ragged
# widths; the final-dot rows with 3 and 4 outputs and a randn dY; one PLUS row with a randn dY
DBL_ROW_CASES = [DblCase(d, N_DBL) for d in ([36, 64, 64, 64, 1], [52, 32, 32, 32, 1], [36, 32, 32, 32, 1],
                                             [20, 32, 32, 32, 1], [52, 32, 32, 32, 33], [36, 32, 32, 32, 33])] + \
                [DblCase(d, N_DBL, plus=True) for d in ([52, 32, 32, 32, 33], [36, 32, 32, 32, 33], [51, 30, 32, 28, 40])] + \
                [DblCase(d, N_DBL, dy="randn") for d in ([35, 64, 64, 64, 3], [44, 64, 64, 64, 4])] + \
                [DblCase([52, 32, 32, 32, 33], N_DBL, dy="randn", plus=True)]
# no fused double backward: row (2, 4, 4, 4, 1) has DBL = 0; row (4, 4, 4, 4, 1) has DBL = 1, but its launch (weight images of
# 49..64 inputs, 100 096 bytes, plus transpose buffer and four staging tiles of each of four waves, 70 144 bytes) is past the
# 163 840 bytes of LDS a launch may use, so
# psdf_mlp_supported declines it (LDS_DECLINED of tests/test_dispatch_tables.py): built, never launched
DBL_UNSUPPORTED = [[20, 64, 64, 64, 1], [52, 64, 64, 64, 1]]
DBL_NUMERICS_CASES = [DblCase(d, N_DBL, lattice, v, misses, plus=d is DBL_REF, tails=tails)
                      for d in (DBL_BASE, DBL_REF)
                      for lattice, tails in ((1e-5, False), (1e-2, False), (1e-2, True))
                      for v, misses in (("ordinary", False), ("decades", True))]
# 1: a single sample; 17: one tile + 1; 63 / 64 / 65: one workgroup's four tiles -1 / exact / +1; 16 423: see N_DBL; 32 807: three
# waves take a third tile, so the two-slot prefetch returns to its first slot
DBL_GEOMETRY_CASES = [DblCase(d, N, plus=d is DBL_REF) for d in (DBL_BASE, DBL_REF) for N in (1, 17, 63, 64, 65, N_DBL, 32_807)]


# ---------------------------------------------------------------------------------------------------------------------------
# the SINGLE-WAVE fp32-MFMA kernels (mlp_bwd_kernel of csrc/mlp_bwd.hip through psdf_mlp_backward and
# psdf_mlp_backward_data_masked, mlp_fwd_kernel of csrc/mlp.hip through psdf_mlp_forward): every row of PSDF_MLP16_ROWS
# (csrc/mlp_dispatch.h) in every launch form it has, shared by tests/test_mlp_single_wave_cases.py (host) and
# tests/test_gpu_mlp_single_wave_float64.py

# launch forms of mlp_bwd_kernel: "dwdx" psdf_mlp_backward(dX, dW); "dw" (NULL, dW); "dx" (dX, NULL): no accumulators, up to 512
# workgroups; "masked" psdf_mlp_backward_data_masked: the "dx" launch with a sample mask
SW_FORMS = ("dwdx", "dw", "dx", "masked")
_ALL, _NO_MASK, _DX = SW_FORMS, ("dwdx", "dw", "dx"), ("dx",)
# (dims, forms): one or more nets per row of PSDF_MLP16_ROWS, in every form the row has.  (The one-output nets of the 64-wide rows
# have their dW+dX form in tests/test_gpu_mlp_baseline_numerics.py as well; here it is what their other forms are compared with.)
# The colour head's dW+dX form reaches this kernel only with PSDF_MLP_WIDE_SPLIT=f32
SW_NETS = [
    ((36, 64, 64, 64, 1), _ALL), ((35, 64, 64, 64, 3), _ALL), ((44, 64, 64, 64, 4), _ALL),                  # (3, 4, 4, 4, 1)
    ((52, 64, 64, 64, 1), _ALL), ((61, 64, 64, 64, 2), _ALL),                                               # (4, 4, 4, 4, 1)
    ((20, 64, 64, 64, 1), _ALL), ((27, 64, 64, 64, 1), _ALL),                                               # (2, 4, 4, 4, 1)
    ((52, 32, 32, 32, 1), _ALL), ((36, 32, 32, 32, 1), _ALL), ((20, 32, 32, 32, 1), _ALL),                  # (4|3|2, 2, 2, 2, 1)
    ((51, 30, 32, 28, 2), _ALL),
    ((52, 32, 32, 32, 33), _NO_MASK), ((36, 32, 32, 32, 33), _NO_MASK), ((51, 30, 32, 28, 40), _NO_MASK),   # (4|3, 2, 2, 2, 3)
    ((52, 64, 64, 64, 65), _DX), ((52, 64, 64, 64, 33), _DX), ((36, 64, 64, 64, 33), _DX),    # (4, 4, 4, 4, 5|3), (3, 4, 4, 4, 3)
    ((50, 60, 64, 56, 70), _DX),
    ((80, 64, 64, 3), _NO_MASK),                                                                            # (5, 4, 4, 0, 1)
]
SW_REF, SW_BASE, SW_HEAD = (52, 32, 32, 32, 33), (36, 64, 64, 64, 1), (80, 64, 64, 3)
# batches, the smallest at which each launch rule of launch_bwd_nw / launch_bwd changes (sw_launch below restates them;
# tests/test_mlp_single_wave_cases.py asserts every claim made here).  The dW forms run min(ceil(tiles / W), 256) workgroups of
# W = 4 waves (8 for 32-wide nets from 2^17 samples on), the data-gradient forms min(ceil(tiles / 4), 512) of 4 waves; wave w of
# workgroup b walks the 16-sample tiles 4 b + w, + 4 x workgroups, ..
#   1: one sample; 17: one tile + 1; 63 / 64 / 65: one workgroup's four tiles - 1 / exact / + 1 (65: a second workgroup with one
#   wave at work on a tile of one sample)
#   16 423 = 256 x 4 x 16 + 39: dW forms: every wave one tile, three waves a second one (two whole tiles and the partial last
#   tile of 7 samples); data-gradient forms: 1027 tiles on 257 workgroups, no wave a second tile
#   32 807 = 512 x 4 x 16 + 39: the same point for the data-gradient forms; dW forms: every wave two tiles, three a third
SW_N_FULL = (1, 17, 63, 64, 65, 16_423, 32_807)
SW_N_DW, SW_N_DX = 16_423, 32_807
# the eight-wave threshold of launch_bwd (32-wide nets, dW forms): 2^17 - 1: four waves, eight tiles each; 2^17 + 19: eight waves,
# four tiles each and two a fifth.  (Baseline-shaped nets, 64 x 3 -> 1, leave this kernel at 2^18 with parameter gradients.)
SW_N_EIGHT = ((1 << 17) - 1, (1 << 17) + 19)
SW_EIGHT_NETS = (SW_REF, (36, 32, 32, 32, 1))
# the fp32 forward (mlp_fwd_kernel): min(ceil(tiles / 4), 1024) workgroups of 4 waves on 32-sample tiles.  131 111 = 1024 x 4 x
# 32 + 39: past the cap, two waves take a second tile, the last tile has 7 samples
SW_N_FWD = (65, 131_111)
# row (4, 4, 2, 1) of PSDF_MLP32_ROWS below the colour net's own widths 111-128-128-64-3, every width short of its last tile
# (a first hidden layer of 96 would be three 32-wide tiles: no row, no forward kernel)
SW_COLOUR_TILES = (100, 112, 128, 48, 2)
SW_FWD_NETS = [d for d, _ in SW_NETS] + [SW_COLOUR_TILES]
# rows of PSDF_MLP32_ROWS (32-wide tiles t1, t2, t3, to, outputs <= 4) with the SPLIT column: psdf_mlp_forward runs the split-bf16
# kernel (path 2) where the net's split image fits 80 KB, the fp32-MFMA kernel (path 1) on the other rows
SW_FWD_SPLIT_ROWS = {(2, 2, 2, 1, True), (1, 1, 1, 1, True), (1, 1, 1, 2, False), (2, 2, 0, 1, True)}
SW_FWD_F32_ROWS = {(2, 2, 2, 3, False), (2, 2, 2, 2, False), (4, 4, 2, 1, True)}


class SwCase:
    """one case of the single-wave kernels: dims (3 or 4 layers), N, the launch forms it runs in, tails (W_1, b_1 times
    TAILS_SCALE)"""

    def __init__(self, dims, N, forms, tails=False):
        self.dims, self.N, self.forms, self.tails = tuple(dims), N, tuple(forms), tails

    def key(self):
        return (self.dims, self.N, self.tails)

    def __repr__(self):
        return "%s N=%d%s" % ("-".join(map(str, self.dims)), self.N, " tails" if self.tails else "")


def _sw_cases():
    cases = []
    for dims, forms in SW_NETS:
        dx_row = forms == _DX
        Ns = SW_N_FULL if dims in (SW_REF, SW_BASE) else (65, SW_N_DX if dx_row else SW_N_DW)
        cases += [SwCase(dims, N, forms) for N in Ns]
    # the masked walk of a SECOND tile: at 16 423 samples the data-gradient launch gives every wave one tile only, so one
    # net per masked row (36-64-64-64-1 has it in its full list) also runs masked at 32 807
    cases += [SwCase(d, SW_N_DX, ("masked",)) for d in ((52, 64, 64, 64, 1), (20, 64, 64, 64, 1), (52, 32, 32, 32, 1),
                                                        (36, 32, 32, 32, 1), (20, 32, 32, 32, 1))]
    cases += [SwCase(d, N, ("dwdx", "dw")) for d in SW_EIGHT_NETS for N in SW_N_EIGHT]
    return cases


SW_CASES = _sw_cases()
SW_TAILS_CASE = SwCase(SW_REF, SW_N_DW, _NO_MASK, tails=True)


def mlp_net(dims, seed):
    """the torch.nn.Linear of any depth with biases ~ N(0, 0.1) (sdf_net for other depths)"""
    torch.manual_seed(seed)
    lin = [torch.nn.Linear(dims[i], dims[i + 1]) for i in range(len(dims) - 1)]
    for l in lin:
        torch.nn.init.normal_(l.bias, 0.0, 0.1)
    return lin


def head_inputs(N, gen):
    """[N, 80] fp32, what the background colour head reads: 64 feature columns ~ randn, 16 columns in [-1, 1]"""
    return torch.cat([torch.randn(N, 64, generator=gen), torch.rand(N, 16, generator=gen) * 2 - 1], 1)


def sw_case(dims, N, tails=False):
    """-> (lin, x [N, K0], gy [N, out]) seeded by the case itself.  x: the encoding's layout at lattice 1e-2 where
    sdf_layout(K0), the head's inputs for 80 columns, plain_inputs otherwise; gy: randn with one row in 16 exactly 0 (rows
    5, 21, ..: the dX rows of these samples have S == 0)"""
    import zlib
    dims = tuple(dims)
    seed = zlib.crc32(repr((dims, N, tails)).encode())
    gen = torch.Generator().manual_seed(seed)
    lin = mlp_net(dims, seed)
    if tails:
        with torch.no_grad():
            lin[0].weight.mul_(TAILS_SCALE)
            lin[0].bias.mul_(TAILS_SCALE)
    K0 = dims[0]
    x = sdf_inputs(K0, N, 1e-2, 0, gen) if sdf_layout(K0) else head_inputs(N, gen) if K0 == 80 else plain_inputs(K0, N, gen)
    gy = torch.randn(N, dims[-1], generator=gen)
    gy[5::16] = 0.0
    return lin, x, gy


def sw_sig16(dims):
    """tile signature of PSDF_MLP16_ROWS (_sig16 of tests/test_dispatch_tables.py)"""
    t = [(w + 15) // 16 for w in dims]
    return (t[0], t[1], t[2], t[3] if len(dims) == 5 else 0, t[-1], dims[-1] <= 4)


def sw_sig32(dims):
    t = [(w + 31) // 32 for w in dims]
    return (t[1], t[2], t[3] if len(dims) == 5 else 0, t[-1], dims[-1] <= 4)


def _walk(ntiles, workgroups, waves):
    """wave w of workgroup b walks the tiles waves b + w, + waves x workgroups, ..: the launch in numbers"""
    stride = workgroups * waves
    return {"waves": waves, "workgroups": workgroups, "tiles": ntiles, "stride": stride,
            "least": ntiles // stride,                              # tiles every wave of the launch walks
            "most": -(-ntiles // stride),                           # tiles of the busiest wave
            "extra": ntiles % stride}                               # waves that walk `most` tiles where most > least


def sw_launch(dims, N, form):
    """launch_bwd and launch_bwd_nw of csrc/mlp_bwd.hip restated: workgroups, waves per workgroup, tiles per wave, and whether
    the last 16-sample tile is partial (`last`: its samples)"""
    assert form in SW_FORMS
    ntiles = -(-N // 16)
    with_dw = form in ("dwdx", "dw")
    narrow = all(w <= 32 for w in dims[1:-1])
    waves = 8 if (with_dw and narrow and N >= 1 << 17) else 4      # the data-gradient kernel is built for four waves only
    r = _walk(ntiles, min(-(-ntiles // waves), 256 if with_dw else 512), waves)
    r["last"] = N - 16 * (ntiles - 1)
    return r


def fwd_launch(N):
    """launch_fwd of csrc/mlp.hip (the fp32 forward) restated, 32-sample tiles"""
    ntiles = -(-N // 32)
    r = _walk(ntiles, min(-(-ntiles // 4), 1024), 4)
    r["last"] = N - 32 * (ntiles - 1)
    return r


def fwd_split_image_bytes(dims):
    """bytes of the split-bf16 image of psdf_mlp_pack (make_split_plan of csrc/mlp_device.h): 16-byte records"""
    nl = len(dims) - 1
    t = [(w + 31) // 32 for w in dims]
    dot = dims[-1] <= 4
    rec = f = 0
    for l in range(nl):
        last_dot = l == nl - 1 and dot
        if not last_dot:
            rec += t[l + 1] * ((dims[0] + 15) // 16 if l == 0 else 2 * t[l]) * 3 * 64
        f += (dims[-1] * t[l] * 32 + 4) if last_dot else t[l + 1] * 32
    return (rec + (f + 3) // 4) * 16


def fwd_path(dims):
    """what psdf_last_path(2) must say after psdf_mlp_forward of this net, by the table"""
    sig = sw_sig32(dims)
    if sig in SW_FWD_SPLIT_ROWS and fwd_split_image_bytes(dims) <= 80 * 1024:
        return 2
    assert sig in SW_FWD_SPLIT_ROWS | SW_FWD_F32_ROWS, dims
    return 1


# skip patterns of the masked form (16-sample tiles; a tile is skipped when ALL its samples are masked)
SW_MASKS = ("none", "all", "interior_tile", "fifteen_of_sixteen", "last_tile", "every_second_tile")
# where a wave walks two tiles (N = 32 807): its first tile masked and its second live, and the reverse
SW_MASKS_TWO_TILES = ("every_second_tile", "first_round", "second_round")


def sw_mask(N, pattern, stride=2048):
    """-> (skip [N] uint8, skipped [N] bool: the samples of fully masked tiles, whose dX columns must keep their contents).
    interior_tile: tile tiles // 2; fifteen_of_sixteen: tile 1 but for its sample 7 (a live tile: all 16 are evaluated);
    last_tile: the partial last tile; every_second_tile: the odd tiles; first_round / second_round: the tiles below / from
    `stride` on (the data-gradient launch's waves x workgroups)"""
    ntiles = -(-N // 16)
    tile = torch.arange(N) // 16
    if pattern == "none":
        skip = torch.zeros(N, dtype=torch.bool)
    elif pattern == "all":
        skip = torch.ones(N, dtype=torch.bool)
    elif pattern == "interior_tile":
        assert 0 < ntiles // 2 < ntiles - 1
        skip = tile == ntiles // 2
    elif pattern == "fifteen_of_sixteen":
        assert ntiles > 2
        skip = tile == 1
        skip[16 + 7] = False
    elif pattern == "last_tile":
        skip = tile == ntiles - 1
    elif pattern == "every_second_tile":
        skip = tile % 2 == 1
    elif pattern == "first_round":
        skip = tile < stride
    else:
        assert pattern == "second_round", pattern
        skip = tile >= stride
    live_tiles = torch.zeros(ntiles, dtype=torch.bool)
    live_tiles[tile[~skip]] = True
    return skip.to(torch.uint8), ~live_tiles[tile]
