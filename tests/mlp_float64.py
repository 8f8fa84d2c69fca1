"""float64 reference of the Linear / GELU nets with every entry's absolute sum, and the inputs of the BASELINE SDF net
{K0 <= 64, 64, 64, 64, 1} as the encoding hands them over -- shared by the per-entry MLP tests (tests/test_gpu_mlp_wide_numerics.py,
tests/test_gpu_mlp_baseline_numerics.py) and by the host restatement of the split-fp16 arithmetic (tests/test_split_f16_numerics.py).

Per-entry metric: |ours - f64| / S with S the entry's own absolute sum in float64 (the error scale of a dot product; it does not
blow up where a sum cancels): dW_l: |dZ_l|^T |H_{l-1}|, db_l: sum |dZ_l|, dX: |dZ_1| |W_1|, Y: |h_{L-1}| |W_L|^T + |b_L|.  An entry
whose S is 0 has no non-zero term at all and must be exactly 0.

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


def sdf_net(K0, seed):
    """the four torch.nn.Linear of K0-64-64-64-1 with biases ~ N(0, 0.1) (as tests/test_gpu_mlp.py makes its split nets)"""
    torch.manual_seed(seed)
    dims = [K0, 64, 64, 64, 1]
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
