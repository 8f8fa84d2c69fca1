"""The workgroup forms of the split forward kernels (csrc/mlp.hip): W waves share one weight image in LDS, W = 4
(mlp_fwd_split_kernel, every net) and the wide form (mlp_fwd_split_wg_kernel, the 64-wide nets).  The form only changes which
wave walks which 32-sample tile, so every built form must give the bytes of the four-wave form; that one is held to the
float64 bars of tests/test_gpu_mlp.py::test_split_f16_forward_against_float64 (4e-6 of the largest output with two fp16
pieces, 3e-6 with three bf16 pieces), and to the bytes the parent of the change that introduced the forms computed
(tests/golden/mlp_forward_parent_bits.npz, written by tools/make_mlp_forward_golden.py with that commit's library): a
rewrite of the evaluator (a shorter GELU tail was tried with the forms) must not move a bit.

Batch sizes: 1, 33 (one tile plus one sample), 255 / 257 and 511 / 513 (an 8-wave and a 16-wave workgroup's worth of tiles
minus and plus one sample: some waves of a workgroup have no tile), CUs x W x 32 + 39 for W = 8 and 16 (one workgroup of W waves
per CU plus two tiles, the last one partial) and 2 x CUs x 16 x 32 + 39 (every wave of a resident round of a wide form -- 16
waves per CU -- walks two tiles, two of them a third; the four-wave form walks four and five).  The smaller batches are prefixes
of the largest one, so one float64 evaluation per net serves all of them."""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FORMS = (4, 8, 16)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mlp_forward_parent_bits.npz")
SENTINEL = 7.0

# (widths, fp16 pieces); K0 = 27: a partial last k-step with rows of the lower half of the wave only
NETS = [([K0, 64, 64, 64, 1], f16) for K0 in (36, 52, 27) for f16 in (True, False)] + [([36, 64, 64, 1], False)]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda")


@pytest.fixture(autouse=True)
def _policy_restored():
    from permuto_sdf_amd.mlp import set_forward_form
    yield
    set_forward_form(0)


def _batch_sizes():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return (1, 33, 255, 257, 511, 513, cus * 8 * 32 + 39, cus * 16 * 32 + 39, 2 * cus * 16 * 32 + 39)


def _forward(dims, x_fm, packed, f16, form, skip=None):
    """-> (status, y): the forward under a forced form; y prefilled so that unwritten entries show"""
    from permuto_sdf_amd import _lib as L
    from permuto_sdf_amd.mlp import _dims_array, set_forward_form
    N = x_fm.shape[1]
    y = torch.full((dims[-1], N), SENTINEL, dtype=torch.float32, device=x_fm.device)
    lib = L.lib()
    set_forward_form(form)
    try:
        args = [L.c_i(len(dims) - 1), _dims_array(dims), L.c_l(N), L.ptr(x_fm), L.ptr(packed)]
        if f16:
            assert skip is None      # (psdf_mlp_forward_f16 has no masked entry point)
            rc = lib.psdf_mlp_forward_f16(*args, L.ptr(y), L.stream())
        elif skip is None:
            rc = lib.psdf_mlp_forward(*args, L.ptr(y), L.stream())
        else:
            rc = lib.psdf_mlp_forward_masked(*args, L.ptr(skip), L.ptr(y), L.stream())
        torch.cuda.synchronize()
    finally:
        set_forward_form(0)
    return int(rc), y


def _net(dims, dev, seed):
    torch.manual_seed(seed)
    nl = len(dims) - 1
    lin = [torch.nn.Linear(dims[i], dims[i + 1]) for i in range(nl)]
    mods = []
    for i, l in enumerate(lin):
        mods.append(l)
        if i < nl - 1:
            mods.append(torch.nn.GELU())
    net = torch.nn.Sequential(*mods).to(dev)
    return net, [l.weight for l in lin], [l.bias for l in lin]


@pytest.mark.parametrize("dims,f16", NETS, ids=lambda v: "-".join(map(str, v)) if isinstance(v, list) else ("f16" if v else "bf16"))
def test_every_form_gives_the_bytes_of_the_four_wave_form(dev, dims, f16):
    import copy
    from permuto_sdf_amd.mlp import last_forward_form, pack_params
    K0 = dims[0]
    sizes = _batch_sizes()
    net, ws, bs = _net(dims, dev, 100 + K0 + len(dims))
    x = torch.randn(max(sizes), K0, device=dev)
    x[:, K0 // 2:] *= 1e-3
    with torch.no_grad():
        y64 = copy.deepcopy(net).double()(x.double())        # [Nmax, 1], once for every batch size
    packed = pack_params(dims, ws, bs, f16=f16)
    # the mask: whole tiles (every third one, and the last) and single samples (every seventh)
    n_all = torch.arange(max(sizes), device=dev)
    mask_all = (((n_all // 32) % 3 == 1) | (n_all % 7 == 3)).to(torch.uint8)
    bar = 4e-6 if f16 else 3e-6
    built = set()
    for N in sizes:
        x_fm = x[:N].t().contiguous()
        masks = [None]
        if not f16:
            m = mask_all[:N].clone()
            m[(N - 1) // 32 * 32:] = 1                        # the (partial) last tile entirely
            masks.append(m.contiguous())
        for skip in masks:
            rc, y4 = _forward(dims, x_fm, packed, f16, 4, skip)
            assert rc == 0 and last_forward_form() == 4, (N, rc)
            ref = y64[:N, 0]
            if skip is None:
                written = torch.ones(N, dtype=torch.bool, device=dev)
            else:       # a tile is evaluated unless every one of its samples is masked
                pad = torch.ones((N + 31) // 32 * 32, dtype=torch.int32, device=dev)
                pad[:N] = skip
                written = (pad.view(-1, 32).min(dim=1).values == 0).repeat_interleave(32)[:N]
                assert bool((y4[0][~written] == SENTINEL).all()), "a fully masked tile was written"
            if bool(written.any()):
                scale = float(ref[written].abs().max())
                err = float((y4[0].double() - ref)[written].abs().max()) / scale
                print("dims %s %s N=%d %s: %.2e of the largest output (bar %.0e)"
                      % (dims, "fp16" if f16 else "bf16", N, "masked" if skip is not None else "plain", err, bar))
                assert err <= bar, (N, err, bar)
            for W in FORMS[1:]:
                before = last_forward_form()
                rc, yw = _forward(dims, x_fm, packed, f16, W, skip)
                if rc == -2:                                   # this form is not built: nothing ran
                    assert bool((yw == SENTINEL).all()) and last_forward_form() == before
                    continue
                assert rc == 0 and last_forward_form() == W, (N, W, rc)
                built.add(W)
                assert torch.equal(yw.view(torch.int32), y4.view(torch.int32)), (N, W, skip is not None)
    assert built, "no wide form is built for a 64-wide net"
    # the policy: a single tile keeps the four-wave form
    rc, y0 = _forward(dims, x[:33].t().contiguous(), packed, f16, 0)
    assert rc == 0 and last_forward_form() == 4


def test_a_form_that_is_not_built_is_declined(dev):
    """the 32-wide nets have the four-wave form only; a value that names no form is an argument error"""
    from permuto_sdf_amd import _lib as L
    from permuto_sdf_amd.mlp import last_forward_form, pack_params
    dims = [36, 32, 32, 32, 1]
    net, ws, bs = _net(dims, dev, 5)
    x_fm = torch.randn(36, 4099, device=dev)
    packed = pack_params(dims, ws, bs)
    rc, y4 = _forward(dims, x_fm, packed, False, 4)
    assert rc == 0 and last_forward_form() == 4 and not bool((y4 == SENTINEL).any())
    for W in (8, 16):
        rc, y = _forward(dims, x_fm, packed, False, W)
        assert rc == -2 and bool((y == SENTINEL).all()) and last_forward_form() == 4, (W, rc)
    f = L.lib().psdf_mlp_forward_set_form
    f.restype = ctypes.c_int
    assert f(3) == -1 and f(32) == -1 and f(-4) == -1 and f(0) == 0
    rc, y = _forward(dims, x_fm, packed, False, 0)
    assert rc == 0 and torch.equal(y, y4)
    assert L.lib().psdf_last_path(2) == 2


@pytest.mark.parametrize("K0", [36, 52])
def test_every_form_gives_the_bytes_of_the_parent(dev, K0):
    from permuto_sdf_amd import _lib as L
    from permuto_sdf_amd.mlp import pack_params
    g = np.load(GOLDEN)
    # provenance: the commit the generating library was built from (the parent of the change that introduced the forms) and
    # the hash of that library, so the file can be regenerated and compared
    assert len(str(g["generated_from_commit"])) == 40 and len(str(g["library_sha256"])) == 64
    dims = [K0, 64, 64, 64, 1]
    x_fm = torch.from_numpy(g["x_%d" % K0]).to(dev).contiguous()
    assert x_fm.shape == (K0, 513)
    ws = [torch.from_numpy(g["w%d_%d" % (i, K0)]).to(dev) for i in range(4)]
    bs = [torch.from_numpy(g["b%d_%d" % (i, K0)]).to(dev) for i in range(4)]
    ran = 0
    for name, f16 in (("f16", True), ("bf16", False)):
        want = torch.from_numpy(g["y_%s_%d" % (name, K0)]).view(torch.int32)
        packed = pack_params(dims, ws, bs, f16=f16)
        for W in (0,) + FORMS:
            rc, y = _forward(dims, x_fm, packed, f16, W)
            if rc == -2 and W in FORMS[1:]:
                continue
            assert rc == 0, (name, W, rc)
            assert L.lib().psdf_last_path(2) == (3 if f16 else 2)
            ran += W > 4
            assert torch.equal(y.cpu().view(torch.int32), want), (name, W)
    assert ran >= 2, "no wide form ran"
