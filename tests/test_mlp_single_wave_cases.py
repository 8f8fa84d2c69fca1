"""Host: the case lists of the single-wave MLP kernels (tests/mlp_float64.py: SW_CASES and what goes with them), which
tests/test_gpu_mlp_single_wave_float64.py runs on the device.  No kernel runs here.

  coverage    the tile signatures of the cases, per launch form, are exactly the sets BWD_DW, BWD_DX and BWD_MASKED of
              tests/test_dispatch_tables.py: a row added to PSDF_MLP16_ROWS fails here until it has a case
  launches    for every batch size of the lists the launch arithmetic of launch_bwd / launch_bwd_nw (csrc/mlp_bwd.hip) and of
              launch_fwd (csrc/mlp.hip), restated in sw_launch / fwd_launch, does what the comments of the lists claim
  the pin     _f64_trace equals unmodified torch float64 autograd to 1e-12 S per entry on a three-layer net, a 33-output net and a
              ragged net (the other host tests pin it for four layers ending in one output)
  tails       the tails case reaches max |z_1| >= 6 with at least 1 % of z_1 within 0.05 of +-sqrt 2
  masks       every skip pattern has the live and skipped tiles it is named after"""
import pytest
import torch

from tests import mlp_float64 as M
from tests.mlp_float64 import _f64_trace, _per_entry
from tests.test_dispatch_tables import BWD_DW, BWD_DX, BWD_MASKED, FWD

PIN = 1e-12


def _all_cases():
    return M.SW_CASES + [M.SW_TAILS_CASE]


def test_cases_cover_every_row_in_every_form():
    sigs = {f: set() for f in M.SW_FORMS}
    for c in _all_cases():
        for f in c.forms:
            sigs[f].add(M.sw_sig16(c.dims))
    assert sigs["dw"] == BWD_DW
    assert sigs["dx"] == BWD_DX
    assert sigs["masked"] == BWD_MASKED
    assert sigs["dwdx"] == BWD_DW
    for dims, forms in M.SW_NETS:
        sig = M.sw_sig16(dims)
        assert sig in BWD_DX, dims
        assert ("dw" in forms) == ("dwdx" in forms) == (sig in BWD_DW), dims
        assert ("masked" in forms) == (sig in BWD_MASKED) and "dx" in forms, dims
    assert len({c.key() + (c.forms,) for c in _all_cases()}) == len(_all_cases())


def test_every_net_has_its_batches():
    by_net = {}
    for c in M.SW_CASES:
        by_net.setdefault(c.dims, set()).add(c.N)
    for dims, forms in M.SW_NETS:
        Ns = by_net[dims]
        if dims in (M.SW_REF, M.SW_BASE):
            assert set(M.SW_N_FULL) <= Ns, dims
        elif forms == ("dx",):
            assert Ns == {65, M.SW_N_DX}, dims
        else:
            assert {65, M.SW_N_DW} <= Ns, dims
    for dims in M.SW_EIGHT_NETS:
        assert set(M.SW_N_EIGHT) <= by_net[dims]
    # parameter gradients of a baseline-shaped net leave this kernel at 2^18 samples
    for c in _all_cases():
        if "dw" in c.forms or "dwdx" in c.forms:
            assert c.N < 1 << 18, c


def test_forward_nets_are_on_the_paths_the_table_gives():
    for dims in M.SW_FWD_NETS:
        assert M.sw_sig32(dims) in FWD, dims
    assert M.SW_FWD_SPLIT_ROWS | M.SW_FWD_F32_ROWS == FWD and not M.SW_FWD_SPLIT_ROWS & M.SW_FWD_F32_ROWS
    one = [d for d in M.SW_FWD_NETS if M.fwd_path(d) == 1]
    assert one == [(52, 64, 64, 64, 65), (52, 64, 64, 64, 33), (36, 64, 64, 64, 33), (50, 60, 64, 56, 70), M.SW_COLOUR_TILES], one
    # the three rows without a split image each have a net; 96 in place of 112 would leave the colour net's row
    assert M.sw_sig32((100, 96, 128, 48, 2)) not in FWD
    assert {M.sw_sig32(d) for d in one} == M.SW_FWD_F32_ROWS
    # the image of the BASELINE net as csrc/mlp_device.h states it
    assert M.fwd_split_image_bytes((36, 64, 64, 64, 1)) == 68_624 and M.fwd_split_image_bytes((64, 64, 64, 64, 4)) <= 80 * 1024


def test_the_library_has_a_kernel_for_every_net_and_form():
    """psdf_mlp_supported (host code of the compiled library) for every net in every form it is listed with, and no masked
    form where none is listed"""
    from permuto_sdf_amd import mlp as P
    for dims, forms in M.SW_NETS:
        d = list(dims)
        assert P.supported(P.OP_BACKWARD_DATA, d), dims
        assert P.supported(P.OP_BACKWARD_DATA_MASKED, d) == ("masked" in forms), dims
        assert P.supported(P.OP_BACKWARD, d), dims                      # (the dX-only rows: through the wide kernel)
    for dims in M.SW_FWD_NETS:
        assert P.supported(P.OP_FORWARD, list(dims)), dims
    assert not P.supported(P.OP_FORWARD, [100, 96, 128, 48, 2])


@pytest.mark.parametrize("form", M.SW_FORMS)
def test_small_batches_do_to_the_launch_what_the_list_says(form):
    dims = M.SW_BASE
    L = lambda N: M.sw_launch(dims, N, form)
    assert (L(1)["workgroups"], L(1)["tiles"], L(1)["last"]) == (1, 1, 1)
    assert (L(17)["workgroups"], L(17)["tiles"], L(17)["last"]) == (1, 2, 1)
    assert (L(63)["workgroups"], L(63)["tiles"], L(63)["last"]) == (1, 4, 15)
    assert (L(64)["workgroups"], L(64)["tiles"], L(64)["last"]) == (1, 4, 16)
    assert (L(65)["workgroups"], L(65)["tiles"], L(65)["last"]) == (2, 5, 1)
    for N in (1, 17, 63, 64, 65):
        assert L(N)["most"] == 1 and L(N)["waves"] == 4


def test_second_tile_batches():
    for dims, _ in M.SW_NETS:
        for form in ("dwdx", "dw"):
            a = M.sw_launch(dims, M.SW_N_DW, form)
            # every wave one tile, three waves a second one: two whole tiles and the partial last one
            assert (a["waves"], a["workgroups"], a["tiles"]) == (4, 256, 1027)
            assert (a["least"], a["most"], a["extra"], a["last"]) == (1, 2, 3, 7)
            b = M.sw_launch(dims, M.SW_N_DX, form)
            # every wave two tiles, three a third: the prefetch returns to its first buffer
            assert (b["workgroups"], b["least"], b["most"], b["extra"], b["last"]) == (256, 2, 3, 3, 7)
        for form in ("dx", "masked"):
            a = M.sw_launch(dims, M.SW_N_DW, form)
            assert (a["workgroups"], a["most"]) == (257, 1)            # below the cap: no wave walks a second tile
            b = M.sw_launch(dims, M.SW_N_DX, form)
            assert (b["waves"], b["workgroups"], b["tiles"], b["stride"]) == (4, 512, 2051, 2048)
            assert (b["least"], b["most"], b["extra"], b["last"]) == (1, 2, 3, 7)
    assert M.SW_N_DW == 256 * 4 * 16 + 39 and M.SW_N_DX == 512 * 4 * 16 + 39
    # the masked form meets a second tile: every masked row has a case at 32 807
    rows = {M.sw_sig16(c.dims) for c in M.SW_CASES if "masked" in c.forms and c.N == M.SW_N_DX}
    assert rows == BWD_MASKED


def test_eight_wave_threshold():
    below, above = M.SW_N_EIGHT
    assert below == (1 << 17) - 1 and above == (1 << 17) + 19
    for dims in M.SW_EIGHT_NETS:
        for form in ("dwdx", "dw"):
            a, b = M.sw_launch(dims, below, form), M.sw_launch(dims, above, form)
            assert (a["waves"], a["workgroups"], a["least"], a["most"], a["last"]) == (4, 256, 8, 8, 15)
            assert (b["waves"], b["workgroups"], b["least"], b["most"], b["extra"], b["last"]) == (8, 256, 4, 5, 2, 3)
        # the data-gradient kernel has the four-wave form only
        assert M.sw_launch(dims, above, "dx")["waves"] == 4
    # a 64-wide net stays on four waves
    assert M.sw_launch(M.SW_BASE, above, "dw")["waves"] == 4
    cases = {(c.dims, c.N) for c in M.SW_CASES if "dwdx" in c.forms and "dw" in c.forms}
    assert {(d, N) for d in M.SW_EIGHT_NETS for N in M.SW_N_EIGHT} <= cases
    assert max(c.N for c in _all_cases()) == above


def test_forward_batches():
    a, b = (M.fwd_launch(N) for N in M.SW_N_FWD)
    assert (a["workgroups"], a["tiles"], a["most"], a["last"]) == (1, 3, 1, 1)
    assert M.SW_N_FWD[1] == 1024 * 4 * 32 + 39
    # past the cap of 1024 workgroups: two waves take a second tile, the last one has 7 samples
    assert (b["workgroups"], b["tiles"], b["least"], b["most"], b["extra"], b["last"]) == (1024, 4098, 1, 2, 2, 7)


@pytest.mark.parametrize("N", (65, M.SW_N_DW, M.SW_N_DX))
def test_masks_are_what_their_names_say(N):
    ntiles = -(-N // 16)
    tile = torch.arange(N) // 16
    patterns = M.SW_MASKS + (M.SW_MASKS_TWO_TILES if N == M.SW_N_DX else ())
    stride = M.sw_launch(M.SW_BASE, N, "masked")["stride"]
    for pattern in patterns:
        skip, skipped = M.sw_mask(N, pattern, stride=2048)
        assert skip.dtype == torch.uint8 and skip.shape == (N,) and skipped.shape == (N,)
        skipped_tiles = set(tile[skipped].tolist())
        assert bool((skip.bool() >= skipped).all())
        # a tile is skipped exactly when all its samples are masked
        full = {t for t in range(ntiles) if bool(skip[16 * t:16 * t + 16].all())}
        assert skipped_tiles == full, pattern
        if pattern == "none":
            assert not full and not bool(skip.any())
        elif pattern == "all":
            assert len(full) == ntiles
        elif pattern == "interior_tile":
            assert full == {ntiles // 2} and 0 < ntiles // 2 < ntiles - 1
        elif pattern == "fifteen_of_sixteen":
            assert not full and int(skip.sum()) == 15 and int(skip[16:32].sum()) == 15
        elif pattern == "last_tile":
            assert full == {ntiles - 1} and N % 16 != 0
        elif pattern == "every_second_tile":
            assert full == set(range(1, ntiles, 2))
        elif pattern == "first_round":
            # every wave with two tiles skips the first and computes the second, into its second prefetch buffer
            assert stride == 2048 and full == set(range(stride)) and ntiles > stride
        else:
            assert stride == 2048 and full == set(range(stride, ntiles)) and full


def _autograd64(lin, x, gy):
    Ws = [l.weight.detach().double().requires_grad_(True) for l in lin]
    bs = [l.bias.detach().double().requires_grad_(True) for l in lin]
    X = x.double().requires_grad_(True)
    h = X
    for i in range(len(Ws)):
        h = torch.nn.functional.linear(h, Ws[i], bs[i])
        if i < len(Ws) - 1:
            h = torch.nn.functional.gelu(h)
    outs = torch.autograd.grad(h, [X] + Ws + bs, gy.double())
    g = {"dX": outs[0]}
    for l in range(len(Ws)):
        g["dW%d" % (l + 1)], g["db%d" % (l + 1)] = outs[1 + l], outs[1 + len(Ws) + l]
    return h.detach(), g


@pytest.mark.parametrize("dims", [M.SW_HEAD, M.SW_REF, (51, 30, 32, 28, 40), (50, 60, 64, 56, 70), (44, 64, 64, 64, 4)],
                         ids=lambda d: "-".join(map(str, d)))
def test_evaluator_matches_float64_autograd(dims):
    lin, x, gy = M.sw_case(dims, 65)
    y, SY, g, S, H, dZ = _f64_trace(lin, x, gy)
    y_ref, ref = _autograd64(lin, x, gy)
    assert len(H) == len(dims) - 1 and len(dZ) == len(dims) - 1
    assert set(g) == set(ref) and len(g) == 2 * (len(dims) - 1) + 1
    worst, bad = _per_entry(y, y_ref, SY)
    assert not bad and worst <= PIN, ("Y", worst)
    for k in g:
        assert g[k].shape == ref[k].shape == S[k].shape, k
        e, bad = _per_entry(g[k], ref[k], S[k])
        assert not bad, (k, "autograd is not exactly 0 where S == 0")
        assert bool(((S[k] == 0) <= (g[k] == 0)).all()), (k, "the evaluator is not exactly 0 where S == 0")
        assert e <= PIN, (k, e)
        worst = max(worst, e)
    # the dX rows of the samples without an upstream gradient have no term
    rows = torch.zeros(65, dtype=torch.bool)
    rows[5::16] = True
    assert bool((S["dX"][rows] == 0).all()) and bool((S["dX"][~rows] > 0).any())
    if M.sdf_layout(dims[0]):
        assert bool((S["dW1"][:, dims[0] - 1] == 0).all())              # the encoding's zero pad column
    print("single wave %s: pin %.1e" % ("-".join(map(str, dims)), worst))


def test_tails_case_reaches_the_tails():
    c = M.SW_TAILS_CASE
    assert c.dims == M.SW_REF and c.N == M.SW_N_DW and c.tails
    lin, x, _ = M.sw_case(c.dims, c.N, tails=True)
    plain, _, _ = M.sw_case(c.dims, c.N)
    z1 = x.double() @ lin[0].weight.detach().double().t() + lin[0].bias.detach().double()
    near = float((((z1.abs() - 2 ** 0.5).abs()) <= 0.05).double().mean())
    print("single wave %r: max |z_1| %.2f, share within 0.05 of +-sqrt 2: %.4f" % (c, float(z1.abs().max()), near))
    assert float(z1.abs().max()) >= 6.0 and near >= 0.01, (float(z1.abs().max()), near)


def test_cases_are_seeded_by_themselves():
    a, b = M.sw_case(M.SW_REF, 65), M.sw_case(M.SW_REF, 65)
    assert all(torch.equal(p.weight, q.weight) and torch.equal(p.bias, q.bias) for p, q in zip(a[0], b[0]))
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    c = M.sw_case(M.SW_REF, 64)
    assert not torch.equal(a[1][:64], c[1])
    x, gy = M.sw_case(M.SW_HEAD, 65)[1:]
    assert x.shape == (65, 80) and float(x[:, 64:].abs().max()) <= 1.0 and float(x[:, :64].abs().max()) > 1.0
    assert gy.shape == (65, 3) and bool((gy[5::16] == 0).all()) and bool((gy[4::16] != 0).all())
