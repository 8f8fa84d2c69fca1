"""Host: the case lists of the fused encode -> MLP forward (tests/fused_float64.py), which tests/test_gpu_fused_float64.py runs on
the device.  No kernel runs here.

  coverage    the tile signatures of the cases are exactly the CASE(...) rows of csrc/fused.hip: a row added there fails here
              until it has a case; every row runs at every batch of FUSED_N, every concat mode at 16 and at 3 levels
  launches    131 111 samples need more tiles than 1024 workgroups x 4 waves, two waves take a second tile and the last tile
              is partial; the smaller batches stay below the cap
  LDS         make_plan restated equals psdf_mlp_packed_size on the nets without a split image; the two LDS cases lie on the two
              sides of 64 KiB by psdf_mlp_packed_size
  no launch   the declined shapes have no row, and an encoding that matches their input width
  masks       every skip pattern has the live and fully masked tiles it is named after
  reference   the float64 MLP equals unmodified torch float64 to 1e-12 S per entry on every row's net, on the float64 encoding of
              the case's own points; torch fp32 on the CPU stays within max(4 t, 5e-6) of it (t is that figure, so by
              construction), no entry has S == 0, and two of the defects the kernel could have -- the features of a level pair
              swapped, the last pseudo-level dropped -- are far beyond the bar"""
import os

import pytest
import torch

from tests import fused_float64 as F
from tests import mlp_float64 as M
from tests.mlp_float64 import _f64_trace, _per_entry

PIN, FLOOR = 1e-12, 5e-6
SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "permuto_sdf_amd", "csrc", "fused.hip")


def test_cases_cover_every_row_of_the_dispatch():
    rows = F.fused_rows_in_source(open(SOURCE).read())
    assert len(rows) == 4 and len(set(rows)) == len(rows), rows
    assert set(rows) == set(F.FUSED_ROWS)
    for row, (hidden, out) in F.FUSED_ROWS.items():
        assert M.sw_sig32((36,) + hidden + (out,)) == row
        assert out % 32 != 0 and (out == 3) == row[4]                   # no multiple of a tile; 3 of the 1..4 of a dot row
    by_row = {}
    for c in F.ROW_CASES:
        assert M.sw_sig32(c.dims) == c.row
        by_row.setdefault(c.row, set()).add(c.N)
    assert by_row == {row: set(F.FUSED_N) for row in F.FUSED_ROWS}
    assert {M.sw_sig32(c.dims) for c in F.CASES} == set(rows)
    assert {M.sw_sig32(c.dims) for c in F.MASK_CASES if c.N == F.N_MID} == set(rows)
    assert {c.N for c in F.MASK_CASES} == {F.N_MID, F.N_CAP}
    assert len({c.key() for c in F.CASES}) == len(F.CASES)
    assert F.N_CAP == M.SW_N_FWD[1]


def test_concat_modes_and_level_counts():
    seen = {(c.levels, c.mode): c for c in F.MODE_CASES}
    assert set(seen) == {(L, m) for L in (16, 3) for m in (F.NONE, F.PADDED, F.APPENDED)}
    assert [seen[(16, m)].dims[0] for m in (F.NONE, F.PADDED, F.APPENDED)] == [32, 36, 35]
    assert [seen[(3, m)].dims[0] for m in (F.NONE, F.PADDED, F.APPENDED)] == [6, 10, 9]
    for c in F.MODE_CASES:
        assert c.feat64 and c.capacity & (c.capacity - 1)             # the runtime modulo
        steps = (c.dims[0] + 1) // 2
        if c.levels == 3:
            assert steps % 2 == 1                                      # the last level pair is half empty
        if c.mode == F.APPENDED:
            assert c.dims[0] % 2 == 1 and steps == c.levels + 2         # in_steps0 rounds up: row 2L+3 must not be written
    assert {c.mode for c in F.MODE_CASES if c.feat64} == {F.NONE, F.PADDED, F.APPENDED}
    assert {c.lattice for c in F.CASES} == {0.5, 1e-5} and {c.window for c in F.CASES} == {"mixed", "c2f"}
    assert {c.points for c in F.CASES} == {"hard", "rays", "vertices"}
    assert [c.conv.get("rank_tie_raises_later") for c in F.CONV_CASES] == [0, 1]
    from permuto_sdf_amd import conventions as CV
    second = [c.conv["hash_multiplier"] for c in F.CONV_CASES if "hash_multiplier" in c.conv]
    assert second and all(m != CV.DEFAULTS["PSDF_ENC_HASH_MULTIPLIER"] for m in second)


def test_batches_do_to_the_launch_what_the_list_says():
    L = F.fused_launch
    assert (L(1)["workgroups"], L(1)["tiles"], L(1)["last"]) == (1, 1, 1)
    assert (L(31)["workgroups"], L(31)["tiles"], L(31)["last"]) == (1, 1, 31)
    assert (L(33)["workgroups"], L(33)["tiles"], L(33)["last"]) == (1, 2, 1)
    a = L(F.N_MID)
    assert (a["workgroups"], a["tiles"], a["most"], a["last"]) == (33, 129, 1, 3)
    for N in F.FUSED_N[:-1]:
        assert L(N)["tiles"] <= F.GRID_CAP * F.WAVES and L(N)["most"] == 1 and L(N)["workgroups"] < F.GRID_CAP
    b = L(F.N_CAP)
    assert F.N_CAP == 1024 * 4 * 32 + 39 and b["tiles"] > F.GRID_CAP * F.WAVES
    # past the cap: two waves take a second tile, the last one has 7 samples
    assert (b["workgroups"], b["tiles"], b["stride"], b["least"], b["most"], b["extra"], b["last"]) == (1024, 4098, 4096, 1, 2, 2, 7)
    assert b == M.fwd_launch(F.N_CAP)                                   # the same rule as launch_fwd of csrc/mlp.hip
    assert max(c.N for c in F.CASES) == F.N_CAP


def test_lds_cases_straddle_the_opt_in():
    from permuto_sdf_amd.mlp import packed_size
    # psdf_mlp_packed_size is the fp32 image that the kernel stages (make_plan) where the net has no split-bf16 image behind it
    # (M.fwd_path 1: the row 64x3 -> 33), and that image plus the split one elsewhere
    for c in F.CASES + F.MASK_CASES:
        if M.fwd_path(c.dims) == 1:
            assert c.row == F.LDS_ROW and F.packed_floats(c.dims) == packed_size(list(c.dims)), c
        else:
            assert 4 * F.packed_floats(c.dims) < F.LDS_OPT_IN and F.packed_floats(c.dims) < packed_size(list(c.dims)), c
    below, above = F.LDS_CASES
    assert (below.row, above.row) == (F.LDS_ROW, F.LDS_ROW) and below.mode == above.mode == F.PADDED
    assert (below.dims[0], above.dims[0]) == (56, 60) and below.N == above.N == F.N_MID
    sizes = [4 * packed_size(list(c.dims)) for c in (below, above)]
    assert sizes[0] < F.LDS_OPT_IN < sizes[1] <= 160 * 1024, sizes
    # no other case opts in
    assert all(4 * F.packed_floats(c.dims) <= F.LDS_OPT_IN for c in F.CASES + F.MASK_CASES if c is not above)
    # the windows the encoding's Setup offers at these level counts
    assert all(c.window == "c2f" for c in F.LDS_CASES)


def test_declined_shapes_have_no_row():
    rows = set(F.fused_rows_in_source(open(SOURCE).read()))
    for levels, mode, dims in F.NO_LAUNCH:
        assert F.channels(levels, mode) == dims[0]
        assert M.sw_sig32(dims) not in rows, dims
    assert [len(d) - 1 for _, _, d in F.NO_LAUNCH] == [3, 4, 4]


@pytest.mark.parametrize("N", (F.N_MID, F.N_CAP))
def test_masks_are_what_their_names_say(N):
    ntiles = -(-N // F.TILE)
    tile = torch.arange(N) // F.TILE
    assert N % F.TILE != 0                                              # the last tile is ragged
    for pattern in (F.FUSED_MASKS if N == F.N_MID else F.FUSED_MASKS_CAP):
        skip, skipped = F.fused_mask(N, pattern)
        assert skip.dtype == torch.uint8 and skip.shape == (N,) and skipped.shape == (N,)
        assert bool((skip.bool() >= skipped).all())
        # a tile is skipped exactly when all its samples below N are masked
        full = {t for t in range(ntiles) if bool(skip[F.TILE * t:F.TILE * t + F.TILE].all())}
        assert set(tile[skipped].tolist()) == full, pattern
        live = set(range(ntiles)) - full
        if pattern == "none":
            assert not full and not bool(skip.any())
        elif pattern == "all":
            assert not live
        elif pattern == "interior_tile":
            assert full == {ntiles // 2} and 0 < ntiles // 2 < ntiles - 1
        elif pattern == "last_tile":
            assert full == {ntiles - 1} and int(skip.sum()) == N - F.TILE * (ntiles - 1) < F.TILE
        elif pattern == "every_second_tile":
            assert full == set(range(1, ntiles, 2)) and live
        elif pattern == "thirty_one_of_thirty_two":
            assert not full and int(skip.sum()) == 31 and int(skip[F.TILE:2 * F.TILE].sum()) == 31
        elif pattern == "last_sample_alone":
            assert full == {ntiles - 2} and int(skip[F.TILE * (ntiles - 1):].sum()) == N - F.TILE * (ntiles - 1) - 1
            assert not bool(skip[N - 1]) and N - F.TILE * (ntiles - 1) > 1
        elif pattern == "second_pass":
            assert full == set(range(4096, ntiles)) and len(full) == 2
        else:
            assert pattern == "first_pass" and full == set(range(4096)) and len(live) == 2
        if pattern not in ("none", "all", "thirty_one_of_thirty_two"):
            assert full and live, pattern


def _torch_forward(lin, x, dtype):
    h = x.to(dtype)
    for i, l in enumerate(lin):
        h = torch.nn.functional.linear(h, l.weight.detach().to(dtype), l.bias.detach().to(dtype))
        if i < len(lin) - 1:
            h = torch.nn.functional.gelu(h)
    return h


@pytest.mark.parametrize("case", [F.FusedCase(c.row, 515, c.levels, c.mode, c.window, c.lattice, c.capacity, c.points)
                                  for c in F.MODE_CASES + F.SCALE_CASES + [F.ROW_CASES[5], F.ROW_CASES[15]]], ids=repr)
def test_reference_on_the_cases_inputs(case):
    """at 515 samples of the case's own point family (the hard family's vertices, 1e3 coordinates and identical points come
    first), on the float64 encoding rounded to fp32"""
    x = F.host_features(case)
    lin = case.net()
    assert x.shape == (515, case.dims[0]) and bool(torch.isfinite(x).all())
    y64, SY, _, _, _, _ = _f64_trace(lin, x, torch.zeros(515, case.dims[-1]))
    assert bool((SY > 0).all())                                         # no entry is excluded
    pin, bad = _per_entry(_torch_forward(lin, x, torch.float64), y64, SY)
    assert not bad and pin <= PIN, pin
    t, _ = _per_entry(_torch_forward(lin, x, torch.float32), y64, SY)
    bar = max(4 * t, FLOOR)
    assert 0 < t <= bar
    # the features of the first level pair swapped (b_even / b_odd exchanged for one pair)
    xs = x.clone()
    xs[:, 0:2], xs[:, 2:4] = x[:, 2:4], x[:, 0:2]
    swapped, _ = _per_entry(_torch_forward(lin, xs, torch.float32), y64, SY)
    # the last two input channels dropped (the last pseudo-level, or the last level without a point)
    xd = x.clone()
    xd[:, -2:] = 0.0
    dropped, _ = _per_entry(_torch_forward(lin, xd, torch.float32), y64, SY)
    print("fused %r on the host: pin %.1e, torch fp32 %.1e, bar %.1e; level pair swapped %.1e, last channels dropped %.1e"
          % (case, pin, t, bar, swapped, dropped))
    if case.lattice == 0.5:
        assert swapped > 100 * bar, (swapped, bar)
    if case.mode != F.NONE:                                             # (without a point the last level is a closed one)
        assert dropped > 100 * bar, (dropped, bar)
