"""The cases of the fused encode -> MLP forward (fused_fwd_kernel of csrc/fused.hip through psdf_encode_mlp_forward): nets,
encodings, batch sizes, launch arithmetic and skip patterns, shared by tests/test_fused_cases.py (host: asserts every claim made
here) and tests/test_gpu_fused_float64.py (device).  No test in here.

The launch (launch_fused): 256 threads = 4 waves per workgroup, wave w of workgroup b walks the 32-sample tiles 4 b + w, + 4 x
workgroups, ..; min(ceil(tiles / 4), 1024) workgroups; the fp32 image of psdf_mlp_pack (make_plan's total, the head of the
psdf_mlp_packed_size floats) is staged in LDS, with hipFuncSetAttribute above 64 KiB.  A tile is skipped when all its samples
below N are masked."""
import re

import torch

from tests import mlp_float64 as M

NONE, PADDED, APPENDED = 0, 1, 2                    # PSDF_ENC_CONCAT_* of csrc/encode_conventions.h
MODE_NAMES = {NONE: "none", PADDED: "padded", APPENDED: "appended"}

# one net per CASE(...) row of psdf_encode_mlp_forward, hidden widths and outputs; the out width is no multiple of a tile where
# the row allows it: 3 of the 1..4 a final-dot row takes, 33 (one MFMA tile + 1 row) on the MFMA rows
FUSED_ROWS = {
    (2, 2, 2, 1, True): ((64, 64, 64), 3),       # 64x3 -> 1..4   (BASELINE SDF net)
    (1, 1, 1, 1, True): ((32, 32, 32), 3),       # 32x3 -> 1..4
    (1, 1, 1, 2, False): ((32, 32, 32), 33),     # 32x3 -> 33     (reference SDF net)
    (2, 2, 2, 2, False): ((64, 64, 64), 33),     # 64x3 -> 33
}
BASE_ROW, REF_ROW, LDS_ROW = (2, 2, 2, 1, True), (1, 1, 1, 2, False), (2, 2, 2, 2, False)
# 1: one sample; 31 / 33: one tile - 1 / + 1 (33: a second wave on a tile of one sample); 4 099 = 128 tiles + 3 samples: 33
# workgroups, the last with one wave at work; 131 111 = 1024 x 4 x 32 + 39 (M.SW_N_FWD): past the cap of 1024 workgroups, two
# waves take a second tile, the last tile has 7 samples
FUSED_N = (1, 31, 33, 4_099, 131_111)
N_MID, N_CAP = 4_099, 131_111
GRID_CAP, WAVES, TILE = 1024, 4, 32
LDS_OPT_IN = 64 * 1024                              # launch_fused asks for the attribute above this many bytes
LDS_LEVELS = (26, 28)                               # row 64x3 -> 33 with a padded point: K0 = 56 below, K0 = 60 above 64 KiB
CAPACITY, CAPACITY_ODD = 2 ** 14, 2 ** 14 + 37      # a mask, and the runtime modulo, in vertex_rows


def channels(levels, mode):
    return {NONE: 2 * levels, PADDED: 2 * (levels + 2), APPENDED: 2 * levels + 3}[mode]


class FusedCase:
    """one launch family: the encoding (levels, concat mode, window of tests/test_gpu_encode_float64.py's Setup, lattice scale,
    table rows, point family), the net of a row, N; feat64: the feat by-product is also held against oracle/encode_float64.py;
    conv: encoding conventions set for the case (permuto_sdf_amd.conventions.set keywords)"""

    def __init__(self, row, N, levels=16, mode=PADDED, window="mixed", lattice=0.5, capacity=CAPACITY, points="hard",
                 feat64=False, conv=None):
        self.row, self.N, self.levels, self.mode, self.window, self.lattice, self.capacity, self.points, self.feat64 = \
            row, N, levels, mode, window, lattice, capacity, points, feat64
        self.conv = dict(conv or {})
        hidden, out = FUSED_ROWS[row]
        self.dims = (channels(levels, mode),) + tuple(hidden) + (out,)

    def key(self):
        return (self.dims, self.N, self.levels, self.mode, self.window, self.lattice, self.capacity, self.points,
                tuple(sorted(self.conv.items())))

    def seed(self):
        import zlib
        return zlib.crc32(repr(self.key()).encode())

    def net(self):
        return M.mlp_net(self.dims, self.seed())

    def __repr__(self):
        conv = "".join(" %s=%d" % kv for kv in sorted(self.conv.items()))
        return "%s N=%d L=%d %s %s lattice=%g T=%d %s%s" % ("-".join(map(str, self.dims)), self.N, self.levels,
                                                          MODE_NAMES[self.mode], self.window, self.lattice, self.capacity,
                                                          self.points, conv)


# every row at every batch: 16 levels + padded point (K0 = 36), the hard point family, the mixed window (level 2 closed)
ROW_CASES = [FusedCase(row, N) for row in FUSED_ROWS for N in FUSED_N]
# concat modes at 16 levels (C = 32 / 36 / 35) and at 3 levels (C = 6 / 10 / 9: 3 / 5 / 5 k-steps, the last level pair half
# empty); the runtime modulo; the coarse-to-fine window (its last levels closed) at 16 levels; feat against float64 in all six
MODE_CASES = [FusedCase(BASE_ROW if levels == 16 else REF_ROW, N_MID, levels=levels, mode=mode, capacity=CAPACITY_ODD,
                        window="c2f" if levels == 16 else "mixed", feat64=True)
              for levels in (16, 3) for mode in (NONE, PADDED, APPENDED)]
# lattice values at initialisation scale (1e-5: the features are far below the point channels and the biases)
SCALE_CASES = [FusedCase(row, N_MID, lattice=1e-5, window="c2f") for row in (BASE_ROW, REF_ROW)]
# the dynamic-LDS opt-in: below and above 64 KiB.  Points on rays inside the unit box: at 2^-25 and finer an elevated
# coordinate of the 1e3 family is past 2^31, where the simplex is no longer defined.  (The mixed window has 24 entries.)
LDS_CASES = [FusedCase(LDS_ROW, N_MID, levels=L, points="rays", window="c2f") for L in LDS_LEVELS]
# rank ties (lattice vertices and faces) under both tie rules, and a second hash multiplier
CONV_CASES = [FusedCase(BASE_ROW, N_MID, points="vertices", conv={"rank_tie_raises_later": 0}),
              FusedCase(BASE_ROW, N_MID, points="vertices", conv={"rank_tie_raises_later": 1, "hash_multiplier": 2654435761})]
CASES = ROW_CASES + MODE_CASES + SCALE_CASES + LDS_CASES + CONV_CASES

# the masked cases: every row at 4 099 (129 tiles, the last of 3 samples), two rows past the grid cap
MASK_CASES = [FusedCase(row, N_MID) for row in FUSED_ROWS] + [FusedCase(row, N_CAP) for row in (BASE_ROW, REF_ROW)]
# "last_tile" at these N is the ragged last tile with all its real samples masked: its lanes n >= N read the mask of N - 1
FUSED_MASKS = ("none", "all", "interior_tile", "last_tile", "every_second_tile", "thirty_one_of_thirty_two",
               "last_sample_alone")
# past the cap: whole tiles masked in the second grid pass (the waves that take a second tile compute, then skip), the reverse,
# and alternating tiles
FUSED_MASKS_CAP = ("second_pass", "first_pass", "every_second_tile")

# shapes the entry admits but has no launch for: (levels, mode, dims)
NO_LAUNCH = [(38, PADDED, (80, 64, 64, 3)),                 # n_layers == 3: no CASE with t3 == 0
             (16, PADDED, (36, 128, 128, 128, 1)),          # hidden 128
             (16, PADDED, (36, 64, 32, 64, 1))]             # hidden 64-32-64


def fused_rows_in_source(text):
    """the CASE(t1, t2, t3, to, final_dot) rows of csrc/fused.hip as tile signatures (M.sw_sig32)"""
    rows = re.findall(r"^\s*CASE\((\d+),\s*(\d+),\s*(\d+),\s*(\d+),\s*(true|false)\)", text, re.M)
    return [(int(a), int(b), int(c), int(o), d == "true") for a, b, c, o, d in rows]


def fused_launch(N):
    """launch_fused restated -> workgroups, tiles, stride, tiles of the idlest / busiest wave, waves with the larger count,
    samples of the last tile"""
    ntiles = -(-N // TILE)
    r = M._walk(ntiles, min(-(-ntiles // WAVES), GRID_CAP), WAVES)
    r["last"] = N - TILE * (ntiles - 1)
    return r


def packed_floats(dims):
    """make_plan of csrc/mlp_device.h restated: floats of the fp32 image, which is what the kernel stages in LDS (the host test
    pins it to psdf_mlp_packed_size on the nets whose packed buffer has no split-bf16 image behind it)"""
    nl = len(dims) - 1
    t = [(w + 31) // 32 for w in dims]
    dot = dims[-1] <= 4
    off = 0
    for l in range(nl):
        last = l == nl - 1
        if l == 0:
            off += t[1] * ((dims[0] + 1) // 2) * 65
        elif last and dot:
            off += dims[-1] * t[l] * 32
        else:
            off += t[l + 1] * t[l] * 16 * 64
        off += 4 if (last and dot) else t[l + 1] * 32
    return off


def fused_mask(N, pattern):
    """-> (skip [N] uint8, skipped [N] bool: the samples of fully masked tiles, whose columns of Y and feat must keep their
    contents).  interior_tile: tile tiles // 2; last_tile: the last tile; every_second_tile: the odd tiles;
    thirty_one_of_thirty_two: tile 1 but for its sample 7 (a live tile: all 32 are evaluated); last_sample_alone: the last two
    tiles but for sample N - 1 (the last tile is live through its last real lane only); second_pass / first_pass: the tiles
    from / below the launch's stride (4096)"""
    ntiles = -(-N // TILE)
    tile = torch.arange(N) // TILE
    stride = fused_launch(N)["stride"]
    if pattern == "none":
        skip = torch.zeros(N, dtype=torch.bool)
    elif pattern == "all":
        skip = torch.ones(N, dtype=torch.bool)
    elif pattern == "interior_tile":
        assert 0 < ntiles // 2 < ntiles - 1
        skip = tile == ntiles // 2
    elif pattern == "last_tile":
        skip = tile == ntiles - 1
    elif pattern == "every_second_tile":
        skip = tile % 2 == 1
    elif pattern == "thirty_one_of_thirty_two":
        assert ntiles > 2
        skip = tile == 1
        skip[TILE + 7] = False
    elif pattern == "last_sample_alone":
        assert ntiles > 2
        skip = tile >= ntiles - 2
        skip[N - 1] = False
    elif pattern == "second_pass":
        skip = tile >= stride
    else:
        assert pattern == "first_pass", pattern
        skip = tile < stride
    live_tiles = torch.zeros(ntiles, dtype=torch.bool)
    live_tiles[tile[~skip]] = True
    return skip.to(torch.uint8), ~live_tiles[tile]


def host_features(case):
    """[N, C] fp32 on the CPU: the float64 encoding of the case's points rounded to fp32 -- what the kernel's feat by-product
    holds up to the bar of the device test; the host test's stand-in for it"""
    from tests.test_gpu_encode_float64 import Setup
    s = make_setup(torch.device("cpu"), case)
    pts = s.points(case.points, case.N)
    return s.evaluator(pts).forward()[0].float()


def make_setup(dev, case):
    """the Setup of tests/test_gpu_encode_float64.py (power-of-two scales, a zero-shift level, its windows and point families)
    for the case: its concat mode (Setup knows the padded layout only), lattice scale and table rows"""
    from permuto_sdf_amd.encoding import _Cfg
    from tests.test_gpu_encode_float64 import Setup
    s = Setup(dev, 3, 2, case.capacity, L=case.levels, window=case.window, seed=case.seed() % 1000, concat=case.mode != NONE)
    if case.mode == APPENDED:
        s.cfg = _Cfg(3, case.capacity, case.levels, 2, True, 1e-3, APPENDED)
        s.mode, s.C = int(s.cfg.concat_mode), s.cfg.channels
    assert s.mode == case.mode and s.C == case.dims[0], (case, s.mode, s.C)
    s.lat = (s.lat * (case.lattice / 0.5)).contiguous()
    return s
