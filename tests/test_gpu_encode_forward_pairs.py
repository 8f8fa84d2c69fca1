"""GPU: the paired launch form of the encode forward (a coarse level and a fine one per thread, csrc/encode.hip:
encode_fwd_pair_kernel) writes the same BYTES as the one-level-per-grid-row form, for every number of pairs.

The form is a process-wide setting (psdf_encode_set_forward_pairs); every comparison here runs the same seeded inputs through
pairs = 0 and through every pairs in 1 .. L // 2 and compares the outputs as integers (so NaN payloads and the sign of a zero
count).  Inputs are made once per shape and never written to."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NS = (1, 255, 257, 1000, 4099)
LS = (1, 2, 3, 5, 16)
PFS = ((3, 2), (4, 2), (2, 2), (3, 4))
CAPS = (2 ** 18, 100003)
CONCATS = (None, "pseudo_levels", "append")
WINDOWS = ("open", "coarse_closed", "fine_closed", "all_closed")
SENTINEL = 1234.5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


@pytest.fixture()
def set_pairs():
    from permuto_sdf_amd import _lib as L

    def f(n):
        L.call("psdf_encode_set_forward_pairs", L.c_i(n))
    yield f
    f(-1)


_cache = {}


def _inputs(dev, P, F, L, cap, fine_first=False):
    """(lattice [L, cap, F], scale_factor [L, P], shifts [L, P], positions [max N, P]) -- seeded, shared, read-only"""
    key = (P, F, L, cap, fine_first)
    if key not in _cache:
        from permuto_sdf_amd.encoding import scale_factor_tensor
        g = torch.Generator().manual_seed(1000 * P + 100 * F + L + cap % 7)
        scales = np.geomspace(1.0, 1e-4, L)
        if fine_first:
            scales = scales[::-1].copy()
        _cache[key] = ((torch.randn(L, cap, F, generator=g) * 0.1).to(dev), scale_factor_tensor(scales, P).to(dev),
                       torch.randn(L, P, generator=g).to(dev), ((torch.rand(max(NS), P, generator=g) - 0.5) * 0.9).to(dev))
    return _cache[key]


def _window(kind, L, dev):
    w = torch.ones(L)
    k = max(1, L // 3)
    if kind == "coarse_closed":
        w[:k] = 0.0
    elif kind == "fine_closed":
        w[L - k:] = 0.0
    elif kind == "all_closed":
        w[:] = 0.0
    else:
        w = 0.25 + 0.75 * torch.linspace(1.0, 0.1, L)      # open, and not all ones: the window is a factor of every weight
    return w.to(dev)


def _cfg(P, F, L, cap, concat):
    from permuto_sdf_amd.encoding import _Cfg
    return _Cfg(P, cap, L, F, concat is not None, 1e-3, concat_layout=concat)


def _bits(t):
    return t.view(torch.int32)


def _forward(cfg, pos, lat, sf, sh, win, **kw):
    from permuto_sdf_amd.encoding import encode_forward_raw
    out = torch.full((cfg.channels, pos.shape[0]), SENTINEL, dtype=torch.float32, device=pos.device)
    return encode_forward_raw(cfg, pos, lat, sf, sh, win, out=out, **kw)


@pytest.mark.parametrize("concat", CONCATS, ids=lambda c: c or "no_concat")
@pytest.mark.parametrize("P,F", PFS)
def test_every_number_of_pairs_writes_the_same_bytes(dev, set_pairs, P, F, concat):
    for cap in CAPS:
        for L in LS:
            lat, sf, sh, allpos = _inputs(dev, P, F, L, cap)
            cfg = _cfg(P, F, L, cap, concat)
            for kind in WINDOWS:
                win = _window(kind, L, dev)
                for N in NS:
                    pos = allpos[:N].contiguous()
                    set_pairs(0)
                    want = _forward(cfg, pos, lat, sf, sh, win)
                    if kind == "open":
                        assert bool((want[:L * F] != SENTINEL).all()) and bool(want[:L * F].abs().max() > 0)
                    for pairs in range(1, L // 2 + 1):
                        set_pairs(pairs)
                        got = _forward(cfg, pos, lat, sf, sh, win)
                        assert torch.equal(_bits(got), _bits(want)), (cap, L, kind, N, pairs)
                    # beyond L // 2 the count is clamped, and -1 is the library's own rule: same bytes again
                    for pairs in (L // 2 + 3, -1):
                        set_pairs(pairs)
                        assert torch.equal(_bits(_forward(cfg, pos, lat, sf, sh, win)), _bits(want)), (cap, L, kind, N, pairs)


@pytest.mark.parametrize("P,F", PFS)
def test_masked_columns_keep_their_sentinel_bytes(dev, set_pairs, P, F):
    for cap in CAPS:
        for L in LS:
            lat, sf, sh, allpos = _inputs(dev, P, F, L, cap)
            cfg = _cfg(P, F, L, cap, "pseudo_levels")
            for kind in ("open", "coarse_closed"):
                win = _window(kind, L, dev)
                for N in NS:
                    pos = allpos[:N].contiguous()
                    skip = (torch.arange(N, device=dev) % 3 == 1).to(torch.uint8)
                    set_pairs(0)
                    want = _forward(cfg, pos, lat, sf, sh, win, skip=skip)
                    assert bool((want[:, skip.bool()] == SENTINEL).all())
                    if N > 1:
                        assert bool((want[:L * F][:, ~skip.bool()] != SENTINEL).all())
                    for pairs in range(1, L // 2 + 1):
                        set_pairs(pairs)
                        got = _forward(cfg, pos, lat, sf, sh, win, skip=skip)
                        assert torch.equal(_bits(got), _bits(want)), (cap, L, kind, N, pairs)


@pytest.mark.parametrize("P,F", PFS)
def test_touched_block_maps_are_byte_equal(dev, set_pairs, P, F):
    shift = 7
    for cap in CAPS:
        for L in LS:
            lat, sf, sh, allpos = _inputs(dev, P, F, L, cap)
            cfg = _cfg(P, F, L, cap, "pseudo_levels")
            for kind in ("open", "fine_closed"):
                win = _window(kind, L, dev)
                for N in NS:
                    pos = allpos[:N].contiguous()
                    maps = []
                    for pairs in range(0, L // 2 + 1):
                        set_pairs(pairs)
                        touched = torch.zeros((L, (cap + (1 << shift) - 1) >> shift), dtype=torch.uint8, device=dev)
                        out = _forward(cfg, pos, lat, sf, sh, win, touched=touched, block_rows_log2=shift)
                        maps.append((touched, out))
                    assert int(maps[0][0].sum()) > 0 or kind != "open"
                    for pairs, (touched, out) in enumerate(maps[1:], 1):
                        assert torch.equal(touched, maps[0][0]), (cap, L, kind, N, pairs)
                        assert torch.equal(_bits(out), _bits(maps[0][1])), (cap, L, kind, N, pairs)


def test_fine_levels_first_is_byte_equal_too(dev, set_pairs):
    """The plan takes the levels as ordered coarse to fine by index; that is a speed heuristic only.  Here the scale list runs the
    other way (index 0 is the finest level): every form still writes the same bytes."""
    P, F, L, cap, N = 3, 2, 16, 2 ** 18, 4099
    lat, sf, sh, allpos = _inputs(dev, P, F, L, cap, fine_first=True)
    assert float(sf[0, 0]) > float(sf[-1, 0])       # scale_factor = 1 / (term * scale): index 0 is the finest
    cfg = _cfg(P, F, L, cap, "pseudo_levels")
    win = _window("open", L, dev)
    pos = allpos[:N].contiguous()
    set_pairs(0)
    want = _forward(cfg, pos, lat, sf, sh, win)
    for pairs in range(1, L // 2 + 1):
        set_pairs(pairs)
        assert torch.equal(_bits(_forward(cfg, pos, lat, sf, sh, win)), _bits(want)), pairs


def test_the_setter_rejects_what_it_cannot_mean(dev, set_pairs):
    from permuto_sdf_amd import _lib as L
    with pytest.raises(L.PsdfError):
        set_pairs(-2)
