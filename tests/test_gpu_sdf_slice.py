"""GPU: cross-sections of an SDF (permuto_sdf_amd/sdf_slice.py, csrc/sdf_slice.hip) on tiny 3-D and 4-D nets (2^10-entry tables,
4 levels).

  1. the layer's points and skip flags, bit for bit against the torch restatement of visualize_sdf_isolines.py:77-92 (float32
     lattice, float64 rotation, .float()) and `Box.check_point_inside_primitive`;
  2. the SDF plane of `render_slice`, bit for bit one `net_eval.masked_sdf` call over the whole layer, in three chunkings;
  3. its colours: the colorize entry applied to 2's values, and that entry against float64 and the exact band decisions, with
     the bar of tests/host/sdf_slice_kernels_check.cpp:
         bar = u (4 T (K - 1) D + 2 D + 2 M),  u = 2^-24, T = |out_lo| + |scale (clamp(s) - in_lo)|, D the largest step between
         neighbouring control values of the channel, M its largest control value
     (t = out_lo + scale (clamp(s) - in_lo) is 3 roundings, the position t (K - 1) one more; the table is continuous with slope
     <= D; b - a, f (b - a), a + ... round once each; one further u M for second-order terms);
  4. a slice cut into a 41 x 53 view whose base planes are the analytic depth and coverage of a sphere: the mask against the
     float64 decision for every ray that the error bounds of the host program (restated in `decide64`) leave decidable, at most
     1 % excluded;
  5. the conveniences and the refusals."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
H, W = 41, 53


def rotation(axis, deg):
    """[3, 3] float32: the rotation by `deg` about `axis`, float64 rounded (Rodrigues)"""
    a = np.asarray(axis, np.float64)
    a = a / np.sqrt((a * a).sum())
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    th = np.deg2rad(deg)
    return (np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)).astype(np.float32)


def tiny_net(dev, P, iters=150):
    """a small encoded SDF fitted for a moment to |x| - 0.3 (P = 3) or |x - c(t)| - 0.25 (P = 4): enough for its values to
    cross the iso-bands.  An input of 11 or 12 channels has no fused BACKWARD kernel (csrc/mlp_dispatch.h starts at 17): this
    fit, which is the test's set-up and not what it checks, differentiates the MLP through torch and says so; the switch is
    off again before the net is handed out, so everything the tests run is the fused forward."""
    from permuto_sdf_amd import FusedMLP, PermutoEncoding
    from permuto_sdf_amd.optim import FusedAdamW
    torch.manual_seed(0)
    enc = PermutoEncoding(P, 2 ** 10, 4, 2, np.geomspace(1.0, 0.1, 4), concat_points=True, concat_points_scaling=1.0,
                          init_scale=1e-3).to(dev)
    mlp = FusedMLP([enc.output_dims(), 32, 32, 32, 1], allow_torch_fallback=True).to(dev)
    opt = FusedAdamW(list(enc.parameters())[:1] + list(mlp.parameters()), lr=5e-3)
    win = torch.ones(4, device=dev)
    for _ in range(iters):
        x = torch.rand(8192, P, device=dev)
        x[:, :3] -= 0.5
        c = torch.zeros_like(x[:, :3])
        if P == 4:
            c[:, 0] = 0.2 * (x[:, 3] - 0.5)
        target = (x[:, :3] - c).norm(dim=1, keepdim=True) - (0.3 if P == 3 else 0.25)
        loss = ((mlp(enc(x, win)) - target) ** 2).mean()
        for p in opt.param_groups[0]["params"]:
            p.grad = None
        loss.backward()
        opt.step()
    mlp.allow_torch_fallback = False
    return types.SimpleNamespace(encoding=enc, mlp_sdf=mlp, window=lambda it: win, P=P)


@pytest.fixture(scope="module")
def nets(dev):
    return {3: tiny_net(dev, 3), 4: tiny_net(dev, 4)}


@pytest.fixture(scope="module")
def small_box():
    from permuto_sdf_amd.box_trace import Box
    return Box([0.9, 1.2, 0.7], [0.05, -0.1, 0.02])      # smaller than the layer [-1, 1)^2: cells of both kinds


@pytest.fixture(scope="module")
def tilted():
    from permuto_sdf_amd.sdf_slice import SlicePlane
    return SlicePlane(rotation((1.0, 2.0, 3.0), 50.0), -0.057)


# ------------------------------------------------------------------------------------------------------------ 1. the layer
def torch_layer(S, plane):
    """visualize_sdf_isolines.py:75-92 on the CPU: float32 lattice, float64 rotation (x a0 + y a1) + z a2, .float()"""
    layer_width = layer_height = S
    x_coord = torch.arange(layer_width).view(-1, 1, 1).repeat(1, layer_height, 1)
    y_coord = torch.arange(layer_height).view(1, -1, 1).repeat(layer_width, 1, 1)
    z_coord = torch.zeros(layer_width, layer_height).view(layer_width, layer_height, 1)
    z_coord += plane.z
    x_coord = x_coord / layer_width - 0.5
    y_coord = y_coord / layer_height - 0.5
    x_coord = x_coord * 2.0
    y_coord = y_coord * 2.0
    x_coord, y_coord = x_coord * plane.extent_scale, y_coord * plane.extent_scale
    point_layer = torch.cat([x_coord, y_coord, z_coord], 2).transpose(0, 1).reshape(-1, 3)
    assert point_layer.dtype == torch.float32
    V, A = point_layer.double(), torch.from_numpy(plane.axes).double()
    return ((V[:, 0:1] * A[:, 0] + V[:, 1:2] * A[:, 1]) + V[:, 2:3] * A[:, 2]).float()


def layer_on_device(plane, box, S, P, dev, time_val=0.37):
    from permuto_sdf_amd.sdf_slice import slice_points_raw
    pts = torch.full((S * S, P), -77.0, device=dev)
    skip = torch.zeros(S * S, dtype=torch.bool, device=dev)
    time = torch.full((1,), time_val, device=dev) if P == 4 else None
    slice_points_raw(plane, box, S, 0, S * S, pts, skip, time)
    return pts, skip


@pytest.mark.parametrize("S", [1, 37, 129])
def test_points_and_skip_flags_bit_for_bit(dev, small_box, tilted, S):
    from permuto_sdf_amd.sdf_slice import SlicePlane, slice_points_raw
    for plane in (tilted, SlicePlane(tilted.axes, 0.11, extent_scale=0.45)):
        want = torch_layer(S, plane).to(dev)
        want_inside = small_box.check_point_inside_primitive(want).view(-1)
        for P in (3, 4):
            pts, skip = layer_on_device(plane, small_box, S, P, dev)
            assert torch.equal(pts[:, :3], want), (S, P)
            assert P == 3 or bool((pts[:, 3] == 0.37).all())
            assert torch.equal(skip, ~want_inside), (S, P)
        if S > 1 and plane is tilted:
            assert 0 < int(want_inside.sum()) < S * S                      # both kinds of cell
            # a range that starts and ends mid-row writes the same rows, and nothing else
            first, count = 5, S * S - 7
            part, flags = torch.full((count + 2, 3), -77.0, device=dev), torch.zeros(count + 2, dtype=torch.bool, device=dev)
            slice_points_raw(plane, small_box, S, first, count, part[1:-1], flags[1:-1], None)
            assert torch.equal(part[1:-1], want[first:first + count]) and torch.equal(flags[1:-1], ~want_inside[first:first + count])
            assert bool((part[0] == -77.0).all()) and bool((part[-1] == -77.0).all())


# ------------------------------------------------------------------------------------------------------------ 2. the SDF plane
def whole_layer_sdf(net, plane, box, S, dev, time_val):
    """ONE masked evaluation of the whole layer -> (sdf [S S] with 0 at masked cells, skip [S S])"""
    from permuto_sdf_amd.net_eval import masked_sdf, one_row_head
    pts, skip = layer_on_device(plane, box, S, net.P, dev, time_val if time_val is not None else 0.0)
    head = one_row_head(net.mlp_sdf, pack=True)
    sdf = torch.zeros((1, S * S), device=dev)
    feat = torch.zeros((net.encoding.cfg.channels, S * S), device=dev)
    masked_sdf(net.encoding, net.window(0), head.dims, head.packed, pts, skip=skip, out=sdf, feat_buf=feat)
    return sdf.view(-1).masked_fill(skip, 0.0), skip


@pytest.mark.parametrize("P,time_val", [(3, None), (4, 0.25), (4, 0.8)])
def test_sdf_plane_is_one_masked_evaluation_in_every_chunking(dev, nets, small_box, tilted, P, time_val):
    from permuto_sdf_amd.sdf_slice import render_slice
    S, net = 37, nets[P]
    want, skip = whole_layer_sdf(net, tilted, small_box, S, dev, time_val)
    longest = max(len(run) for run in "".join("1" if s else "0" for s in skip.tolist()).split("0"))
    assert longest >= 63 and float(want.abs().max()) > 0.05    # whole 32-sample tiles are masked; the field is not flat
    for chunk in (S * S, 1000, 33):
        img = render_slice(net, tilted, small_box, S, time_val=time_val, max_points_per_chunk=chunk)
        assert tuple(img.sdf.shape) == (1, S, S) and tuple(img.rgb.shape) == (3, S, S)
        assert torch.equal(img.sdf.view(-1), want), (P, chunk)
        assert torch.equal(img.inside.view(-1), (~skip).float())
    if P == 4:      # the time reaches the net
        other = render_slice(net, tilted, small_box, S, time_val=0.5)
        assert not torch.equal(other.sdf.view(-1), want)


# ------------------------------------------------------------------------------------------------------------ 3. the colours
def colorize_on_device(style, values, skipped, dev):
    """the colorize entry over `values` laid out as the first cells of a square layer -> rgb [n, 3], sdf [n], inside [n]"""
    from permuto_sdf_amd.sdf_slice import SliceImage, slice_colorize_raw
    n = len(values)
    S = int(np.ceil(np.sqrt(n + 3)))
    out = SliceImage(*(torch.full((c, S, S), -77.0, device=dev) for c in (3, 1, 1)))
    slice_colorize_raw(style, S, 3, n, torch.as_tensor(values, device=dev), torch.as_tensor(skipped, device=dev), out)
    for plane in (out.rgb, out.sdf, out.inside):      # nothing outside the range
        flat = plane.view(plane.shape[0], -1)
        assert bool((flat[:, :3] == -77.0).all()) and bool((flat[:, 3 + n:] == -77.0).all())
    return (out.rgb.view(3, -1)[:, 3:3 + n].t().cpu().numpy(), out.sdf.view(-1)[3:3 + n].cpu().numpy(),
            out.inside.view(-1)[3:3 + n].cpu().numpy())


def check_colours(style, values, skipped, rgb, sdf_plane, inside_plane):
    """the float64 colour check and the exact band decisions of tests/host/sdf_slice_kernels_check.cpp -> worst error / bar"""
    values, skipped = np.asarray(values, np.float32), np.asarray(skipped, bool)
    lo, hi, band_rgb = style.band_table()
    band = np.full(values.shape, -1)
    with np.errstate(invalid="ignore"):
        for i in range(style.nr_lines):
            band[(values > lo[i]) & (values < hi[i])] = i                 # float32 compares, both strict, the last one wins
    nan = np.isnan(values)
    # skipped cells: 0 in all three planes; the others: the value and 1
    assert not rgb[skipped].any() and not sdf_plane[skipped].any() and not inside_plane[skipped].any()
    live = ~skipped
    assert np.array_equal(sdf_plane[live], values[live], equal_nan=True) and (inside_plane[live] == 1.0).all()
    assert not rgb[live & nan].any()                                      # a NaN matches no band and takes the colour 0
    in_band = live & ~nan & (band >= 0)
    assert np.array_equal(rgb[in_band], band_rgb[band[in_band]])          # bit for bit the band's colour
    base = live & ~nan & (band < 0)
    tab = style.table32().astype(np.float64)
    K = tab.shape[0]
    in_lo, in_hi, out_lo, scale = (float(v) for v in style.base_map32())
    s = values[base].astype(np.float64)
    c = np.minimum(np.maximum(s, in_lo), in_hi)
    t = out_lo + scale * (c - in_lo)
    T = abs(out_lo) + np.abs(scale * (c - in_lo))
    u = np.clip(t, 0.0, 1.0) * (K - 1)
    j = np.minimum(u.astype(np.int64), K - 2)
    want = tab[j] + (u - j)[:, None] * (tab[j + 1] - tab[j])
    D, M = np.abs(np.diff(tab, axis=0)).max(0), np.abs(tab).max(0)
    bar = U * (4.0 * T[:, None] * (K - 1) * D[None, :] + 2.0 * D[None, :] + 2.0 * M[None, :])
    err = np.abs(rgb[base].astype(np.float64) - want)
    assert (err <= bar).all(), float((err / bar).max())
    return float((err / bar).max()) if base.any() else 0.0, int(in_band.sum())


def bound_inputs(style):
    """every lo_i and hi_i, nextafter either side, overlapping centres, negatives, values above 0.3, a NaN; then skipped cells"""
    lo, hi, _ = style.band_table()
    v = []
    for b in np.concatenate([lo, hi]):
        v += [b, np.nextafter(b, np.float32(-np.inf)), np.nextafter(b, np.float32(np.inf))]
    v += [np.float32(i * style.distance + 0.75 * style.distance) for i in range(style.nr_lines)]
    v += [-0.5, -0.01, -1e-30, 0.31, 0.45, 7.0, -np.inf, np.inf, np.nan]
    skipped = [False] * len(v) + [True] * 3
    v += [style.distance, np.nan, 0.1]
    return np.asarray(v, np.float32), np.asarray(skipped, bool)


def test_colorize_against_float64_and_exact_band_decisions(dev):
    from permuto_sdf_amd.sdf_slice import IsoStyle
    worst = 0.0
    for style in (IsoStyle(), IsoStyle(width=0.05), IsoStyle(width=0.004, distance=0.011, nr_lines=32),
                  IsoStyle(table=((0.9, 0.1, 0.5), (0.0, 1.0, 0.5))), IsoStyle(nr_lines=0)):
        values, skipped = bound_inputs(style)
        rng = np.random.default_rng(5)
        values = np.concatenate([values, rng.uniform(-0.1, 0.5, 3000).astype(np.float32)])
        skipped = np.concatenate([skipped, rng.uniform(size=3000) < 0.02])
        w, in_band = check_colours(style, values, skipped, *colorize_on_device(style, values, skipped, dev))
        assert in_band > 0 or style.nr_lines == 0
        worst = max(worst, w)
        if style.width > style.distance:       # overlapping bands: the later one wins
            lo, hi, rgb = style.band_table()
            s = np.float32(0.75 * style.distance)
            assert lo[0] < s < hi[0] and lo[1] < s < hi[1]
            got = colorize_on_device(style, np.asarray([s], np.float32), np.asarray([False]), dev)[0][0]
            assert np.array_equal(got, rgb[1]) and not np.array_equal(rgb[0], rgb[1])
    print("colours: worst error / bar %.3f" % worst)
    assert 0.0 < worst <= 1.0


@pytest.mark.parametrize("P,time_val", [(3, None), (4, 0.25)])
def test_slice_colours_are_the_colorize_entry_on_the_sdf_plane(dev, nets, small_box, tilted, P, time_val):
    from permuto_sdf_amd.sdf_slice import IsoStyle, render_slice
    S, net = 37, nets[P]
    want_sdf, skip = whole_layer_sdf(net, tilted, small_box, S, dev, time_val)
    for style in (IsoStyle(), IsoStyle(width=0.02, distance=0.017)):
        img = render_slice(net, tilted, small_box, S, style=style, time_val=time_val, max_points_per_chunk=1000)
        values, skipped = want_sdf.cpu().numpy(), skip.cpu().numpy()
        rgb, sdf_plane, inside = colorize_on_device(style, values, skipped, dev)
        assert np.array_equal(img.rgb.view(3, -1).t().cpu().numpy(), rgb)
        w, in_band = check_colours(style, values, skipped, rgb, sdf_plane, inside)
        assert in_band > 10 and 0.0 < w <= 1.0                      # the field crosses iso-bands
        # skipped cells are 0 in all three planes
        assert not img.rgb.view(3, -1)[:, skip].any() and not img.sdf.view(-1)[skip].any() and not img.inside.view(-1)[skip].any()


# ------------------------------------------------------------------------------------------------------------ 4. the cut
def scene(dev):
    """the camera, plane, box and sphere of tests/host/sdf_slice_kernels_check.cpp"""
    from permuto_sdf_amd import render
    from permuto_sdf_amd.box_trace import Box
    from permuto_sdf_amd.sdf_slice import SlicePlane
    K = torch.tensor([[40.0, 0.0, 26.5], [0.0, 40.0, 20.5], [0.0, 0.0, 1.0]])
    tf = torch.eye(4)
    tf[:3, :3] = torch.from_numpy(rotation((1.0, 2.0, 3.0), 12.0))
    tf[:3, 3] = torch.tensor([0.15, -0.1, -1.4])
    frame = render.Frame(K.to(dev), tf.to(dev), H, W)
    plane = SlicePlane(rotation((0.1, 1.0, 0.05), 65.0), 0.05, extent_scale=0.45)
    return frame, plane, Box([1.0, 1.0, 0.8], [0.02, -0.03, 0.05])


def sphere_planes(o, d, dev, radius=0.3):
    """the analytic depth and coverage of a sphere about the origin, float64 rounded, and a colour pattern"""
    o, d = o.double().cpu().numpy(), d.double().cpu().numpy()
    b, c = (o * d).sum(1), (o * o).sum(1) - float(np.float32(radius)) ** 2
    disc = b * b - c
    t = -b - np.sqrt(np.maximum(disc, 0.0))
    hit = (disc > 0) & (t > 0)
    weights = torch.from_numpy(hit.astype(np.float32)).view(1, H, W).to(dev)
    depth = torch.from_numpy(np.where(hit, t, 0.0).astype(np.float32)).view(1, H, W).to(dev)
    p = torch.arange(H * W)
    rgb = torch.stack([0.25 + 0.125 * ch + (p % 7).float() * 0.0625 for ch in range(3)]).view(3, H, W).to(dev)
    return rgb, depth, weights


def decide64(plane, box, o, d, weights, depth):
    """the float64 decision of every ray and whether the float32 kernel must agree with it: the error bounds of the host
    program, term for term"""
    o, d = o.double().cpu().numpy(), d.double().cpu().numpy()
    A = plane.axes.astype(np.float64)
    a0, a1, n = A[:, 0], A[:, 1], A[:, 2]
    z, ext = float(np.float32(plane.z)), float(np.float32(plane.extent_scale))
    tr, half = np.asarray(box._tr_c, np.float64), np.asarray(box._half_c, np.float64)
    N, Dn = ((z * n - o) * n).sum(1), (d * n).sum(1)
    errN = 5 * U * (np.abs(n) * (np.abs(z * n) + np.abs(o))).sum(1)
    errD = 3 * U * np.abs(n * d).sum(1)
    ok = np.abs(Dn) > 2 * errD
    with np.errstate(divide="ignore", invalid="ignore"):
        t = N / Dn
        errt = (errN + np.abs(t) * errD) / (np.abs(Dn) - errD) + U * np.abs(t)
        p = o + t[:, None] * d
        errp = np.abs(d) * errt[:, None] + U * np.abs(t[:, None] * d) + U * np.abs(p)
        u, v = (p * a0).sum(1), (p * a1).sum(1)
        erru = (np.abs(a0) * errp).sum(1) + 3 * U * np.abs(a0 * p).sum(1)
        errv = (np.abs(a1) * errp).sum(1) + 3 * U * np.abs(a1 * p).sum(1)
        q = p - tr
        errq = errp + U * np.abs(q)
        ok &= np.abs(t) > errt
        ok &= (np.abs(np.abs(q) - half) > errq).all(1)
        ok &= (np.abs(u + ext) > erru) & (np.abs(u - ext) > erru) & (np.abs(v + ext) > errv) & (np.abs(v - ext) > errv)
        surface = weights != 0
        ok &= ~surface | (np.abs(t - depth) > errt)
        in_box = ((q < half) & (q > -half)).all(1)
        in_layer = (u >= -ext) & (u < ext) & (v >= -ext) & (v < ext)
        take = (t > 0) & in_layer & in_box & (~surface | (t < depth))
    return types.SimpleNamespace(checked=ok, take=take, t=t, errt=errt, Dn=Dn, in_front=t > 0, in_box=in_box, in_layer=in_layer,
                                 surface=surface)


def test_cutting_a_slice_into_a_view(dev, nets):
    from permuto_sdf_amd import _lib as L
    from permuto_sdf_amd import render
    from permuto_sdf_amd.net_eval import masked_sdf, one_row_head
    from permuto_sdf_amd.sdf_slice import IsoStyle, cut_slice_into
    frame, plane, box = scene(dev)
    o, d = render.frame_rays(frame)
    rgb0, depth0, weights0 = sphere_planes(o, d, dev)
    dec = decide64(plane, box, o, d, weights0.view(-1).cpu().numpy(), depth0.view(-1).double().cpu().numpy())
    # the cap on the float64 geometry, and the rays that must be there
    c = dec.checked
    kinds = dict(grazing=int((np.abs(dec.Dn) < 0.02).sum()), behind=int((c & ~dec.in_front).sum()),
                 miss_box=int((c & dec.in_front & ~dec.in_box).sum()), over_sphere=int((c & dec.take & dec.surface).sum()),
                 under_sphere=int((c & ~dec.take & dec.surface & dec.in_front & dec.in_box & dec.in_layer).sum()),
                 no_surface=int((c & dec.take & ~dec.surface).sum()))
    print("cut: %d of %d rays excluded (cap %d); %s" % (int((~c).sum()), H * W, H * W // 100, kinds))
    assert int((~c).sum()) * 100 <= H * W
    assert kinds["grazing"] >= 20 and all(v >= 10 for v in kinds.values()), kinds
    for P, time_val in ((3, None), (4, 0.61)):
        net = nets[P]
        rgb, depth, weights = rgb0.clone(), depth0.clone(), weights0.clone()
        mask = cut_slice_into(net, plane, box, frame, rgb, depth, weights, time_val=time_val)
        m = mask.view(-1).cpu().numpy()
        assert set(np.unique(m)) <= {0.0, 1.0} and tuple(mask.shape) == (1, H, W)
        assert np.array_equal(m[c] == 1.0, dec.take[c]), int(((m == 1.0) != dec.take)[c].sum())
        sl = mask.view(-1) == 1.0
        # untouched pixels keep their bits in all base planes; slice pixels hold t and 1
        assert torch.equal(rgb.view(3, -1)[:, ~sl], rgb0.view(3, -1)[:, ~sl])
        assert torch.equal(depth.view(-1)[~sl], depth0.view(-1)[~sl]) and torch.equal(weights.view(-1)[~sl], weights0.view(-1)[~sl])
        assert bool((weights.view(-1)[sl] == 1.0).all())
        sel = sl.cpu().numpy() & c
        assert (np.abs(depth.view(-1).double().cpu().numpy()[sel] - dec.t[sel]) <= dec.errt[sel]).all()
        # the colours: the begin entry's own points through the net and the colorize rule
        n = H * W
        pts, skip, t = torch.empty((n, P), device=dev), torch.empty(n, dtype=torch.bool, device=dev), torch.empty(n, device=dev)
        time = torch.full((1,), time_val, device=dev) if P == 4 else None
        L.call("psdf_slice_cut_begin", L.c_i(n), L.c_i(P), plane._axes_c, L.c_f(plane.z), L.c_f(plane.extent_scale), box._tr_c,
               box._half_c, L.ptr(o), L.ptr(d), L.ptr(time), L.c_i(H), L.c_i(W), L.c_l(0), L.ptr(weights0), L.ptr(depth0), L.ptr(pts),
               L.ptr(skip), L.ptr(t), L.stream())
        assert torch.equal(~skip, sl) and torch.equal(depth.view(-1)[sl], t[sl]) and not t[skip].any()
        assert torch.equal(pts[skip][:, :3], o[skip]) and (P == 3 or bool((pts[:, 3] == time_val).all()))
        head = one_row_head(net.mlp_sdf, pack=True)
        sdf = torch.zeros((1, n), device=dev)
        masked_sdf(net.encoding, net.window(0), head.dims, head.packed, pts, skip=skip, out=sdf,
                   feat_buf=torch.zeros((net.encoding.cfg.channels, n), device=dev))
        want_rgb = colorize_on_device(IsoStyle(), sdf.view(-1).cpu().numpy(), skip.cpu().numpy(), dev)[0]
        got = rgb.view(3, -1).t().cpu().numpy()
        assert np.array_equal(got[sl.cpu().numpy()], want_rgb[sl.cpu().numpy()])
        assert len(np.unique(got[sl.cpu().numpy()], axis=0)) > 5          # not one flat colour
        # a frame that spans three chunks gives the planes of one chunk bit for bit
        assert render.FramePlan(H, W, 1, 1024).nr_chunks == 3
        rgb3, depth3, weights3 = rgb0.clone(), depth0.clone(), weights0.clone()
        mask3 = cut_slice_into(net, plane, box, frame, rgb3, depth3, weights3, time_val=time_val, max_rays_per_chunk=1024)
        assert torch.equal(mask3, mask) and torch.equal(rgb3, rgb) and torch.equal(depth3, depth) and torch.equal(weights3, weights)


# ------------------------------------------------------------------------------------------------------------ 5. conveniences
def test_conveniences_return_the_planes_of_the_free_functions(dev):
    from permuto_sdf_amd import render, sdf_fit
    from permuto_sdf_amd.box_trace import Box, render_box_traced
    from permuto_sdf_amd.bridge import OccupancyGrid
    from permuto_sdf_amd.sdf_slice import SlicedFrame, SlicePlane, cut_slice_into, render_slice
    from permuto_sdf_amd.train_step import HyperParams, SdfNet
    frame, plane, _ = scene(dev)
    g = torch.Generator().manual_seed(2)
    nrm = torch.nn.functional.normalize(torch.randn(4000, 3, generator=g), dim=1)
    fitter = sdf_fit.SdfFitter(sdf_fit.OrientedCloud((nrm * 0.25).to(dev), nrm.to(dev)), n_surf=1000, n_off=1000)
    for _ in range(3):
        fitter.step()
    box = fitter.box()
    wide = SlicePlane(plane.axes, plane.z)                                   # the reference's [-1, 1): it leaves the unit box
    a, b = fitter.slice(wide, size=48), render_slice(fitter.net, wide, box, 48, it=fitter.iter)
    assert torch.equal(a.rgb, b.rgb) and torch.equal(a.sdf, b.sdf) and torch.equal(a.inside, b.inside)
    assert bool(a.inside.any()) and not bool(a.inside.all())
    # render() without a slice: the planes of the tree before this module
    plain, want = fitter.render(frame, nr_sphere_traces=5), render_box_traced(fitter.net, box, frame, it=fitter.iter, nr_sphere_traces=5)
    assert type(plain) is type(want) and plain.normals_cam is None
    assert all(torch.equal(getattr(plain, k), getattr(want, k)) for k in ("normals", "weights_sum", "depth"))
    # render(slice=...): (n + 1) / 2 with the slice cut in
    cut = fitter.render(frame, slice=plane, nr_sphere_traces=5)
    assert isinstance(cut, SlicedFrame) and cut.depth is cut.base.depth and cut.weights_sum is cut.base.weights_sum
    rgb = (want.normals + 1.0) * 0.5
    mask = cut_slice_into(fitter.net, plane, box, frame, rgb, want.depth, want.weights_sum, it=fitter.iter)
    assert torch.equal(cut.rgb, rgb) and torch.equal(cut.depth, want.depth) and torch.equal(cut.weights_sum, want.weights_sum)
    assert torch.equal(cut.slice_mask, mask) and bool(mask.any()) and torch.equal(cut.base.normals, want.normals)
    # the frame renderer's SDF net (1 + 32 outputs), with the cube of its occupancy grid as the box
    hp = HyperParams()
    torch.manual_seed(3)
    holder = types.SimpleNamespace(sdf=SdfNet(hp).to(dev), rgb=None, bg=None, grid=OccupancyGrid(32, 1.0, [0.0, 0.0, 0.0], device=dev),
                                   sphere=None, hp=hp, with_mask=False)
    rnd = render.FrameRenderer(holder)
    assert rnd.box().sizes_xyz == [1.0, 1.0, 1.0] and rnd.box().translation == [0.0, 0.0, 0.0]
    a, b = rnd.slice(plane, size=48), render_slice(holder.sdf, plane, Box([1.0, 1.0, 1.0]), 48)
    assert torch.equal(a.rgb, b.rgb) and torch.equal(a.sdf, b.sdf) and torch.equal(a.inside, b.inside) and bool(a.sdf.any())


def test_refusals(dev, nets):
    from permuto_sdf_amd import render
    from permuto_sdf_amd._lib import PsdfError
    from permuto_sdf_amd.sdf_slice import IsoStyle, cut_slice_into, render_slice
    frame, plane, box = scene(dev)
    planes = lambda device: (torch.zeros(3, H, W, device=device), torch.zeros(1, H, W, device=device), torch.zeros(1, H, W, device=device))
    # mixed devices
    with pytest.raises(PsdfError):
        cut_slice_into(nets[3], plane, box, frame, *planes("cpu"))
    with pytest.raises(PsdfError):
        cut_slice_into(nets[3], plane, box, render.Frame(frame.K.cpu(), frame.tf_world_cam.cpu(), H, W), *planes(dev))
    cpu_net = types.SimpleNamespace(encoding=nets[3].encoding.__class__(3, 2 ** 10, 4, 2, np.geomspace(1.0, 0.1, 4)), mlp_sdf=nets[3].mlp_sdf,
                                    window=nets[3].window)
    with pytest.raises(PsdfError):
        render_slice(cpu_net, plane, box, 16)
    # a wrong time
    for P, wrong in ((3, 0.5), (4, None)):
        with pytest.raises(ValueError):
            render_slice(nets[P], plane, box, 16, time_val=wrong)
        with pytest.raises(ValueError):
            cut_slice_into(nets[P], plane, box, frame, *planes(dev), time_val=wrong)
    # size < 1, a table with K < 2, planes of another shape
    with pytest.raises(ValueError):
        render_slice(nets[3], plane, box, 0)
    with pytest.raises(ValueError):
        IsoStyle(table=((0.5, 0.5, 0.5),))
    with pytest.raises(ValueError):
        cut_slice_into(nets[3], plane, box, frame, torch.zeros(3, H, W + 1, device=dev), *planes(dev)[1:])
