"""GPU: mesh extraction (permuto_sdf_amd/mesh.py over csrc/mesh.hip) against the repository's own host stand-in,
compat/skimage/measure.py, fed the same fp32 volume.  The stand-in is the yardstick, not under test: its vertex order is the
sorted order of its edge keys lo * N + hi, which this file recomputes from the volume (every grid edge of the seven direction
classes whose ends differ in `inside`) and checks against the stand-in's own positions before it relies on them.

Derived bars (u = 2^-24, the bound on the relative error of one fp32 rounding; the device's `/` and sqrtf are correctly rounded):
  positions  t = fl(f_lo / fl(f_lo - f_hi)) from the stand-in's own fp32 f: r = 2 roundings on t <= 1; p = fl(x + t) and the
             stand-in's final cast to fp32 are one rounding each of a value below max(X, Y, Z): (r + 2 max(X, Y, Z)) u.
  normals    per component of g = g_lo + (g_hi - g_lo) t: 1 (central difference; the halving is exact) on each of g_lo, g_hi,
             1 on their difference, 2 carried by t, 1 on the product, 1 on the sum, each of a quantity below |g_lo| + |g_hi|:
             7 u (|g_lo| + |g_hi|), which the normalisation divides by |g|; the norm itself (three squares and two sums of
             positive terms 3 u, halved by the root, + 1 for the root), the division and the stand-in's cast to fp32 add
             1.5 + 1 + 1 + 1 <= 5 roundings of a component below 1.  With (|g_lo| + |g_hi|) / |g| >= 1:
             |n - n_ref| <= NORMAL_ROUNDINGS u (|g_lo| + |g_hi|) / |g| with NORMAL_ROUNDINGS = 12 (first order in u).
"""
import importlib.util
import os
import subprocess
import sys
import warnings
from unittest import mock

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
T_ROUNDINGS = 2
NORMAL_ROUNDINGS = 12
# corner offsets (dx, dy, dz) of the seven edge classes
OFFSETS = [(dx, dy, dz) for dx in (0, 1) for dy in (0, 1) for dz in (0, 1)][1:]


def _load_standin():
    spec = importlib.util.spec_from_file_location("_standin_measure", os.path.join(ROOT, "compat", "skimage", "measure.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


STANDIN = _load_standin()


class _IgnoresNan(np.ndarray):
    """the stand-in refuses a volume that holds a NaN (`vol.min()` is NaN); its algorithm below that check is well defined
    (NaN is outside).  Handing it an array whose min / max skip NaN runs that algorithm unchanged."""

    def min(self, *a, **k):
        return np.nanmin(np.asarray(self))

    def max(self, *a, **k):
        return np.nanmax(np.asarray(self))


class _NumpyProxy:
    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def asarray(a, *args, **kw):
        return np.asarray(a, *args, **kw).view(_IgnoresNan)


def standin(vol, level, ignore_nan=False):
    """-> verts f32 [V,3], faces [F,3], normals f32, keys [V] (sorted lo * N + hi), lo [V], hi [V]"""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")        # inf - inf, 0 / 0 on the non-finite volume
        if ignore_nan:
            with mock.patch.object(STANDIN, "np", _NumpyProxy()):
                out = STANDIN.marching_cubes(vol, level)
        else:
            out = STANDIN.marching_cubes(vol, level)
    verts, faces, normals = (np.asarray(a) for a in out[:3])
    X, Y, Z = vol.shape
    N = X * Y * Z
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        inside = (vol - np.float32(level)) < 0
    lin = np.arange(N, dtype=np.int64).reshape(X, Y, Z)
    los, his = [], []
    for dx, dy, dz in OFFSETS:
        a = (slice(0, X - dx), slice(0, Y - dy), slice(0, Z - dz))
        b = (slice(dx, X), slice(dy, Y), slice(dz, Z))
        cross = inside[a] != inside[b]
        los.append(lin[a][cross])
        his.append(lin[b][cross])
    lo, hi = np.concatenate(los), np.concatenate(his)
    order = np.argsort(lo * N + hi)
    lo, hi = lo[order], hi[order]
    assert len(lo) == len(verts), "the recomputed edge set is not the stand-in's"
    # the recomputed keys ARE the stand-in's vertex order: its positions follow from them exactly
    v = (vol - np.float32(level)).reshape(-1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        t = v[lo].astype(np.float64) / (v[lo].astype(np.float64) - v[hi].astype(np.float64))
        xyz = lambda i: np.stack([i // (Y * Z), (i // Z) % Y, i % Z], 1).astype(np.float64)      # noqa: E731
        mine = (xyz(lo) + (xyz(hi) - xyz(lo)) * t[:, None]).astype(np.float32)
    assert np.array_equal(mine, verts, equal_nan=True)
    return verts, faces.astype(np.int64), normals, lo * N + hi, lo, hi


def sphere(shape, radius, centre=None):
    X, Y, Z = shape
    c = centre if centre is not None else [(s - 1) / 2 + 0.13 for s in shape]
    g = np.stack(np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing="ij"), -1).astype(np.float64)
    return (np.linalg.norm(g - np.array(c), axis=-1) - radius).astype(np.float32)


def volumes():
    rng = np.random.default_rng(7)
    noise = rng.standard_normal((48, 48, 48)).astype(np.float32)
    bad = rng.standard_normal((36, 36, 36)).astype(np.float32)
    idx = rng.integers(0, 36, size=(12, 3))
    for k, (i, j, l) in enumerate(idx):
        bad[i, j, l] = (np.nan, np.inf, -np.inf)[k % 3]
    two = np.array([[[-1.0, 2.0], [0.5, -0.25]], [[3.0, -0.0], [0.0, 1.0]]], dtype=np.float32)
    return {
        "sphere64": (sphere((64, 64, 64), 20.3), 0.0),
        "sphere128": (sphere((128, 128, 128), 45.7), 0.0),
        "sphere33x70x129": (sphere((33, 70, 129), 12.4), 0.0),
        "noise48": (noise, 0.0),
        "integers40": (rng.integers(-2, 3, size=(40, 40, 40)).astype(np.float32), 0.0),
        "sphere64_level": (sphere((64, 64, 64), 20.3) * 0.01, 0.05),
        "two": (two, 0.0),
        "nonfinite36": (bad, 0.0),
    }


VOLUMES = volumes()
SPHERES = ("sphere64", "sphere128", "sphere33x70x129", "sphere64_level")


def _rows_sorted(a):
    a = np.asarray(a)
    return a[np.lexsort(a.T[::-1])]


def _cyclic(f):
    """rotate every triangle so that its smallest index comes first (orientation kept)"""
    f = np.asarray(f)
    k = f.argmin(1)
    r = np.arange(len(f))
    return np.stack([f[r, k], f[r, (k + 1) % 3], f[r, (k + 2) % 3]], 1)


def _directed(f, V):
    f = np.asarray(f, dtype=np.int64)
    return np.concatenate([f[:, 0] * V + f[:, 1], f[:, 1] * V + f[:, 2], f[:, 2] * V + f[:, 0]])


@pytest.mark.parametrize("name", list(VOLUMES))
def test_generic_entry_against_the_standin(dev, name, capsys):
    from permuto_sdf_amd.mesh import marching_tetrahedra
    vol, level = VOLUMES[name]
    nonfinite = name == "nonfinite36"
    if name == "integers40":
        assert int((vol == 0).sum()) > 5000
    rv, rf, rn, keys, lo, hi = standin(vol, level, ignore_nan=nonfinite)
    X, Y, Z = vol.shape
    N = X * Y * Z
    verts, faces, normals, values, edges = marching_tetrahedra(torch.from_numpy(vol).to(dev), level, return_edges=True,
                                                               _check_range=not nonfinite)
    verts, faces, normals, edges = verts.cpu().numpy(), faces.cpu().numpy().astype(np.int64), normals.cpu().numpy(), edges.cpu().numpy()
    assert values.shape == (len(verts),) and bool((values == np.float32(level)).all())
    # the vertex-edge set, in the stand-in's order (so vertex indices mean the same on both sides)
    assert edges.shape == (len(keys), 2) and np.array_equal(edges[:, 0], lo) and np.array_equal(edges[:, 1], hi)
    V = len(keys)
    assert 20 <= V or name == "two"
    # every face, as an unordered triple, with multiplicity
    assert faces.shape == rf.shape
    assert np.array_equal(_rows_sorted(np.sort(faces, 1)), _rows_sorted(np.sort(rf, 1)))
    if name in SPHERES:      # on smooth data the stand-in's finite-difference orientation is the combinatorial one
        assert np.array_equal(_rows_sorted(_cyclic(faces)), _rows_sorted(_cyclic(rf)))
    d = _directed(faces, V)
    assert len(np.unique(d)) == len(d), "a directed edge occurs twice: the orientation is not consistent"
    if name in SPHERES:
        rev = _directed(faces[:, ::-1], V)
        assert np.array_equal(np.sort(d), np.sort(rev))
        assert V - len(d) // 2 + len(faces) == 2
    # positions: every vertex whose stand-in position is finite
    finite = np.isfinite(rv).all(1)
    if not nonfinite:
        assert finite.all()
    else:
        bad = ~np.isfinite(vol.reshape(-1))
        assert (bad[lo[~finite]] | bad[hi[~finite]]).all() and 0 < (~finite).sum() <= 7 * 2 * int(bad.sum())
    bar = (T_ROUNDINGS + 2 * max(X, Y, Z)) * U
    err = np.abs(verts[finite].astype(np.float64) - rv[finite].astype(np.float64)).max()
    with capsys.disabled():
        print("\n  %-16s V %7d F %7d  worst position error / bar = %.3f" % (name, V, len(faces), err / bar))
    assert np.isfinite(verts[finite]).all() and err <= bar
    # normals of the generic entry (the stand-in's: interpolated volume gradient), on the spheres
    if name in SPHERES:
        g = np.stack(np.gradient(vol.astype(np.float64)), -1).reshape(-1, 3)
        t = (vol.reshape(-1)[lo] - np.float32(level)).astype(np.float64)
        t = t / (t - (vol.reshape(-1)[hi] - np.float32(level)).astype(np.float64))
        gi = g[lo] + (g[hi] - g[lo]) * t[:, None]
        scale = (np.linalg.norm(g[lo], axis=1) + np.linalg.norm(g[hi], axis=1)) / np.linalg.norm(gi, axis=1)
        nerr = np.linalg.norm(normals.astype(np.float64) - rn.astype(np.float64), axis=1) / (NORMAL_ROUNDINGS * U * scale)
        with capsys.disabled():
            print("  %-16s worst normal error / bar = %.3f (%d roundings)" % (name, nerr.max(), NORMAL_ROUNDINGS))
        assert nerr.max() <= 1.0


def test_generic_entry_raises_where_the_standin_raises(dev):
    from permuto_sdf_amd.mesh import marching_tetrahedra
    vol = VOLUMES["sphere64"][0]
    cases = [(vol[0], 0.0), (vol[:1], 0.0), (vol[:, :, :1], 0.0), (vol, float(vol.max())), (vol, float(vol.min())),
             (vol, float(vol.max()) + 1.0), (vol, -1e9), (VOLUMES["nonfinite36"][0], 0.0)]
    for v, level in cases:
        with pytest.raises(ValueError) as a:
            STANDIN.marching_cubes(v, level)
        with pytest.raises(ValueError) as b:
            marching_tetrahedra(torch.from_numpy(np.ascontiguousarray(v)).to(dev), level)
        assert str(a.value) == str(b.value)
    for v, level in ((vol, float(np.nextafter(vol.max(), np.float32(0)))), (vol[:2, :2, :2], float(vol[:2, :2, :2].mean()))):
        STANDIN.marching_cubes(v, level)                        # neither raises just inside the range
        marching_tetrahedra(torch.from_numpy(np.ascontiguousarray(v)).to(dev), level)


def test_two_runs_are_bit_identical(dev):
    from permuto_sdf_amd.mesh import marching_tetrahedra
    for name in ("noise48", "sphere128"):
        v = torch.from_numpy(VOLUMES[name][0]).to(dev)
        a = marching_tetrahedra(v, VOLUMES[name][1], return_edges=True)
        b = marching_tetrahedra(v, VOLUMES[name][1], return_edges=True)
        for x, y in zip(a, b):
            assert torch.equal(x, y)


# ---- the streamed extractor ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fitted(dev):
    from tests.test_gpu_sphere_trace import fit_sphere_sdf
    enc, mlp, win, loss = fit_sphere_sdf(dev)
    assert loss < 1e-4
    return enc, mlp, win


def _tracer_style_gradient(enc, mlp, win, pts):
    """the launches of SphereTracer.trace's analytic normal (permuto_sdf_amd/sphere_trace.py), at pts"""
    import ctypes
    from permuto_sdf_amd import _lib as L
    from permuto_sdf_amd.encoding import _head, _tail, encode_forward_raw
    from permuto_sdf_amd.mlp import _dims_array, mlp_forward_raw, pack_params
    R, dev = pts.shape[0], pts.device
    ws = [l.weight.detach() for l in mlp.layers]
    bs = [l.bias.detach() for l in mlp.layers]
    ws[-1], bs[-1] = ws[-1][0:1].contiguous(), bs[-1][0:1].contiguous()
    dims = list(mlp.dims[:-1]) + [1]
    packed = pack_params(dims, ws, bs)
    feat = encode_forward_raw(enc.cfg, pts, enc.lattice_values.detach(), enc.scale_factor, enc.random_shift_per_level.detach(), win)
    sdf = mlp_forward_raw(dims, feat, packed)
    none = torch.zeros(R, dtype=torch.bool, device=dev)
    d_feat = torch.empty_like(feat)
    gy = torch.ones_like(sdf)
    Wp = (ctypes.c_void_p * len(ws))(*[w.data_ptr() for w in ws])
    Bp = (ctypes.c_void_p * len(bs))(*[b.data_ptr() for b in bs])
    L.call("psdf_mlp_backward_data_masked", L.c_i(len(ws)), _dims_array(dims), L.c_l(R), L.ptr(feat), Wp, Bp, L.ptr(gy),
           L.ptr(none), L.ptr(d_feat), L.stream())
    grads = torch.zeros((R, 3), dtype=torch.float32, device=dev)
    L.call("psdf_encode_backward_positions_masked", *_head(enc.cfg, R), L.ptr(pts), L.ptr(enc.lattice_values.detach()),
           L.ptr(enc.scale_factor), L.ptr(enc.random_shift_per_level.detach()), L.ptr(win), *_tail(enc.cfg), L.ptr(d_feat),
           L.ptr(none), L.ptr(grads), L.stream())
    return sdf.view(-1), grads


def _sdf_on_vertices_bound(enc, mlp, win, mesh, h):
    sdf, grads = _tracer_style_gradient(enc, mlp, win, mesh.V.contiguous())
    worst, bound = float(sdf.abs().max()), h * float(grads.norm(dim=1).max())
    return worst, bound


def test_extractor_equals_the_generic_entry_for_every_slab_size(dev, fitted, capsys):
    from permuto_sdf_amd.mesh import MeshExtractor, marching_tetrahedra
    enc, mlp, win = fitted
    n, lo, hi = 96, -0.5, 0.5
    ex = MeshExtractor(enc, mlp, win)
    first = None
    for slab in (1, 7, n - 1, None):
        m = ex.extract(n, lo, hi, slab_planes=slab, point_budget=200000 if slab == 7 else None, return_edges=True,
                       return_volume=True)
        assert m.nr_evaluated == n ** 3 and m.volume.shape == (n, n, n) and bool(torch.isfinite(m.volume).all())
        verts, faces, _, _, edges = marching_tetrahedra(m.volume, 0.0, normals=False, return_edges=True)
        assert torch.equal(m.edges, edges)                                        # the vertex-edge set, same order
        assert np.array_equal(_rows_sorted(np.sort(m.F.cpu().numpy(), 1)), _rows_sorted(np.sort(faces.cpu().numpy(), 1)))
        assert torch.equal(m.F, faces)                                            # (and the same order of faces)
        assert torch.equal(m.V, verts / (n - 1) * (hi - lo) + lo)                 # bit-equal positions per edge
        if first is None:
            first = m
        else:       # the slab size changes nothing, bit for bit
            assert torch.equal(m.volume, first.volume) and torch.equal(m.V, first.V) and torch.equal(m.F, first.F)
            assert torch.equal(m.NV, first.NV)
    m = first
    assert m.V.shape[0] > 10000 and m.F.shape[0] > 20000
    # the evaluated volume against the public forward at the same points: encode 1e-6 + MLP 4e-6 of the largest |sdf|
    axis = torch.linspace(lo, hi, n, device=dev)
    pts = torch.stack(torch.meshgrid(axis, axis, axis, indexing="ij"), -1).reshape(-1, 3).contiguous()
    with torch.no_grad():
        ref = mlp(enc(pts, win)).view(n, n, n)
    big = float(ref.abs().max())
    err = float((m.volume - ref).abs().max())
    with capsys.disabled():
        print("\n  extractor volume vs module forward: %.2e of the largest |sdf| (bar 5e-6)" % (err / big))
    assert err <= 5e-6 * big
    # vertices lie on the surface of the field, normals are the analytic gradient
    worst, bound = _sdf_on_vertices_bound(enc, mlp, win, m, (hi - lo) / (n - 1))
    assert worst <= bound, (worst, bound)
    _, grads = _tracer_style_gradient(enc, mlp, win, m.V.contiguous())
    want = torch.nn.functional.normalize(grads, dim=1)
    assert float((m.NV.norm(dim=1) - 1).abs().max()) < 1e-5
    with capsys.disabled():
        print("  NV vs tracer-style launches: max |diff| %.1e, bit-equal: %s" % (float((m.NV - want).abs().max()), torch.equal(m.NV, want)))
    assert float((m.NV - want).abs().max()) <= 1e-4
    assert float((m.NV * torch.nn.functional.normalize(m.V, dim=1)).sum(1).median()) > 0.98      # outward
    # from_sdf_net-style construction and the callable form agree on what they were given
    c = MeshExtractor(lambda p: mlp(enc(p.contiguous(), win))).extract(n, lo, hi, return_edges=True)
    assert c.NV is None and c.V.shape[1] == 3 and c.F.shape[0] > 20000


def _shell_grid(dev, n_vox, all_false=False):
    from permuto_sdf import OccupancyGrid
    occ = scene.shell_occupancy(O.Oracle("port"), n_vox, r0=0.3, width=0.05, drop=0.0)
    if all_false:
        occ = np.zeros_like(occ)
    grid = OccupancyGrid(n_vox, 1.0, [0, 0, 0])
    grid.set_grid_occupancy(torch.from_numpy(occ).to(dev))
    return grid


def test_sparse_mode_equals_dense_and_evaluates_a_shell(dev):
    from permuto_sdf_amd.mesh import MeshExtractor
    ex = MeshExtractor(lambda p: p.norm(dim=1, keepdim=True) - 0.3)
    grid = _shell_grid(dev, 64)
    n = 96
    for slab in (None, 5):
        dense = ex.extract(n, -0.5, 0.5, slab_planes=slab, return_edges=True)
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            sparse = ex.extract(n, -0.5, 0.5, slab_planes=slab, occupancy_grid=grid, return_edges=True)
        assert not [w for w in caught if "extracting densely" in str(w.message)]      # h = 1/95 is below the voxel size 1/64
        assert dense.nr_evaluated == n ** 3 and dense.V.shape[0] > 10000
        assert torch.equal(sparse.edges, dense.edges) and torch.equal(sparse.V, dense.V) and torch.equal(sparse.F, dense.F)
        assert 0 < sparse.nr_evaluated < 0.30 * n ** 3, sparse.nr_evaluated / n ** 3
    with pytest.raises(ValueError, match="Surface level must be within volume data range"):
        ex.extract(n, -0.5, 0.5, occupancy_grid=_shell_grid(dev, 64, all_false=True))
    with pytest.warns(UserWarning, match="extracting densely"):      # h = 1/31 exceeds the voxel size 1/64
        coarse = ex.extract(32, -0.5, 0.5, occupancy_grid=grid, return_edges=True)
    dense = ex.extract(32, -0.5, 0.5, return_edges=True)
    assert coarse.nr_evaluated == 32 ** 3 and torch.equal(coarse.V, dense.V) and torch.equal(coarse.F, dense.F)


def test_sparse_mode_of_the_network_equals_dense(dev, fitted):
    """the masked encode + MLP launches: skipped points are never read, the mesh is the dense one"""
    from permuto_sdf_amd.mesh import MeshExtractor
    enc, mlp, win = fitted
    ex = MeshExtractor(enc, mlp, win)
    dense = ex.extract(96, -0.5, 0.5, return_edges=True)
    sparse = ex.extract(96, -0.5, 0.5, occupancy_grid=_shell_grid(dev, 64), return_edges=True, slab_planes=9)
    assert torch.equal(sparse.edges, dense.edges) and torch.equal(sparse.V, dense.V) and torch.equal(sparse.F, dense.F)
    assert torch.equal(sparse.NV, dense.NV) and sparse.nr_evaluated < 0.30 * 96 ** 3


def test_save_ply_writes_the_standins_file(dev, fitted, tmp_path):
    from permuto_sdf_amd.mesh import MeshExtractor
    enc, mlp, win = fitted
    m = MeshExtractor(enc, mlp, win).extract(48, -0.5, 0.5)
    mine, theirs = str(tmp_path / "mine.ply"), str(tmp_path / "theirs.ply")
    m.save_ply(mine)
    c = m.cpu()
    np.savez(str(tmp_path / "mesh.npz"), V=c.V.numpy(), F=c.F.numpy(), NV=c.NV.numpy())
    # compat/easypbr puts the stand-ins of other packages on sys.path when imported: in a process of its own
    code = ("import sys, numpy as np; sys.path.insert(0, %r); import easypbr; d = np.load(%r); m = easypbr.Mesh(); "
            "m.V, m.F, m.NV = d['V'], d['F'], d['NV']; m.save_to_file(%r)"
            % (os.path.join(ROOT, "compat"), str(tmp_path / "mesh.npz"), theirs))
    subprocess.check_call([sys.executable, "-c", code])
    a, b = open(mine, "rb").read(), open(theirs, "rb").read()
    head = a[:a.index(b"end_header\n") + len(b"end_header\n")]
    V, F = c.V.shape[0], c.F.shape[0]
    assert b"element vertex %d\n" % V in head and b"element face %d\n" % F in head and b"property float nz\n" in head
    assert len(a) == len(head) + 24 * V + 13 * F
    first = np.frombuffer(a[len(head):len(head) + 24 * 16], dtype="<f4").reshape(16, 6)
    assert np.array_equal(first[:, :3], c.V.numpy()[:16]) and np.array_equal(first[:, 3:], c.NV.numpy()[:16])
    assert a == b


def test_512_cubed_streams_and_is_watertight(dev, fitted, capsys):
    from permuto_sdf_amd.mesh import MeshExtractor
    enc, mlp, win = fitted
    n = 512
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    m = MeshExtractor(enc, mlp, win).extract(n, -0.5, 0.5)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    resident = n ** 3 * (4 + 4 * enc.cfg.channels)          # the whole volume + the features of all its points
    with capsys.disabled():
        print("\n  512^3: V %d F %d, peak device memory %.0f MiB = %.3f of the resident volume + features"
              % (m.V.shape[0], m.F.shape[0], peak / 2 ** 20, peak / resident))
    assert peak < resident / 4
    V = m.V.shape[0]
    f = m.F.long()
    a = torch.cat([f[:, 0], f[:, 1], f[:, 2]])
    b = torch.cat([f[:, 1], f[:, 2], f[:, 0]])
    und = torch.minimum(a, b) * V + torch.maximum(a, b)
    _, counts = torch.unique(und, return_counts=True)
    assert bool((counts == 2).all()), "not watertight"
    assert torch.unique(a * V + b).numel() == a.numel()          # consistently oriented
    worst, bound = _sdf_on_vertices_bound(enc, mlp, win, m, 1.0 / (n - 1))
    assert worst <= bound, (worst, bound)
    assert float((m.NV.norm(dim=1) - 1).abs().max()) < 1e-5


def test_empty_ranges_and_bad_arguments_of_the_entry_points(dev):
    """N == 0 is OK (no launch, NULL pointers accepted); plane ranges outside the buffer are argument errors, not reads"""
    from permuto_sdf_amd import _lib as L
    lib = L.lib()
    i, f, l = L.c_i, L.c_f, L.c_l
    vol = torch.zeros(4 * 5 * 6, device=dev)
    mask = torch.zeros(4 * 5 * 6, dtype=torch.uint8, device=dev)
    cnt = torch.zeros(4 * 5 * 6, dtype=torch.int32, device=dev)
    dims = (i(4), i(5), i(6), i(0), i(4))
    assert lib.psdf_mesh_classify(None, None, f(0), *dims, i(2), i(2), i(1), i(1), None, None, None, None) == 0
    assert lib.psdf_mesh_emit_vertices(None, f(0), *dims, i(3), i(3), None, None, l(0), None, None, None, None) == 0
    assert lib.psdf_mesh_emit_faces(None, None, f(0), *dims, i(0), i(0), None, None, None, None, None) == 0
    assert lib.psdf_mesh_grid_points(i(4), i(5), i(6), i(0), l(0), l(0), None, None, None, None, None) == 0
    assert lib.psdf_mesh_sparse_mask(l(0), i(64), f(1), (L.c_f * 3)(0, 0, 0), None, None, f(0.01), None, None, None) == 0
    # a buffer of planes 1..2 of 4: vertex plane 2 needs value plane 3, cell plane 2 likewise; cells end at X - 1
    part = (i(4), i(5), i(6), i(1), i(2))
    assert lib.psdf_mesh_classify(L.ptr(vol), None, f(0), *part, i(1), i(3), i(1), i(1), L.ptr(mask), L.ptr(cnt), L.ptr(cnt), None) == -1
    assert lib.psdf_mesh_classify(L.ptr(vol), None, f(0), *part, i(1), i(1), i(1), i(3), L.ptr(mask), L.ptr(cnt), L.ptr(cnt), None) == -1
    assert lib.psdf_mesh_classify(L.ptr(vol), None, f(0), *dims, i(0), i(0), i(0), i(4), L.ptr(mask), L.ptr(cnt), L.ptr(cnt), None) == -1
    assert lib.psdf_mesh_emit_faces(L.ptr(vol), None, f(0), *dims, i(0), i(4), L.ptr(mask), L.ptr(cnt), L.ptr(cnt), L.ptr(cnt), None) == -1
    assert lib.psdf_mesh_classify(L.ptr(vol), None, f(0), i(4), i(5), i(6), i(2), i(3), i(2), i(3), i(2), i(2), L.ptr(mask),
                                  L.ptr(cnt), L.ptr(cnt), None) == -1                     # xbase + nplanes > X
    nrm = torch.zeros(8, 3, device=dev)                                                  # volume normals need the whole volume
    assert lib.psdf_mesh_emit_vertices(L.ptr(vol), f(0), *part, i(1), i(2), L.ptr(mask), L.ptr(cnt), l(0), L.ptr(nrm), None,
                                       L.ptr(nrm), None) == -2
    torch.cuda.synchronize()
