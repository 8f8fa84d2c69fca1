"""The host side of the SDF cross-sections (permuto_sdf_amd/sdf_slice.py, csrc/sdf_slice.hip, csrc/sdf_slice_plan.h), checked
without a GPU.

  * tests/host/sdf_slice_kernels_check.cpp runs the kernels' own source on the CPU (tests/host/hip_on_host) under the address
    and undefined-behaviour sanitizers: the layer's points bit for bit against a scalar restatement of the reference's lines, the
    band decisions exactly, the colours and the cut against float64 at derived bars, canaries around every output (the program
    states the cases and the bars);
  * the header lists exactly the new entries with what they replace and the library exports them; empty ranges and bad
    arguments return their codes with no GPU;
  * `IsoStyle`'s band table is the float64 formula rounded to float32; the module refuses CPU tensors and a time that does not
    fit the field; the kernel file stays compilable on the host."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests.test_frame_host import CSRC, ROOT, _build_and_run

ENTRIES = ["psdf_slice_colorize", "psdf_slice_cut_begin", "psdf_slice_cut_resolve", "psdf_slice_points"]


def test_kernel_source_on_the_cpu_under_sanitizers(tmp_path):
    out = _build_and_run(tmp_path, "sdf_slice_kernels_check",
                         ["-x", "c++", "-std=c++20", "-ffp-contract=off", "-Wno-unused-function", "-I",
                          os.path.join(ROOT, "tests", "host", "hip_on_host")])
    print(out)
    for S, cells in ((1, "[0, 1)"), (2, "[0, 4)"), (37, "[0, 1369)"), (37, "[5, 1367)")):
        for P in (3, 4):
            assert re.search(r"points\s+S =\s+%d, cells %s, rows of %d" % (S, re.escape(cells), P), out), (S, cells, P)
    for label in ("defaults", "overlapping", "32 lines"):
        assert re.search(r"%s\s+colorize .* 1 NaN, 6 skipped, bounds: ok" % label, out), label
    # the cut: the cap on the float64 geometry alone, and every kind of ray
    m = re.search(r"float64 geometry: (\d+) of 2173 rays unchecked \(cap 21\), (\d+) grazing, (\d+) behind the camera, (\d+) miss the "
                  r"box, (\d+) slice over sphere, (\d+) sphere over slice, (\d+) slice on no surface", out)
    unchecked, *kinds = (int(v) for v in m.groups())
    assert unchecked <= 21 and all(k >= 10 for k in kinds), m.groups()
    assert "pixels [1024, 2048)" in out and "pixels [2048, 2173)" in out
    worst = [float(v) for v in re.search(r"worst error / bar: colour ([\d.]+), cut point ([\d.]+), cut t ([\d.]+)", out).groups()]
    assert all(0.0 < w <= 1.0 for w in worst), worst


def test_the_kernel_file_stays_compilable_on_the_host():
    src = open(os.path.join(CSRC, "sdf_slice.hip")).read()
    assert not re.search(r"__shfl|__ballot|__shared__|atomic|__builtin_amdgcn", src)
    assert '#include "sdf_slice_plan.h"' in src
    plan = open(os.path.join(CSRC, "sdf_slice_plan.h")).read()
    assert set(re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", plan)) <= {"cmath", "cstdint"}
    assert not re.search(r"\bhip[A-Z_]|__device__|__global__|__host__", plan)
    from permuto_sdf_amd import build
    assert "-ffp-contract=off" in build.FLAGS and "sdf_slice.hip" not in build.EXTRA


@pytest.fixture(scope="module")
def lib():
    from permuto_sdf_amd import build
    return ctypes.CDLL(build.build(verbose=False))


def test_header_lists_the_entries_and_the_library_exports_them(lib):
    header = open(os.path.join(ROOT, "include", "psdf.h")).read()
    assert sorted(set(re.findall(r"\b(psdf_slice_[a-z0-9_]+)\s*\(", header))) == ENTRIES
    assert not [n for n in ENTRIES if not hasattr(lib, n)]
    section = header[header.index("/* ---- sdf_slice.hip ---- */"):]
    section = section[:section.index("/* ---- ", 10)]
    assert sorted(re.findall(r"\bint (psdf_[a-z0-9_]+)\(", section)) == ENTRIES
    for name, cites in (("psdf_slice_points", ("visualize_sdf_isolines.py:69-92, 96-101", "aabb.py:28-42", "render_from_frame.py:71-166")),
                        ("psdf_slice_colorize", ("visualize_sdf_isolines.py:111-138", "common_utils.py:150-154", "NGPGui.cxx:22-25")),
                        ("psdf_slice_cut_begin", ("visualize_sdf_isolines.py:158-162",)),
                        ("psdf_slice_cut_resolve", ("visualize_sdf_isolines.py:158-162", ":111-138"))):
        comment = header[:header.index("int " + name + "(")].rsplit("/*", 1)[1]
        assert "replaces:" in comment, name
        for c in cites:
            assert c in re.sub(r"\s+", " ", comment), (name, c)
        assert "void* stream);" in header[header.index("int " + name + "("):].split(";")[0] + ";"
    assert "unpinned" in section


def test_empty_ranges_and_bad_arguments_without_a_gpu(lib):
    st, f, z = None, ctypes.c_float, ctypes.c_int64(0)
    p = ctypes.c_void_p(4096)          # (never read: every call below returns before a launch)
    tri, axes, base = (f * 3)(0.5, 0.5, 0.5), (f * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1), (f * 4)(0.0, 0.3, 0.2, 8 / 3)
    bands = (f * 99)()

    def points(S=37, first=5, count=100, stride=3, time=None, pts=p, ax=axes):
        return lib.psdf_slice_points(S, ctypes.c_int64(first), count, stride, ax, f(0.1), f(1.0), tri, tri, time, pts, p, st)

    def colorize(S=37, first=5, count=100, K=9, lines=15, lo=bands, table=p, sdf=p):
        return lib.psdf_slice_colorize(S, ctypes.c_int64(first), count, sdf, p, table, K, base, lines, lo, bands, bands, p, p, p, st)

    def begin(R=100, stride=3, time=None, H=41, W=53, first=37, t=p):
        return lib.psdf_slice_cut_begin(R, stride, axes, f(0.1), f(1.0), tri, tri, p, p, time, H, W, ctypes.c_int64(first), p, p, p, p, t, st)

    def resolve(R=100, K=9, lines=15, H=41, W=53, first=37, mask=p):
        return lib.psdf_slice_cut_resolve(R, p, p, p, p, K, base, lines, bands, bands, bands, H, W, ctypes.c_int64(first), p, p, p, mask, st)

    # a count of 0 returns 0 before anything is looked at
    assert lib.psdf_slice_points(0, z, 0, 7, None, f(0), f(1), None, None, None, None, None, st) == 0
    assert lib.psdf_slice_colorize(0, z, 0, None, None, None, 0, None, 99, None, None, None, None, None, None, st) == 0
    assert lib.psdf_slice_cut_begin(0, 7, None, f(0), f(1), None, None, None, None, None, 0, 0, z, None, None, None, None, None, st) == 0
    assert lib.psdf_slice_cut_resolve(0, None, None, None, None, 0, None, 99, None, None, None, 0, 0, z, None, None, None, None, st) == 0
    # points
    assert points(count=-1) == -1 and points(stride=5) == -1 and points(stride=2) == -1 and points(stride=4, time=None) == -1
    assert points(first=-1) == -1 and points(first=37 * 37 - 99) == -1 and points(S=0) == -1
    assert points(pts=None) == -1 and points(ax=None) == -1
    assert points(S=46341) == -2 and points(S=65536) == -2          # S S >= 2^31
    # colorize
    assert colorize(lines=33) == -1 and colorize(lines=-1) == -1 and colorize(K=1) == -1 and colorize(K=65537) == -1
    assert colorize(lo=None) == -1 and colorize(table=None) == -1 and colorize(sdf=None) == -1
    assert colorize(first=37 * 37 - 99) == -1 and colorize(count=-3) == -1
    assert colorize(S=46341) == -2
    # the cut
    assert begin(R=-1) == -1 and begin(stride=7) == -1 and begin(stride=4) == -1 and begin(H=0) == -1
    assert begin(first=-1) == -1 and begin(first=41 * 53 - 99) == -1 and begin(t=None) == -1
    assert begin(H=65536, W=32768) == -2
    assert resolve(R=-1) == -1 and resolve(lines=33) == -1 and resolve(K=1) == -1 and resolve(first=41 * 53 - 99) == -1
    assert resolve(mask=None) == -1
    assert resolve(H=65536, W=32768) == -2


def test_band_table_is_the_float64_formula_rounded_to_float32():
    from permuto_sdf_amd.sdf_slice import MAX_LINES, PUBU, IsoStyle, table_lookup64
    style = IsoStyle()
    assert (style.width, style.distance, style.nr_lines) == (0.005, 0.03, 15)                  # NGPGui.cxx:22-25
    assert style.base_map == (0.0, 0.3, 0.2, 1.0) and style.line_map == (0.0, 0.2, 0.3, 1.0)   # visualize_sdf_isolines.py:120, 135
    assert style.table == PUBU and len(PUBU) == 9 and PUBU[0] == (1.0, 247 / 255, 251 / 255) and PUBU[8] == (2 / 255, 56 / 255, 88 / 255)
    for style in (style, IsoStyle(width=0.05, distance=0.017, nr_lines=32), IsoStyle(nr_lines=0)):
        lo, hi, rgb = style.band_table()
        assert lo.dtype == hi.dtype == rgb.dtype == np.float32 and rgb.shape == (style.nr_lines, 3)
        tab = np.asarray(style.table, np.float32).astype(np.float64)
        for i in range(style.nr_lines):
            centre = i * style.distance                                                        # visualize_sdf_isolines.py:125-127
            assert lo[i] == np.float32(centre - style.width / 2) and hi[i] == np.float32(centre + style.width / 2)
            t = 0.3 + ((1.0 - 0.3) / (0.2 - 0.0)) * (min(max(centre, 0.0), 0.2) - 0.0)          # map_range_np, common_utils.py:162-166
            u = t * 8
            j = min(int(u), 7)
            want = tab[j] + (u - j) * (tab[j + 1] - tab[j])
            assert np.array_equal(rgb[i], want.astype(np.float32)), i
    # the first line is the table at 0.3, the lines from 0.2 on its last control point
    lo, hi, rgb = IsoStyle().band_table()
    assert np.array_equal(rgb[7], np.asarray(PUBU[8], np.float32)) and np.array_equal(rgb[14], rgb[7])
    assert np.allclose(rgb[0], table_lookup64(np.asarray(PUBU), 0.3), atol=1e-7)
    assert np.array_equal(IsoStyle().base_map32(), np.asarray([0.0, 0.3, 0.2, 0.8 / 0.3], np.float64).astype(np.float32))
    for bad in (dict(nr_lines=MAX_LINES + 1), dict(nr_lines=-1), dict(table=((0.0, 0.0, 0.0),)), dict(table=((0.0, 1.0), (1.0, 0.0))),
                dict(base_map=(0.3, 0.3, 0.0, 1.0))):
        with pytest.raises(ValueError):
            IsoStyle(**bad)
    assert hash(IsoStyle()) == hash(IsoStyle())          # the device copy of a style's table is kept per style


def test_module_refuses_cpu_tensors_and_a_time_that_does_not_fit_the_field():
    import permuto_sdf_amd
    from permuto_sdf_amd import FusedMLP, PermutoEncoding, box_trace, render, sdf_slice
    from permuto_sdf_amd._lib import PsdfError
    assert permuto_sdf_amd.sdf_slice is sdf_slice and "sdf_slice" in permuto_sdf_amd.__all__
    for name in ("SlicePlane", "IsoStyle", "PUBU", "SliceImage", "SlicedFrame", "render_slice", "cut_slice_into"):
        assert getattr(permuto_sdf_amd, name) is getattr(sdf_slice, name) and name in permuto_sdf_amd.__all__
    box = box_trace.Box([1.0, 1.0, 1.0])
    frame = render.Frame(torch.eye(3), torch.eye(4), 41, 53)
    plane = sdf_slice.SlicePlane.from_frame(frame, -0.057)
    assert np.array_equal(plane.axes, np.eye(3, dtype=np.float32)) and plane.z == -0.057 and plane.extent_scale == 1.0
    rot = torch.tensor([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    tf = torch.eye(4)
    tf[:3, :3] = rot
    assert np.array_equal(sdf_slice.SlicePlane.from_frame(render.Frame(torch.eye(3), tf, 4, 4), 0.0).axes, rot.numpy())   # the columns
    for bad in (dict(axes=np.eye(4), z=0.0), dict(axes=np.eye(3), z=0.0, extent_scale=0.0)):
        with pytest.raises(ValueError):
            sdf_slice.SlicePlane(**bad)
    planes = torch.zeros(3, 41, 53), torch.zeros(1, 41, 53), torch.zeros(1, 41, 53)
    for P in (3, 4):
        enc = PermutoEncoding(P, 2 ** 10, 4, 2, np.geomspace(1.0, 0.1, 4), concat_points=True, concat_points_scaling=1.0)
        mlp = FusedMLP([enc.output_dims(), 32, 32, 32, 1])
        net = type("Net", (), {"encoding": enc, "mlp_sdf": mlp, "window": staticmethod(lambda it: torch.ones(4))})
        wrong, right = (None, 0.5) if P == 4 else (0.5, None)
        with pytest.raises(ValueError):
            sdf_slice.render_slice(net, plane, box, 16, time_val=wrong)
        with pytest.raises(ValueError):
            sdf_slice.cut_slice_into(net, plane, box, frame, *planes, time_val=wrong)
        with pytest.raises(PsdfError):
            sdf_slice.render_slice(net, plane, box, 16, time_val=right)
        with pytest.raises(PsdfError):
            sdf_slice.cut_slice_into(net, plane, box, frame, *planes, time_val=right)
        for bad in (dict(size=0), dict(size=16, max_points_per_chunk=0)):
            with pytest.raises(ValueError):
                sdf_slice.render_slice(net, plane, box, time_val=right, **bad)
        with pytest.raises(PsdfError):
            sdf_slice.render_slice(net, plane, box, 46341, time_val=right)      # S S >= 2^31: refused before anything is allocated
    # the conveniences exist, and the existing signatures keep their defaults
    import inspect
    from permuto_sdf_amd import sdf_fit
    assert callable(sdf_fit.SdfFitter.slice) and callable(render.FrameRenderer.slice) and callable(render.FrameRenderer.box)
    sig = inspect.signature(sdf_fit.SdfFitter.render)
    assert list(sig.parameters)[:4] == ["self", "frame", "t", "box"] and sig.parameters["slice"].default is None
