"""The host side of grid-free sphere tracing in a box (permuto_sdf_amd/box_trace.py, csrc/box_trace.hip), checked without a GPU.

  * tests/host/box_trace_kernels_check.cpp runs the kernels' own source on the CPU (tests/host/hip_on_host) under the address
    and undefined-behaviour sanitizers: the intersection bit for bit against a scalar restatement of the reference's aabb.py,
    begin and step for rows of 3 and of 4 floats, the planes against float64 at derived bars, R in {0, 1, 255, 257} with canaries
    around every output (the program states the cases and the bars);
  * the header lists the entries with what they replace and the library exports them; empty batches and bad arguments return
    their codes with no GPU;
  * `Box` computes its bounds in float32 in the reference's order; the module refuses CPU tensors and a time that does not fit
    the field."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests.test_frame_host import CSRC, ROOT, _build_and_run

ENTRIES = ["psdf_box_ray_intersection", "psdf_box_trace_begin", "psdf_box_trace_resolve", "psdf_box_trace_step"]


def test_kernel_source_on_the_cpu_under_sanitizers(tmp_path):
    out = _build_and_run(tmp_path, "box_trace_kernels_check",
                         ["-x", "c++", "-std=c++20", "-ffp-contract=off", "-Wno-unused-function", "-I",
                          os.path.join(ROOT, "tests", "host", "hip_on_host")])
    print(out)
    for R in (0, 1, 255, 257):
        assert re.search(r"intersection\s+R =\s+%d:" % R, out) and re.search(r"resolve\s+R =\s+%d, rows of 4" % R, out), R
        assert re.search(r"begin \+ step\s+R =\s+%d, rows of 3" % R, out) and re.search(r"begin \+ step\s+R =\s+%d, rows of 4" % R, out), R
    assert "face test" in out and "0.6 x 0.65 x 0.5 box" in out
    worst = [float(v) for v in re.search(r"worst error / bar: normals ([\d.]+), camera normals ([\d.]+), depth ([\d.]+)", out).groups()]
    assert all(0.0 < w <= 1.0 for w in worst), worst


def test_the_kernel_file_stays_compilable_on_the_host():
    src, shared = (open(os.path.join(CSRC, f)).read() for f in ("box_trace.hip", "frame_device.h"))
    for text in (src, shared):
        assert not re.search(r"__shfl|__ballot|wave_sum|wave_incl|__builtin_amdgcn|__shared__|atomic", text)
    # the surface pixel, with its normalize_eps, is the shared header's
    assert '#include "frame_device.h"' in src and "surface_hit(" in src and "st_surface(" in src and "box_inside(" in src
    assert '#include "composite_device.h"' in shared and "normalize_eps" in shared


@pytest.fixture(scope="module")
def lib():
    from permuto_sdf_amd import build
    return ctypes.CDLL(build.build(verbose=False))


def test_header_lists_the_entries_and_the_library_exports_them(lib):
    header = open(os.path.join(ROOT, "include", "psdf.h")).read()
    assert sorted(set(re.findall(r"\b(psdf_box_[a-z0-9_]+)\s*\(", header))) == ENTRIES
    assert not [n for n in ENTRIES if not hasattr(lib, n)]
    for name, cites in (("psdf_box_ray_intersection", "aabb.py:47-100"), ("psdf_box_trace_begin", "sdf_utils.py:122"),
                        ("psdf_box_trace_step", "aabb.py:28-42"), ("psdf_box_trace_resolve", "sdf_utils.py:221-231")):
        comment = header[:header.index("int " + name + "(")].rsplit("/*", 1)[1]
        assert "replaces:" in comment and cites in comment, name
        assert "void* stream);" in header[header.index("int " + name + "("):].split(";")[0] + ";"
    # the position backward with the caller's scratch, which makes a captured trace's normals the eager trace's
    for name in ("psdf_encode_backward_positions_masked_ws", "psdf_encode_backward_positions_workspace_bytes"):
        assert name + "(" in header and hasattr(lib, name)


def test_empty_batches_and_bad_arguments_without_a_gpu(lib):
    st, f = None, ctypes.c_float
    z, p = ctypes.c_int64(0), ctypes.c_void_p(4096)          # (never read: every call below returns before a launch)
    box = (f * 3)(0.5, 0.5, 0.5)
    assert lib.psdf_box_ray_intersection(0, None, None, None, None, None, None, None, None, None, st) == 0
    assert lib.psdf_box_trace_begin(0, 3, None, None, None, None, None, None, None, None, st) == 0
    assert lib.psdf_box_trace_step(0, 4, None, None, None, None, f(0.9), f(1e-3), None, None, st) == 0
    assert lib.psdf_box_trace_resolve(0, 3, None, None, None, None, None, None, f(0.01), None, 0, 0, z, None, None, None, None, st) == 0
    assert lib.psdf_box_ray_intersection(-1, box, box, p, p, p, p, p, p, p, st) == -1
    assert lib.psdf_box_ray_intersection(5, box, None, p, p, p, p, p, p, p, st) == -1
    assert lib.psdf_box_trace_begin(5, 4, box, box, p, p, None, p, p, p, st) == -1          # rows of 4 floats need the time
    assert lib.psdf_box_trace_begin(5, 2, box, box, p, p, p, p, p, p, st) == -1
    assert lib.psdf_box_trace_begin(-5, 3, box, box, p, p, p, p, p, p, st) == -1
    assert lib.psdf_box_trace_step(5, 3, box, box, p, None, f(0.9), f(1e-3), p, p, st) == -1
    assert lib.psdf_box_trace_step(5, 7, box, box, p, p, f(0.9), f(1e-3), p, p, st) == -1

    def resolve(R=10, P=4, g=p, cam=None, rot=None, H=41, W=53, first=37, img=p):
        return lib.psdf_box_trace_resolve(R, P, p, p, p, p, g, p, f(0.01), rot, H, W, ctypes.c_int64(first), img, cam, p, p, st)

    assert resolve(R=-1) == -1 and resolve(P=5) == -1 and resolve(g=None) == -1 and resolve(img=None) == -1
    assert resolve(cam=p) == -1 and resolve(H=0) == -1 and resolve(first=-1) == -1 and resolve(first=41 * 53 - 9) == -1
    assert resolve(H=65536, W=32768) == -2
    # the scratch of the position backward: none for one group of levels, groups * N * P floats otherwise; host only
    nbytes = lib.psdf_encode_backward_positions_workspace_bytes
    nbytes.restype = ctypes.c_int64
    assert nbytes(3, 2, ctypes.c_int64(1000), 6, 1) == 0                               # 6 + 2 levels: one group of 8
    assert nbytes(4, 2, ctypes.c_int64(1000), 24, 1) == 4 * 1000 * 4 * 4               # 24 + 2 levels in groups of 8
    assert nbytes(3, 2, ctypes.c_int64(1 << 17), 24, 1) == 13 * (1 << 17) * 3 * 4      # groups of 2 from 2^17 points on
    assert nbytes(3, 2, ctypes.c_int64(0), 24, 1) == 0
    assert lib.psdf_encode_backward_positions_masked_ws(4, 2, ctypes.c_int64(0), 24, 1 << 18, None, None, None, None, None, 1, f(1.0),
                                                        None, None, None, None, z, st) == 0
    assert lib.psdf_encode_backward_positions_masked_ws(4, 2, ctypes.c_int64(1000), 24, 1 << 18, p, p, p, p, p, 1, f(1.0), p, p, p,
                                                        None, z, st) == -1           # the scratch is missing


def test_box_bounds_in_float32_in_the_references_order():
    from permuto_sdf_amd.box_trace import Box
    sizes, trans = [0.6, 0.65, 0.5], [0.1, -0.05, 0.2]
    box = Box(sizes, trans)
    s, t = torch.as_tensor(sizes), torch.as_tensor(trans)                        # aabb.py:48-49, on torch's float32
    assert np.array_equal(box.bb_min, (-s / 2 + t).numpy()) and np.array_equal(box.bb_max, (s - s / 2 + t).numpy())
    assert box.bb_min.dtype == np.float32 and np.array_equal(box.half, torch.tensor([x / 2 for x in sizes]).numpy())
    unit = Box([1.0, 1.0, 1.0])
    assert list(unit.bb_min) == [-0.5] * 3 and list(unit.bb_max) == [0.5] * 3 and list(unit.half) == [0.5] * 3
    # the inside test is strict, about the translation (aabb.py:28-42); plain torch, any device
    pts = torch.tensor([[0.0, 0.0, 0.0], [0.5, 0.0, 0.0], [0.49999997, 0.0, 0.0], [0.0, -0.5, 0.0], [0.0, 0.0, 0.6]])
    assert unit.check_point_inside_primitive(pts).view(-1).tolist() == [True, False, True, False, False]
    assert box.check_point_inside_primitive(torch.tensor([[0.1, -0.05, 0.2, 0.7], [0.1, -0.05, 0.46, 0.7]])).view(-1).tolist() == [True, False]
    r = box.rand_points_inside(2000, generator=torch.Generator().manual_seed(1))
    assert tuple(r.shape) == (2000, 3) and bool(box.check_point_inside_primitive(r).float().mean() > 0.99)
    assert bool((r.min(0).values < torch.tensor(box.bb_min) + 0.02).all()) and bool((r.max(0).values > torch.tensor(box.bb_max) - 0.02).all())
    for bad in (([1.0, 1.0], [0, 0, 0]), ([1.0, 0.0, 1.0], [0, 0, 0]), ([1.0, 1.0, 1.0], [0, 0])):
        with pytest.raises(ValueError):
            Box(*bad)


def test_module_refuses_cpu_tensors_and_a_time_that_does_not_fit_the_field():
    import permuto_sdf_amd
    from permuto_sdf_amd import FusedMLP, PermutoEncoding, box_trace, render
    from permuto_sdf_amd._lib import PsdfError
    assert permuto_sdf_amd.box_trace is box_trace and "box_trace" in permuto_sdf_amd.__all__
    for name in ("Box", "BoxTracer", "BoxPlayer", "BoxTracedFrame", "render_box_traced"):
        assert getattr(permuto_sdf_amd, name) is getattr(box_trace, name) and name in permuto_sdf_amd.__all__
    box = box_trace.Box([1.0, 1.0, 1.0])
    o, d = torch.zeros(5, 3), torch.ones(5, 3)
    with pytest.raises(PsdfError):
        box.ray_intersection(o, d)
    for P in (3, 4):
        enc = PermutoEncoding(P, 2 ** 10, 4, 2, np.geomspace(1.0, 0.1, 4), concat_points=True, concat_points_scaling=1.0)
        tracer = box_trace.BoxTracer(enc, FusedMLP([enc.output_dims(), 32, 32, 32, 1]), box)
        assert tracer.pos_dim == P and hasattr(tracer, "_sdf")
        with pytest.raises(ValueError):
            tracer.trace(o, d, time_val=None if P == 4 else 0.5)
        with pytest.raises(PsdfError):
            tracer.trace(o, d, time_val=0.5 if P == 4 else None)
        with pytest.raises(PsdfError):
            tracer.capture(o, d, time_val=0.5 if P == 4 else None)
    frame = render.Frame(torch.eye(3), torch.eye(4), 41, 53)
    net = type("Net", (), {"encoding": enc, "mlp_sdf": tracer.mlp, "window": staticmethod(lambda it: torch.ones(4))})
    with pytest.raises(PsdfError):
        box_trace.render_box_traced(net, box, frame, time_val=0.5)
    with pytest.raises(PsdfError):
        box_trace.BoxPlayer(net, box, frame)
    # SdfFitter's conveniences exist and SdfFitNet's docstring no longer says a 4-D net can only be cut
    from permuto_sdf_amd import sdf_fit
    assert callable(sdf_fit.SdfFitter.tracer) and callable(sdf_fit.SdfFitter.render)
    assert "BoxTracer" in sdf_fit.SdfFitNet.__doc__
