"""The host side of coloured meshes (permuto_sdf_amd/mesh_color.py, csrc/mesh_color.hip, csrc/mesh_color_plan.h), checked
without a GPU.

  * csrc/mesh_color_plan.h is host-only arithmetic with a sanitized stand-alone check; mesh_color.hip itself is compiled against
    tests/host/hip_on_host and both kernels run under the address and undefined-behaviour sanitizers against float64;
  * the SH evaluator has one home, csrc/sh_device.h, which sampling.hip and mesh_color.hip include;
  * the library exports exactly the three names the header declares; empty inputs and bad arguments return their codes with no GPU;
  * `ExtractedMesh.save_ply` writes colours after the normals, and a mesh without colours is written byte for byte as before
    (the two cases without colours are regression checks: they pass on the commit before colours too, against bytes built here
    from the documented layout);
  * `MeshColorizer.colors` refuses bad arguments before it touches a device."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests.test_nerf_host import _cxx, _sanitized

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "permuto_sdf_amd", "csrc")
NAMES = ["psdf_mesh_color_finish", "psdf_mesh_color_inputs", "psdf_mesh_color_plan"]


# ------------------------------------------------------------------------------------------------------- the native side
def test_plan_header_under_sanitizers(tmp_path):
    """csrc/mesh_color_plan.h alone, as plain C++17: tests/host/mesh_color_plan_check.cpp, a program with its own main"""
    _sanitized(tmp_path, "mesh_color_plan_check.cpp", "c++17", [])


def test_both_kernels_source_on_the_cpu_under_sanitizers(tmp_path):
    """csrc/mesh_color.hip itself, compiled as C++ against tests/host/hip_on_host: both kernels run in buffers of exactly the
    declared extents and are compared with float64 entry by entry; tests/host/mesh_color_kernels_check.cpp, a stand-alone program
    with its own main, under ASan and UBSan"""
    if _cxx() is not None and not _cxx().endswith("clang++"):
        pytest.skip("the stand-in header is written for clang")
    _sanitized(tmp_path, "mesh_color_kernels_check.cpp", "c++20", ["-I", os.path.join(ROOT, "tests", "host", "hip_on_host")])


def _code(name):
    src = open(os.path.join(CSRC, name)).read()
    return src, re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))


def test_plan_header_is_host_only_and_the_kernels_are_plain():
    src, _ = _code("mesh_color_plan.h")
    assert set(re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", src)) <= {"cstdint"}
    assert not re.search(r"\bhip[A-Z_]|__device__|__global__|__host__", src)
    hip, code = _code("mesh_color.hip")
    for header in ("mesh_color_plan.h", "composite_device.h", "sh_device.h"):
        assert '#include "%s"' % header in hip, header
    for word in ("atomic", "asm", "__shared__", "__shfl", "__syncthreads", "hipMalloc", "Synchronize", "hipMemcpy"):
        assert word not in code, word
    # the expressions whose bits other entries hold
    assert "1.0f / (1.0f + expf(-" in code and "normalize_eps(" in code and "sh_eval(" in code and "rintf(" in code


def test_the_sh_evaluator_has_one_home():
    _, header = _code("sh_device.h")
    assert header.count("0.28209479177387814f") == 1 and header.count("o[48] =") == 1
    for name in os.listdir(CSRC):
        if name.endswith((".hip", ".h")) and name != "sh_device.h":
            _, code = _code(name)
            assert "0.48860251190291987f" not in code, name
    _, sampling = _code("sampling.hip")
    assert '#include "sh_device.h"' in sampling and "sh_eval(degree, x, y, z, out + (int64_t)i * channels)" in sampling


@pytest.fixture(scope="module")
def lib():
    from permuto_sdf_amd import build
    return ctypes.CDLL(build.build(verbose=False))


def test_library_exports_exactly_the_declared_mesh_color_entries(lib):
    header = open(os.path.join(ROOT, "include", "psdf.h")).read()
    start = header.index("/* ---- mesh_color.hip ---- */")
    end = header.find("/* ---- ", start + 10)
    section = header[start:end if end > 0 else len(header)]
    assert sorted(set(re.findall(r"\bint (psdf_[a-z0-9_]+)\s*\(", section))) == NAMES
    assert not [n for n in NAMES if not hasattr(lib, n)]
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    if os.path.exists(nm):
        out = subprocess.run([nm, "-D", "--defined-only", lib._name], capture_output=True, text=True).stdout
        assert sorted(set(re.findall(r"\b(psdf_mesh_color[a-z0-9_]*)\b", out))) == NAMES
    from permuto_sdf_amd import mesh_color
    plan = open(os.path.join(CSRC, "mesh_color_plan.h")).read()
    assert mesh_color._PLAN_FIELDS == int(re.search(r"FIELDS = (\d+);", plan).group(1))
    assert mesh_color._PLAN_FIELDS == int(re.search(r"#define PSDF_MESH_COLOR_PLAN_FIELDS (\d+)", header).group(1))
    assert (mesh_color.MODE_NORMAL, mesh_color.MODE_CAMERA) == tuple(
        int(v) for v in re.search(r"MODE_NORMAL = (\d+), MODE_CAMERA = (\d+);", plan).groups())


def test_empty_inputs_return_before_any_pointer_check_and_bad_arguments_are_refused(lib):
    i64, st = ctypes.c_int64, None
    p = ctypes.c_void_p(4096)          # never read: every call below returns before a launch
    assert lib.psdf_mesh_color_inputs(i64(0), None, None, None, -4, 99, None, None, -1, -1, None, None, st) == 0
    assert lib.psdf_mesh_color_finish(i64(0), None, None, None, st) == 0

    def inputs(n=1, pts=p, grad=p, y=p, g=32, mode=0, eye=p, x=p, C=111, sh=51):
        return lib.psdf_mesh_color_inputs(i64(n), pts, grad, y, g, mode, eye, x, C, sh, None, None, st)

    assert inputs(n=-1) == -1 and inputs(g=-1, C=78) == -1 and inputs(mode=2) == -1 and inputs(mode=-1) == -1 and inputs(sh=-1) == -1
    assert inputs(C=110) == -1 and inputs(C=112) == -1 and inputs(sh=52) == -1 and inputs(g=31) == -1
    assert inputs(grad=None) == -1 and inputs(y=None) == -1 and inputs(x=None) == -1
    assert inputs(mode=1, pts=None) == -1 and inputs(mode=1, eye=None) == -1
    assert inputs(n=2 ** 31) == -2 and inputs(C=2 ** 16 + 1, sh=2 ** 16 + 1 - 60) == -2
    assert lib.psdf_mesh_color_finish(i64(-1), p, p, p, st) == -1 and lib.psdf_mesh_color_finish(i64(1), None, p, p, st) == -1
    assert lib.psdf_mesh_color_finish(i64(2 ** 31), p, p, p, st) == -2
    assert lib.psdf_mesh_color_finish(i64(1), p, None, None, st) == 0          # nothing asked for: no launch

    out = (i64 * 7)()
    assert lib.psdf_mesh_color_plan(51, 32, 111, i64(2 ** 31 + 5), i64(1 << 18), out) == 0
    assert list(out) == [51, 76, 79, 111, 111, 8193, 5]
    assert lib.psdf_mesh_color_plan(51, 32, 111, i64(0), i64(7), out) == 0 and list(out)[5:] == [0, 0]
    assert lib.psdf_mesh_color_plan(51, 32, 111, i64(5), i64(7), None) == -1
    assert lib.psdf_mesh_color_plan(52, 32, 111, i64(5), i64(7), out) == -1 and lib.psdf_mesh_color_plan(51, 32, 111, i64(5), i64(0), out) == -1
    assert lib.psdf_mesh_color_plan(51, 32, 111, i64(-1), i64(7), out) == -1 and lib.psdf_mesh_color_plan(0, 32, 60, i64(5), i64(7), out) == -1
    assert lib.psdf_mesh_color_plan(51, 32, 111, i64(5), i64(2 ** 31), out) == -2


# ------------------------------------------------------------------------------------------------------- the file format
def _tetrahedron():
    V = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.25, -0.5, 1.0]])
    F = torch.tensor([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], dtype=torch.int32)
    NV = torch.nn.functional.normalize(V - V.mean(0), dim=1)
    C = torch.tensor([[0, 1, 2], [255, 128, 127], [17, 254, 3], [200, 100, 50]], dtype=torch.uint8)
    return V, F, NV, C


def _documented_bytes(V, F, NV, C):
    """the file as the layout says it: an ASCII header, then per vertex three (six with normals) little-endian floats and, with
    colours, three bytes; per face one byte 3 and three little-endian int32"""
    import struct
    props = ["x", "y", "z"] + (["nx", "ny", "nz"] if NV is not None else [])
    head = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % len(V)
    head += "".join("property float %s\n" % p for p in props)
    if C is not None:
        head += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    head += "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % len(F)
    body = b""
    for i in range(len(V)):
        body += struct.pack("<3f", *V[i].tolist())
        if NV is not None:
            body += struct.pack("<3f", *NV[i].tolist())
        if C is not None:
            body += struct.pack("<3B", *C[i].tolist())
    for f in F.tolist():
        body += struct.pack("<B3i", 3, *f)
    return head.encode("ascii") + body


@pytest.mark.parametrize("with_normals", [False, True])
@pytest.mark.parametrize("with_colours", [False, True])
def test_save_ply_layout_and_byte_count(tmp_path, with_normals, with_colours):
    from permuto_sdf_amd.mesh import ExtractedMesh
    V, F, NV, C = _tetrahedron()
    NV, C = (NV if with_normals else None), (C if with_colours else None)
    mesh = ExtractedMesh(V, F, NV, C=C) if with_colours else ExtractedMesh(V, F, NV)      # (without C: the parent's call)
    path = str(tmp_path / "mesh.ply")
    mesh.save_ply(path)
    data = open(path, "rb").read()
    want = _documented_bytes(V, F, NV, C)
    assert data == want
    header, body = data[:data.index(b"end_header\n") + 11], data[data.index(b"end_header\n") + 11:]
    per_vertex = 12 + (12 if with_normals else 0) + (3 if with_colours else 0)
    assert per_vertex == {(False, False): 12, (True, False): 24, (False, True): 15, (True, True): 27}[(with_normals, with_colours)]
    assert len(body) == 4 * per_vertex + 4 * 13
    text = header.decode("ascii")
    assert ("property uchar red\nproperty uchar green\nproperty uchar blue\nelement face 4\n" in text) == with_colours
    assert ("property float nz\n" in text) == with_normals
    if with_colours:        # after the normals, before the faces
        assert text.index("property uchar red") > text.index("property float nz" if with_normals else "property float z")
    # reading it back with numpy
    fields = [("v", "<f4", (3,))] + ([("n", "<f4", (3,))] if with_normals else []) + ([("c", "u1", (3,))] if with_colours else [])
    rec = np.frombuffer(body[:4 * per_vertex], dtype=fields)
    assert rec.dtype.itemsize == per_vertex and np.array_equal(rec["v"], V.numpy())
    if with_normals:
        assert np.array_equal(rec["n"], NV.numpy())
    if with_colours:
        assert np.array_equal(rec["c"], C.numpy())
    faces = np.frombuffer(body[4 * per_vertex:], dtype=[("k", "u1"), ("i", "<i4", (3,))])
    assert np.array_equal(faces["i"], F.numpy()) and (faces["k"] == 3).all()


def test_colours_of_another_length_or_of_an_empty_mesh_are_not_written(tmp_path):
    from permuto_sdf_amd.mesh import ExtractedMesh
    V, F, NV, C = _tetrahedron()
    path = str(tmp_path / "mesh.ply")
    ExtractedMesh(V, F, NV, C=C[:3]).save_ply(path)
    assert open(path, "rb").read() == _documented_bytes(V, F, NV, None)
    empty = ExtractedMesh(V[:0], F[:0], NV[:0], C=C[:0])
    empty.save_ply(path)
    assert open(path, "rb").read() == _documented_bytes(V[:0], F[:0], None, None)
    carried = ExtractedMesh(V, F, NV, C=C).cpu()
    assert carried.C is not None and torch.equal(carried.C, C) and ExtractedMesh(V, F).C is None


# ------------------------------------------------------------------------------------------------------- the Python layer
def test_colorizer_refuses_bad_arguments_before_it_touches_a_device():
    import permuto_sdf_amd
    from permuto_sdf_amd import mesh_color
    from permuto_sdf_amd._lib import PsdfError
    assert permuto_sdf_amd.MeshColorizer is mesh_color.MeshColorizer and "MeshColorizer" in permuto_sdf_amd.__all__
    assert "VertexColors" in permuto_sdf_amd.__all__ and mesh_color.VertexColors._fields == ("rgb", "rgb_u8", "normals")
    dev = torch.device("cpu")
    assert mesh_color._view("normal", dev) == (0, None)
    mode, eye = mesh_color._view([1, 2.5, -3], dev)
    assert mode == 1 and eye.dtype == torch.float32 and eye.tolist() == [1.0, 2.5, -3.0]
    from permuto_sdf_amd.render import Frame
    tf = torch.eye(4)
    tf[:3, 3] = torch.tensor([0.5, -0.25, 2.0])
    mode, eye = mesh_color._view(Frame(torch.eye(3), tf, 4, 4), dev)
    assert mode == 1 and eye.tolist() == [0.5, -0.25, 2.0]
    for bad in ("camera", "", [1.0, 2.0], torch.zeros(4), torch.zeros(2, 3), None, object()):
        with pytest.raises(ValueError):
            mesh_color._view(bad, dev)
    from permuto_sdf_amd.train_step import HyperParams, RgbNet, SdfNet
    hp = HyperParams()
    colorizer = mesh_color.MeshColorizer(SdfNet(hp), RgbNet(hp))
    assert colorizer.it == mesh_color._IT_WINDOW_OPEN
    with pytest.raises(PsdfError):                # CPU tensors: there is no CPU path
        colorizer.colors(torch.zeros(5, 3))
    with pytest.raises(ValueError):
        mesh_color.ColorPlan(51, 32, 111, 10, 0)
    with pytest.raises(ValueError):
        mesh_color.ColorPlan(52, 32, 111, 10, 4)
    plan = mesh_color.ColorPlan(51, 32, 111, 600, 256)
    assert (plan.c_enc, plan.c_sh, plan.c_normal, plan.c_geom, plan.C, plan.nr_chunks, plan.last_chunk) == (51, 76, 79, 111, 111, 3, 88)
