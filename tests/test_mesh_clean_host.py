"""The host side of the mesh cleaning (permuto_sdf_amd/mesh_clean.py, csrc/mesh_clean.hip), checked without a GPU.

  * the yardstick of the GPU tests, tests/mesh_clean_reference.py, is pinned to scipy: its dilation equals
    scipy.ndimage.binary_dilation with the structure built from the spans, its "edge" components equal
    scipy.sparse.csgraph.connected_components over the edges that occur exactly twice; the ellipse tables for 3, 5 and 7 equal
    matrices written by hand (OpenCV and trimesh themselves are not available: both rules stay unpinned);
  * tests/host/mesh_clean_plan_check.cpp, a stand-alone program that includes nothing but csrc/mesh_clean_plan.h, reproduces
    hand-derived plans under the address and undefined-behaviour sanitizers;
  * tests/host/mesh_clean_kernels_check.cpp runs the kernels' own source on CPU threads (tests/host/hip_on_host, concurrent mode)
    under the same sanitizers and a time limit, against brute force;
  * the plan header is host-only, and the library exports the entries include/psdf.h declares."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import mesh_clean_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "permuto_sdf_amd", "csrc")
KERNELS_CHECK_SECONDS = 600      # a union-find that does not terminate fails here, not on a device


def test_ellipse_tables_done_by_hand():
    from permuto_sdf_amd import mesh_clean as mc
    for fn in (ref.ellipse_half_widths, mc.ellipse_half_widths):
        assert fn(1) == [0]
        assert fn(3) == [0, 1, 0]
        assert fn(5) == [0, 2, 2, 2, 0]
        assert fn(7) == [0, 2, 3, 3, 3, 2, 0]
        assert fn(101)[:8] == [0, 10, 14, 17, 20, 22, 24, 26] and fn(101)[50] == 50 and fn(101) == fn(101)[::-1]
    assert all(ref.ellipse_half_widths(k) == mc.ellipse_half_widths(k) for k in range(1, 140))
    cross = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], dtype=bool)
    five = np.array([[0, 0, 1, 0, 0], [1, 1, 1, 1, 1], [1, 1, 1, 1, 1], [1, 1, 1, 1, 1], [0, 0, 1, 0, 0]], dtype=bool)
    seven = np.array([[0, 0, 0, 1, 0, 0, 0], [0, 1, 1, 1, 1, 1, 0], [1, 1, 1, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1, 1],
                      [0, 1, 1, 1, 1, 1, 0], [0, 0, 0, 1, 0, 0, 0]], dtype=bool)
    for k, want in ((3, cross), (5, five), (7, seven)):
        assert np.array_equal(ref.element_matrix(ref.ellipse_half_widths(k)), want)


@pytest.mark.parametrize("half_widths", [[0], [0, 1, 0], ref.ellipse_half_widths(21), ref.ellipse_half_widths(101), [9, 0, 3]],
                         ids=["1", "3", "21", "101", "asymmetric"])
def test_reference_dilation_is_scipys_binary_dilation(half_widths):
    ndi = pytest.importorskip("scipy.ndimage")
    r = np.random.default_rng(3)
    masks = r.random((2, 60, 90)) < 0.004
    masks[:, 0, 0] = masks[:, 0, -1] = masks[:, -1, 0] = masks[:, -1, -1] = True
    masks[0, 30, :] |= r.random(90) < 0.1
    got = ref.dilate(masks, half_widths)
    # scipy dilates by the Minkowski sum, cv.dilate by the reflected element: the same for the ellipses, rows reversed otherwise
    structure = ref.element_matrix(half_widths)[::-1]
    for m, g in zip(masks, got):
        assert np.array_equal(g, ndi.binary_dilation(m, structure=structure, border_value=0))
    assert got.any() and (len(half_widths) == 101 or not got.all())     # (the 101-row ellipse covers an image this small)


def test_reference_packing_round_trip_and_padding():
    bits = np.random.default_rng(0).random((2, 3, 70)) < 0.5
    words = ref.pack(bits)
    assert words.shape == (2, 3, 3) and words.dtype == np.int32
    back = ((words.view(np.uint32)[..., None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(2, 3, 96).astype(bool)
    assert np.array_equal(back[:, :, :70], bits) and not back[:, :, 70:].any()


def _soup(seed, nV, nF):
    return np.random.default_rng(seed).integers(0, nV, (nF, 3)).astype(np.int32)


def _strip(n, seed=None):
    order = np.arange(n) if seed is None else np.random.default_rng(seed).permutation(n)
    return np.stack([order, order + 1, order + 2], 1).astype(np.int32)


@pytest.mark.parametrize("F, nV", [(_soup(0, 300, 500), 300), (_soup(1, 2000, 1500), 2000), (_strip(3000, 2), 3002),
                                   (np.array([[0, 1, 2], [2, 3, 4]]), 5), (np.array([[0, 1, 2], [0, 1, 3], [1, 0, 4]]), 5),
                                   (np.array([[0, 1, 2], [0, 1, 2]]), 3), (np.array([[0, 0, 1], [0, 1, 2], [1, 2, 3]]), 4)],
                         ids=["soup300", "soup2000", "strip", "bow-tie", "three-on-an-edge", "identical", "equal-indices"])
def test_reference_edge_components_are_scipys_connected_components(F, nV):
    sparse = pytest.importorskip("scipy.sparse")
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    nF = len(F)
    # the edges that occur exactly twice, counted independently of the yardstick: a dictionary of half-edges
    users = {}
    for f, (a, b, c) in enumerate(F.tolist()):
        for u, v in ((a, b), (b, c), (c, a)):
            users.setdefault((min(u, v), max(u, v)), []).append(f)
    pairs = [fs for (u, v), fs in users.items() if len(fs) == 2 and u != v]
    rows, cols = [p[0] for p in pairs], [p[1] for p in pairs]
    graph = sparse.coo_matrix((np.ones(len(pairs)), (rows, cols)), shape=(nF, nF))
    count, comp = csgraph.connected_components(graph, directed=False)
    labels, sizes = ref.face_components(F, nV, "edge")
    assert (sizes > 0).sum() == count
    first = np.full(count, nF)
    np.minimum.at(first, comp, np.arange(nF))
    assert np.array_equal(labels, first[comp])
    assert np.array_equal(sizes, np.bincount(labels, minlength=nF))


def test_reference_vertex_components_and_largest_component_by_hand():
    F = np.array([[0, 1, 2], [2, 3, 4], [5, 6, 7], [6, 7, 8], [7, 8, 9]])
    V = np.arange(30, dtype=np.float32).reshape(10, 3)
    labels, sizes = ref.face_components(F, 10, "vertex")
    assert labels.tolist() == [0, 0, 2, 2, 2] and sizes.tolist() == [2, 0, 3, 0, 0]
    labels, sizes = ref.face_components(F, 10, "edge")
    assert labels.tolist() == [0, 1, 2, 2, 2] and sizes.tolist() == [1, 1, 3, 0, 0]
    Vl, Fl = ref.largest_component(V, F)
    assert np.array_equal(Vl, V[5:]) and Fl.tolist() == [[0, 1, 2], [1, 2, 3], [2, 3, 4]]
    # a tie: the component with the smaller label
    Vt, Ft = ref.largest_component(V, F[:2], "edge")
    assert np.array_equal(Vt, V[:3]) and Ft.tolist() == [[0, 1, 2]]


def test_reference_vertex_test_rules_by_hand():
    # one view, an identity-like camera: u = x / z, v = y / z
    P = np.array([[[1.0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]])
    dilated = np.zeros((1, 4, 6), dtype=bool)
    dilated[0, 2, 3] = True
    V = np.array([[3, 2, 1], [2.5, 2, 1], [3.5, 2, 1], [2, 2, 1], [-0.5, 0, 1], [-0.51, 0, 1], [5.5, 3.5, 1], [5.51, 0, 1], [0, 4, 1],
                  [3, 2, 0], [np.nan, 0, 1], [1e30, 1e30, 1e-30], [-6, -4, -2], [0, 0, 1]], dtype=np.float32)
    # the set bit; 2.5 -> 2 and 3.5 -> 4 (half to even): clear; column 2: clear; -0.5 -> -0 is column 0: clear; -0.51 -> -1: outside;
    # (5.5, 3.5) -> (6, 4): outside; 5.51 -> 6: outside; row 4: outside
    want = [True, False, False, False, False, True, True, True, True,
            True, True, True, True, False]    # p2 == 0; NaN; far outside; behind the camera, onto the set bit; pixel (0, 0): clear
    assert ref.inside_masks(V, P, dilated).tolist() == want
    assert ref.inside_masks(V, P[:, :3], dilated).tolist() == want


def _compiler():
    return next((c for c in ("/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++", shutil.which("clang++"),
                             shutil.which("g++")) if c and os.path.exists(c)), None)


def test_plan_arithmetic_stand_alone_under_sanitizers(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("neither ROCm's clang++ nor g++ is installed")
    exe = str(tmp_path / "mesh_clean_plan_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "host", "mesh_clean_plan_check.cpp"), "-o", exe]
    if not cxx.endswith("clang++"):     # clang links the sanitizer runtimes into the program by default, g++ on request
        cmd[1:1] = ["-static-libasan", "-static-libubsan"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, " ".join(cmd) + "\n" + r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr


def test_kernel_source_on_cpu_threads_under_sanitizers(tmp_path):
    """csrc/mesh_clean.hip itself, compiled as C++ against tests/host/hip_on_host in concurrent mode (the kernels ballot, and the
    union-find is raced by 256 threads), driven like mesh_clean.py drives it and compared with brute force by
    tests/host/mesh_clean_kernels_check.cpp: a stand-alone program with its own main, under ASan and UBSan and a time limit"""
    cxx = _compiler()
    if cxx is None:
        pytest.skip("neither ROCm's clang++ nor g++ is installed")
    exe = str(tmp_path / "mesh_clean_kernels_check")
    cmd = [cxx, "-x", "c++", "-std=c++20", "-O1", "-g", "-ffp-contract=off", "-Wno-unused-function", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "tests", "host", "hip_on_host"), "-I", CSRC,
           os.path.join(ROOT, "tests", "host", "mesh_clean_kernels_check.cpp"), "-o", exe, "-lpthread"]
    if not cxx.endswith("clang++"):
        cmd[1:1] = ["-static-libasan", "-static-libubsan"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, " ".join(cmd) + "\n" + r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=KERNELS_CHECK_SECONDS)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr


def test_mesh_clean_plan_h_is_host_only():
    src = open(os.path.join(CSRC, "mesh_clean_plan.h")).read()
    assert set(re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", src)) <= {"cmath", "cstdint", "cstdlib"}
    assert not re.search(r"\bhip[A-Z_]|__device__|__global__|__host__", src)
    hip = open(os.path.join(CSRC, "mesh_clean.hip")).read()
    assert '#include "mesh_clean_plan.h"' in hip
    # the budget and the caps did not stay behind as copies
    assert "LDS_BYTES =" not in hip and "MAX_HALF_WIDTH =" not in hip


@pytest.fixture(scope="module")
def lib():
    from permuto_sdf_amd import build
    return ctypes.CDLL(build.build(verbose=False))


def test_library_exports_the_mesh_clean_entries_and_its_plan_is_the_headers(lib):
    header = open(os.path.join(ROOT, "include", "psdf.h")).read()
    assert "/* ---- mesh_clean.hip ---- */" in header
    names = sorted(set(re.findall(r"\b(psdf_mesh_clean_[a-z0-9_]+)\s*\(", header)))
    assert len(names) == 13, names
    assert not [n for n in names if not hasattr(lib, n)]
    out = (ctypes.c_int64 * 9)()
    hw = (ctypes.c_int * 101)(*ref.ellipse_half_widths(101))
    i64 = ctypes.c_int64
    # the plans mesh_clean_plan_check.cpp derives by hand, through the entry Python calls
    assert lib.psdf_mesh_clean_dilate_plan(i64(64), i64(1200), i64(1600), hw, i64(101), out) == 0
    assert list(out) == [50, 156, 256, 7, 8, 50, 3584, 19200, 65536 + 384]
    assert lib.psdf_mesh_clean_dilate_plan(i64(3), i64(150), i64(200), hw, i64(101), out) == 0
    assert list(out)[:8] == [50, 150, 250, 1, 1, 7, 3, 113]
    assert lib.psdf_mesh_clean_dilate_plan(i64(1), i64(0), i64(200), hw, i64(101), out) == -1
    assert lib.psdf_mesh_clean_dilate_plan(i64(1), i64(5), i64(5), hw, i64(100), out) == -1
    hw[3] = 255
    assert lib.psdf_mesh_clean_dilate_plan(i64(1), i64(5), i64(5), hw, i64(101), out) == -1
    lib.psdf_mesh_clean_union_find_cap.restype = ctypes.c_int64
    assert lib.psdf_mesh_clean_union_find_cap(i64(20000)) == 20001


def test_empty_batches_return_before_any_pointer_check_and_bad_arguments_are_refused(lib):
    z, one, st = ctypes.c_int64(0), ctypes.c_int64(1), None
    assert lib.psdf_mesh_clean_row_distance(None, z, 0, 0, 128, None, st) == 0
    assert lib.psdf_mesh_clean_dilate(None, z, 0, 0, None, 0, None, st) == 0
    assert lib.psdf_mesh_clean_inside_masks(None, z, None, 3, None, 0, 0, None, st) == 0
    assert lib.psdf_mesh_clean_face_keep(None, z, None, z, None, None, None, st) == 0
    assert lib.psdf_mesh_clean_emit_vertices(z, None, None, None, None, None, None, None, None, None, st) == 0
    assert lib.psdf_mesh_clean_emit_faces(None, z, None, None, None, None, st) == 0
    assert lib.psdf_mesh_clean_edge_keys(None, z, z, None, None, st) == 0
    assert lib.psdf_mesh_clean_link_edges(None, None, z, None, None, st) == 0
    assert lib.psdf_mesh_clean_link_vertices(None, z, z, None, None, st) == 0
    assert lib.psdf_mesh_clean_flatten(None, z, None, None, None, st) == 0
    assert lib.psdf_mesh_clean_face_labels(None, z, z, None, None, None, None, st) == 0
    # argument errors, before any launch
    p = ctypes.c_void_p(4096)
    hw = (ctypes.c_int * 3)(0, 1, 0)
    assert lib.psdf_mesh_clean_row_distance(p, one, 0, 5, 128, p, st) == -1
    assert lib.psdf_mesh_clean_row_distance(p, one, 5, 5, 256, p, st) == -1
    assert lib.psdf_mesh_clean_row_distance(None, one, 5, 5, 128, p, st) == -1
    assert lib.psdf_mesh_clean_dilate(p, one, 5, 5, hw, 2, p, st) == -1
    assert lib.psdf_mesh_clean_dilate(p, one, 5, 0, hw, 3, p, st) == -1
    assert lib.psdf_mesh_clean_dilate(p, one, 5, 5, (ctypes.c_int * 3)(0, 255, 0), 3, p, st) == -1
    assert lib.psdf_mesh_clean_dilate(p, one, 5, 5, (ctypes.c_int * 257)(), 257, p, st) == -2
    assert lib.psdf_mesh_clean_dilate(p, one, 5, 5, hw, 3, None, st) == -1
    assert lib.psdf_mesh_clean_inside_masks(p, ctypes.c_int64(-1), p, 1, p, 5, 5, p, st) == -1
    assert lib.psdf_mesh_clean_inside_masks(p, one, None, 1, p, 5, 5, p, st) == -1
    assert lib.psdf_mesh_clean_inside_masks(p, ctypes.c_int64(2 ** 31), p, 1, p, 5, 5, p, st) == -2
    assert lib.psdf_mesh_clean_face_keep(p, one, p, one, None, p, None, st) == -1
    assert lib.psdf_mesh_clean_edge_keys(p, ctypes.c_int64(2 ** 30), one, p, p, st) == -2
    assert lib.psdf_mesh_clean_flatten(p, one, p, None, None, st) == -1
