"""The host side of the mesh evaluation (permuto_sdf_amd/mesh_eval.py, csrc/mesh_eval.hip), checked without a GPU.

  * the yardstick of the GPU tests, tests/mesh_eval_reference.py, equals sklearn.neighbors.NearestNeighbors -- the library the
    DTU protocol itself uses -- on 3 000 points: radius_neighbors feeds the same sequential loop, kneighbors gives the distances;
  * tests/host/mesh_eval_plan_check.cpp, a stand-alone program that includes nothing but csrc/mesh_eval_plan.h, reproduces
    hand-derived grids under the address and undefined-behaviour sanitizers;
  * tests/host/mesh_eval_kernels_check.cpp runs the kernels' own source on CPU threads (tests/host/hip_on_host) under the same
    sanitizers, against brute-force float64;
  * the plan header is host-only, and the host-only entries of the library agree with it."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import mesh_eval_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "permuto_sdf_amd", "csrc")


def noisy_sphere(seed, n):
    r = np.random.default_rng(seed)
    v = r.standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return (v * 0.4 + r.standard_normal((n, 3)) * 0.002).astype(np.float32)


@pytest.mark.parametrize("seed, radius", [(0, 0.02), (2, 0.05)])
def test_reference_thinning_is_the_protocols_loop_over_sklearn_neighbours(seed, radius):
    skln = pytest.importorskip("sklearn.neighbors")
    p = noisy_sphere(seed, 3000)
    order = np.random.default_rng(seed + 100).permutation(len(p))
    # sklearn's neighbour lists of the unshuffled cloud drive the helper's own formulation of the walk (eval.py:85-93 walks the
    # shuffled copy; visiting row order[k] of the original k-th is the same walk)
    cloud = p.astype(np.float64)
    lists = skln.NearestNeighbors(radius=radius, algorithm="kd_tree").fit(cloud).radius_neighbors(cloud, return_distance=False)
    want = np.ones(len(p), dtype=bool)
    for cur in order:
        if want[cur]:
            want[lists[cur]] = False
            want[cur] = True
    assert 100 < want.sum() < len(p)
    assert np.array_equal(ref.radius_thin(p, radius, order), want)
    pytest.importorskip("scipy.spatial")
    assert np.array_equal(ref.radius_thin(p, radius, order, tree=True), want)


def test_reference_nearest_is_sklearns_kneighbors():
    skln = pytest.importorskip("sklearn.neighbors")
    r, q = noisy_sphere(5, 3000).astype(np.float64) * 500, noisy_sphere(6, 3000).astype(np.float64) * 500 + 0.3
    d_sk, i_sk = skln.NearestNeighbors(n_neighbors=1, algorithm="kd_tree").fit(r).kneighbors(q, n_neighbors=1, return_distance=True)
    d, i = ref.nearest(q, r)
    assert np.array_equal(i, i_sk[:, 0])
    assert np.abs(d - d_sk[:, 0]).max() <= 4 * 2.0 ** -53 * d.max()
    pytest.importorskip("scipy.spatial")
    d_t, i_t = ref.nearest(q, r, tree=True)
    assert np.array_equal(i_t, i) and np.array_equal(d_t, d)
    assert ref.nearest(q[:3], r[:0])[1].tolist() == [-1, -1, -1]


def test_reference_sampling_counts_and_order_on_triangles_done_by_hand():
    # right isosceles, legs 3.5 x density: n1 = n2 = 3, lattice (i + 1/2) / 3; kept iff i + j + 1 < 3 or, on the knife edge
    # i + j + 1 = 3, whatever float64 makes of a_i + b_j < 1
    d = 0.25
    V = np.array([[0, 0, 0], [3.5 * d, 0, 0], [0, 3.5 * d, 0], [1, 1, 1]], dtype=np.float32)
    F = np.array([[0, 1, 2], [0, 0, 1], [3, 3, 3]])
    cloud, counts, margin = ref.sample_surface(V, F, d)
    a = (np.arange(4) + 0.5) / 3.0
    want = [(i, j) for i in range(4) for j in range(4) if a[i] + a[j] < 1]
    assert counts.tolist() == [len(want), 0, 0] and 3 <= len(want) <= 6 and margin[0] > 0.1
    assert np.array_equal(cloud[:4], V.astype(np.float64))
    assert np.allclose(cloud[4:], [[a[i] * 3.5 * d, a[j] * 3.5 * d, 0] for i, j in want], rtol=0, atol=1e-15)
    # smaller than the density: n1 = n2 = 0, the one candidate sits at 1/2 x 10^7 and is rejected
    small = np.array([[0, 0, 0], [0.1 * d, 0, 0], [0, 0.1 * d, 0]], dtype=np.float32)
    assert ref.sample_surface(small, np.array([[0, 1, 2]]), d)[1].tolist() == [0]


def test_plan_arithmetic_stand_alone_under_sanitizers(tmp_path):
    cxx = next((c for c in ("/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++", shutil.which("clang++"),
                            shutil.which("g++")) if c and os.path.exists(c)), None)
    if cxx is None:
        pytest.skip("neither ROCm's clang++ nor g++ is installed")
    exe = str(tmp_path / "mesh_eval_plan_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "host", "mesh_eval_plan_check.cpp"), "-o", exe]
    if not cxx.endswith("clang++"):     # clang links the sanitizer runtimes into the program by default, g++ on request
        cmd[1:1] = ["-static-libasan", "-static-libubsan"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, " ".join(cmd) + "\n" + r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr


def test_kernel_source_on_cpu_threads_under_sanitizers(tmp_path):
    """csrc/mesh_eval.hip itself, compiled as C++ against tests/host/hip_on_host (a stand-in for the HIP runtime header that runs
    a launch on CPU threads), driven like mesh_eval.py drives it and compared with brute-force float64 by
    tests/host/mesh_eval_kernels_check.cpp: a stand-alone program with its own main, under ASan and UBSan"""
    cxx = next((c for c in ("/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++", shutil.which("clang++"),
                            shutil.which("g++")) if c and os.path.exists(c)), None)
    if cxx is None:
        pytest.skip("neither ROCm's clang++ nor g++ is installed")
    exe = str(tmp_path / "mesh_eval_kernels_check")
    cmd = [cxx, "-x", "c++", "-std=c++20", "-O1", "-g", "-ffp-contract=off", "-Wno-unused-function", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "tests", "host", "hip_on_host"), "-I", CSRC,
           os.path.join(ROOT, "tests", "host", "mesh_eval_kernels_check.cpp"), "-o", exe, "-lpthread"]
    if not cxx.endswith("clang++"):
        cmd[1:1] = ["-static-libasan", "-static-libubsan"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, " ".join(cmd) + "\n" + r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr


def test_mesh_eval_plan_h_is_host_only():
    src = open(os.path.join(CSRC, "mesh_eval_plan.h")).read()
    assert set(re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", src)) <= {"cmath", "cstdint", "cstdlib"}
    assert not re.search(r"\bhip[A-Z_]|__device__|__global__|__host__", src)
    hip = open(os.path.join(CSRC, "mesh_eval.hip")).read()
    assert '#include "mesh_eval_plan.h"' in hip
    # the tile capacity and the grid arithmetic did not stay behind as copies
    assert "TILE_CAPACITY =" not in hip and "COARSEN" not in hip


def test_thinning_grid_is_planned_with_the_radius_the_sweeps_compare_against(lib):
    """psdf_mesh_thin_sweep refuses a grid whose edge is below fp32(radius) x (1 + 1/512) (csrc/mesh_eval.hip); radius_thin rounds
    the radius once (mesh_eval.fp32) and plans with that value, so a radius that decides the edge is always accepted -- planning
    with the unrounded double would be refused for the radii whose fp32 value lies above it"""
    from permuto_sdf_amd import mesh_eval as me
    margin = 1 + 1 / 512
    oe, dims, cells = (ctypes.c_float * 4)(), (ctypes.c_int * 3)(), ctypes.c_int64(0)
    d3 = lambda *v: (ctypes.c_double * 3)(*v)    # noqa: E731

    def edge(min_edge):          # a unit box with 3 x 10^6 points: the radius decides the edge
        assert lib.psdf_mesh_eval_grid_plan(d3(0, 0, 0), d3(1, 1, 1), ctypes.c_int64(3000000), ctypes.c_double(min_edge),
                                            ctypes.c_int64(0), oe, dims, ctypes.byref(cells), None) == 0
        return float(oe[3])

    radii = [0.008, 0.004, 0.016, 0.064, 0.02, 0.05, 0.2] + np.random.default_rng(0).uniform(0.01, 2.0, 2000).tolist()
    unrounded_refused = 0
    for r in radii:
        r32 = me.fp32(r)
        assert r32 == float(np.float32(r))
        assert edge(r32) >= r32 * margin, r
        unrounded_refused += edge(r) < r32 * margin
    assert unrounded_refused > 100 and edge(0.008) < me.fp32(0.008) * margin


@pytest.fixture(scope="module")
def lib():
    from permuto_sdf_amd import build
    return ctypes.CDLL(build.build(verbose=False))


def test_library_exports_the_mesh_eval_entries_and_its_plan_is_the_headers(lib):
    header = open(os.path.join(ROOT, "include", "psdf.h")).read()
    names = sorted(set(re.findall(r"\b(psdf_mesh_(?:eval|sample|thin|nn)_[a-z0-9_]+)\s*\(", header)))
    assert len(names) == 9, names
    assert not [n for n in names if not hasattr(lib, n)]
    src = open(os.path.join(CSRC, "mesh_eval_plan.h")).read()
    assert lib.psdf_mesh_eval_tile_capacity() == int(re.search(r"TILE_CAPACITY = (\d+);", src).group(1))
    # the plans mesh_eval_plan_check.cpp derives by hand, through the entry Python calls
    oe, dims = (ctypes.c_float * 4)(), (ctypes.c_int * 3)()
    cells, blocks = ctypes.c_int64(-1), ctypes.c_int64(-1)
    d3 = lambda *v: (ctypes.c_double * 3)(*v)    # noqa: E731

    def plan(lo, hi, n, min_edge, budget):
        return lib.psdf_mesh_eval_grid_plan(d3(*lo), d3(*hi), ctypes.c_int64(n), ctypes.c_double(min_edge), ctypes.c_int64(budget),
                                            oe, dims, ctypes.byref(cells), ctypes.byref(blocks))

    assert plan((0, 0, 0), (100, 100, 100), 960000, 0.0, 1000000) == 0
    assert (oe[3], list(dims), cells.value, blocks.value) == (1.220703125, [82, 82, 82], 551368, 9261)
    assert plan((1, 2, 3), (1, 2, 3), 5, 0.25, 0) == 0 and (list(oe), list(dims), cells.value) == ([1, 2, 3, 0.25048828125], [1, 1, 1], 1)
    assert plan((0, 0, 0), (1, 1, 1), 2 ** 31 - 1, 0.0, 0) == 0
    assert plan((0, 0, 0), (1, 1, 1), 2 ** 31, 0.0, 0) == -2
    assert plan((0, 0, 0), (1, 1, 1), 0, 0.0, 0) == -1
    assert plan((0, 0, 0), (float("nan"), 1, 1), 4, 0.0, 0) == -1


def test_empty_batches_return_before_any_pointer_check_and_bad_arguments_are_refused(lib):
    z, one, st = ctypes.c_int64(0), ctypes.c_int64(1), None
    dens, f0 = ctypes.c_double(0.2), ctypes.c_float(1.0)
    assert lib.psdf_mesh_sample_count(None, z, None, z, dens, None, None, st) == 0
    assert lib.psdf_mesh_sample_emit(None, z, None, z, dens, None, None, st) == 0
    assert lib.psdf_mesh_eval_cell_keys(None, z, None, None, 0, None, st) == 0
    assert lib.psdf_mesh_thin_sweep(None, None, None, z, None, None, None, f0, None, None, st) == 0
    assert lib.psdf_mesh_nn_cooperative(None, z, None, None, z, None, None, None, f0, None, None, None, None, st) == 0
    assert lib.psdf_mesh_nn_ring(None, z, None, z, None, None, None, f0, None, None, None, st) == 0
    # argument errors, before any launch
    p = ctypes.c_void_p(4096)
    assert lib.psdf_mesh_sample_count(p, one, p, one, ctypes.c_double(0.0), p, p, st) == -1
    assert lib.psdf_mesh_sample_count(None, one, p, one, dens, p, p, st) == -1
    assert lib.psdf_mesh_eval_cell_keys(p, ctypes.c_int64(-1), None, None, 0, p, st) == -1
    oe, dims = (ctypes.c_float * 4)(0, 0, 0, 1.0), (ctypes.c_int * 3)(4, 4, 4)
    assert lib.psdf_mesh_eval_cell_keys(p, one, oe, (ctypes.c_int * 3)(4, 0, 4), 0, p, st) == -1
    assert lib.psdf_mesh_eval_cell_keys(p, one, (ctypes.c_float * 4)(0, 0, 0, 0.0), dims, 0, p, st) == -1
    assert lib.psdf_mesh_eval_cell_keys(p, ctypes.c_int64(2 ** 31), oe, dims, 0, p, st) == -2
    # a thinning grid whose cells are narrower than the radius would miss neighbours: refused
    assert lib.psdf_mesh_thin_sweep(p, p, p, one, p, oe, dims, ctypes.c_float(1.0), p, p, st) == -1
    assert lib.psdf_mesh_nn_cooperative(p, one, p, p, one, p, oe, dims, ctypes.c_float(-1.0), p, p, p, p, st) == -1
    assert lib.psdf_mesh_nn_ring(p, one, p, one, p, oe, dims, ctypes.c_float(float("nan")), p, p, p, st) == -1
