"""What the writers of image planes share lives in ONE place per side: permuto_sdf_amd/csrc/frame_device.h on the device (the
three-channel store, the camera-frame normal, the depth along a ray, the surface pixel, the box test), csrc/frame_plan.h for the
range check of a chunk, permuto_sdf_amd/frame.py in Python (the camera, its rays and chunks, the open lattice window, the device
check, the planes, the pool swap, the stacking of views).  These tests read the sources with the comments stripped: an expression
of one of them that turns up in a second file, or a helper called without its header, is a copy coming back.  No GPU, no library."""
import ast
import os
import re

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "permuto_sdf_amd")
CSRC = os.path.join(PKG, "csrc")
SOURCES = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".h"))}
CODE = {f: re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S)) for f, src in SOURCES.items()}
HOME, PLAN = "frame_device.h", "frame_plan.h"
WRITERS = ("frame_composite.hip", "frame_trace.hip", "box_trace.hip", "sdf_slice.hip", "frame_rays.hip")
HELPERS = ("st_planes", "camera_normal", "ray_depth", "surface_hit", "st_surface", "box_inside", "triple")
PYTHON = {f: open(os.path.join(PKG, f)).read() for f in sorted(os.listdir(PKG)) if f.endswith(".py")}


def _includes(f, seen=None):
    """every csrc file that f includes, directly or through another"""
    seen = set() if seen is None else seen
    for inc in re.findall(r'#include\s+"([^"]+)"', SOURCES[f]):
        if inc in SOURCES and inc not in seen:
            seen.add(inc)
            _includes(inc, seen)
    return seen


def _files_with(pattern):
    return [f for f, src in CODE.items() if re.search(pattern, src)]


def test_each_shared_definition_is_in_the_header_and_nowhere_else():
    for name in ("st_planes", "box_inside", "camera_normal", "ray_depth", "surface_hit", "st_surface"):
        assert _files_with(r"__forceinline__\s+[\w:]+\s+%s\s*\(" % name) == [HOME], name
    for name in ("Triple", "SurfacePixel"):
        assert _files_with(r"\bstruct\s+%s\b" % name) == [HOME], name
    assert _files_with(r"\bTriple\s+triple\s*\(") == [HOME]


def test_the_rotation_and_the_depth_are_written_once():
    assert _files_with(r"rot\[0\]\s*\*") == [HOME]
    assert [f for f, src in CODE.items() if "(q.x * d.x + q.y * d.y) + q.z * d.z" in src] == [HOME]
    # sdf_slice.hip's own dot products have another grouping and stay its own
    assert len(re.findall(r"\bdot3\s*\(", CODE["sdf_slice.hip"])) >= 2


def test_one_range_check():
    assert _files_with(r"[<>]=?\s*(\w+::)*MAX_PIXELS\b") == [PLAN]
    assert "MAX_CELLS" not in CODE["sdf_slice_plan.h"] and "MAX_CELLS" not in CODE["sdf_slice.hip"]
    assert not [f for f, src in CODE.items() if f.endswith(".hip") and re.search(r"\bint\s+check_range\s*\(", src)]
    assert _files_with(r"\bint\s+check_range\s*\(") == [PLAN]
    for f in WRITERS:
        assert re.search(r"\w*plan::check_range\s*\(", CODE[f]), f
    # where a plan's refusal is returned as an entry's status, an assertion says that the numbers agree
    assert re.search(r"static_assert\s*\([^;]*PLAN_ERR_ARG\s*==\s*PSDF_ERR_ARG[^;]*PLAN_ERR_UNSUPPORTED\s*==\s*PSDF_ERR_UNSUPPORTED", CODE[HOME])


def test_every_caller_includes_the_header():
    use = re.compile(r"\b(%s)\s*\(|\b(Triple|SurfacePixel)\b" % "|".join(HELPERS))
    users = [f for f, src in CODE.items() if f != HOME and use.search(src)]
    assert set(users) == set(WRITERS) - {"frame_rays.hip"}      # (the ray kernel writes no plane: frame_plan.h is all it takes)
    for f in users:
        assert HOME in _includes(f), f
    for f in WRITERS:
        assert PLAN in _includes(f), f
    assert "composite_device.h" in _includes(HOME)
    # the header compiles as C++ on the host: no cross-lane operation and no LDS in it
    assert not re.search(r"__shfl|__ballot|wave_sum|wave_incl|__builtin_amdgcn|__shared__|__syncthreads|atomic", CODE[HOME])


def test_the_python_side_has_one_copy_of_each():
    assert [f for f, src in PYTHON.items() if "9999999" in src] == ["frame.py"]
    for text in ("def planes(", "def _check_devices("):
        assert not [f for f, src in PYTHON.items() if text in src], text
    assert sum(src.count("render_views needs at least one frame") for src in PYTHON.values()) == 1
    assert sum(src.count("the frame lives on") for src in PYTHON.values()) == 1
    assert sum(len(re.findall(r"\.max_nr_samples\s*=[^=]", src)) for f, src in PYTHON.items()
               if f in ("frame.py", "render.py", "nerf_view.py")) == 2       # frame.sample_pool: set, and put back


def test_no_function_imports_from_render_and_frame_py_is_a_leaf():
    for f, src in PYTHON.items():
        for node in ast.walk(ast.parse(src)):
            if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef)):
                inner = [n for n in ast.walk(node) if isinstance(n, ast.ImportFrom) and n.level == 1 and n.module == "render"]
                assert not inner, (f, node.name)
    imports = [n for n in ast.walk(ast.parse(PYTHON["frame.py"])) if isinstance(n, (ast.Import, ast.ImportFrom))]
    package = [n for n in imports if isinstance(n, ast.ImportFrom) and n.level]
    assert [(n.module, [a.name for a in n.names]) for n in package] == [(None, ["_lib"])]
    # the names callers and tests use stay reachable, as the same objects
    from permuto_sdf_amd import frame, mesh_color, nerf_view, render
    assert render.Frame is frame.Frame and render.FramePlan is frame.FramePlan and render.frame_rays is frame.frame_rays
    assert render.OccupancyGrid is not None
    assert nerf_view.IT_WINDOW_OPEN == mesh_color._IT_WINDOW_OPEN == frame.IT_WINDOW_OPEN
