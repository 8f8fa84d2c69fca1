"""CPU: the marching-tetrahedra tables of the mesh kernels (permuto_sdf_amd/csrc/mesh_tables.h), parsed from the header, against
the tables compat/skimage/measure.py freezes -- and the winding rule the header states, which the stand-in does not have (it
orients by finite-difference normals): one fixed order per (tetrahedron, case) whose mid-edge geometric normal points from the
inside corners to the outside corners, reversed for the complementary case."""
import importlib.util
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "permuto_sdf_amd", "csrc", "mesh_tables.h")


def _standin():
    spec = importlib.util.spec_from_file_location("_standin_measure", os.path.join(ROOT, "compat", "skimage", "measure.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _table(name, shape):
    """the initialiser of `name` in the header as an int array (C literals: a leading 0 is octal)"""
    text = re.sub(r"//[^\n]*|/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"\b%s\b(?:\[\d+\])+\s*=\s*(\{.*?\})\s*;" % name, text, flags=re.S).group(1)
    vals = [int(t, 8) if len(t) > 1 and t[0] == "0" else int(t) for t in re.findall(r"\d+", body)]
    return np.array(vals).reshape(shape)


def _tables():
    return (_table("PSDF_MT_TETS", (6, 4)), _table("PSDF_MT_NTRI", (16,)), _table("PSDF_MT_TRIS", (6, 16, 2, 3)),
            _table("PSDF_MT_DIR_OF_OFFSET", (8,)), _table("PSDF_MT_OFFSET_OF_DIR", (7,)))


def _triangles(tris, t, case, ntri):
    """[(lo, hi) x 3] per triangle of one (tetrahedron, case)"""
    out = []
    for k in range(2):
        codes = tris[t, case, k]
        if k < ntri[case]:
            assert (codes != 0o377).all()
            out.append([(int(c) >> 3, int(c) & 7) for c in codes])
        else:
            assert (codes == 0o377).all()
    return out


def test_tetrahedra_and_case_edges_equal_the_standin():
    m = _standin()
    tets, ntri, tris, _, _ = _tables()
    assert {frozenset(t) for t in tets.tolist()} == {frozenset(t) for t in m._TETS.tolist()} and len(tets) == 6
    assert tets.tolist() == m._TETS.tolist()          # same order, so that `case` means the same bit assignment
    for t in range(6):
        for case in range(16):
            want = sorted(sorted(tuple(sorted((int(m._TETS[t][a]), int(m._TETS[t][b])))) for a, b in tri)
                          for tri in m._CASES.get(case, []))
            got = sorted(sorted(e) for e in _triangles(tris, t, case, ntri))
            assert got == want, (t, case)
            assert ntri[case] == len(m._CASES.get(case, []))


def test_edges_are_owned_by_their_lower_corner_and_directions_follow_the_linear_index():
    tets, ntri, tris, dir_of, off_of = _tables()
    for t in range(6):
        for case in range(16):
            for tri in _triangles(tris, t, case, ntri):
                for lo, hi in tri:
                    assert lo & hi == lo and lo != hi and lo in tets[t] and hi in tets[t]
    assert sorted(off_of.tolist()) == list(range(1, 8))
    for d, c in enumerate(off_of.tolist()):
        assert dir_of[c] == d
    # corner offset c = dx + 2 dy + 4 dz; the direction order is the order of the linear offset (dx Y + dy) Z + dz for any Y, Z >= 2
    for Y, Z in ((2, 2), (5, 3), (70, 129)):
        lin = [((c & 1) * Y + ((c >> 1) & 1)) * Z + (c >> 2) for c in off_of.tolist()]
        assert lin == sorted(lin) and len(set(lin)) == 7


def test_stored_winding_points_from_inside_to_outside_and_complements_are_reversed():
    m = _standin()
    tets, ntri, tris, _, _ = _tables()
    corner = m._CORNER.astype(np.float64)
    for t in range(6):
        for case in range(1, 15):
            inside = [int(tets[t][i]) for i in range(4) if case >> i & 1]
            outside = [int(tets[t][i]) for i in range(4) if not case >> i & 1]
            direction = corner[outside].mean(0) - corner[inside].mean(0)
            mine = _triangles(tris, t, case, ntri)
            for tri in mine:
                p = [0.5 * (corner[lo] + corner[hi]) for lo, hi in tri]
                normal = np.cross(p[1] - p[0], p[2] - p[0])
                assert normal @ direction > 1e-6, (t, case, tri)
            other = _triangles(tris, t, 15 - case, ntri)
            assert len(other) == len(mine)
            for a, b in zip(mine, other):
                rev = [a[0], a[2], a[1]]
                assert any(rev == b[i:] + b[:i] for i in range(3)), (t, case, a, b)
