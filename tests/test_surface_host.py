"""The surface rule on the CPU (tests/_surface_ref.py): the Kuhn cut and its combinatorial winding, the device's
copy of that rule (csrc/surface_tets.h, compiled here with g++), the orientation rounds on hand-made chains, the signed distance
of a plane, the --orient specs and the mesh writer."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _components_ref as components_ref                                # noqa: E402
import _surface_ref as ref                                              # noqa: E402
from pcgcv1_amd import surface                                          # noqa: E402
from pcgcv1_amd.dataprocess.mesh2pc_open3d import read_triangle_mesh    # noqa: E402


# ---------------------------------------------------------------------------- the Kuhn cut
def _analytic_mesh(points, bits, f_of):
    cells, k = ref.cells_and_vertices(points, bits)
    return ref.marching_tetrahedra(cells, ref.vertex_keys(k, bits), f_of(k + 0.5), bits)


def test_kuhn_cut_of_an_analytic_sphere_is_closed_and_consistently_wound():
    centre = np.array([7.3, 7.9, 8.1])
    p = ref.sphere(centre, 5.2, n=40000)
    v, t, ids = _analytic_mesh(p, 4, lambda x: np.linalg.norm(x - centre, axis=1) - 5.2)
    _, ucount, dmax = ref.edge_census(t)
    assert len(t) > 1000 and (ucount == 2).all() and dmax == 1
    assert ref.euler(v, t) == 2 and ref.boundary_loops(t) == (0, 0)
    assert (np.diff(ids) > 0).all() and len(ids) == len(v)
    volume = ref.signed_volume(v, t)
    assert 0.97 < volume / (4 / 3 * np.pi * 5.2 ** 3) < 1.0            # inscribed: linear interpolation of a convex f
    np.testing.assert_allclose(np.linalg.norm(v - centre, axis=1), 5.2, atol=0.08)
    np.testing.assert_array_equal(ref.canonical(t), surface.canonical(t))


def test_an_f_of_exactly_zero_keeps_the_mesh_closed_with_zero_area_triangles():
    p = np.stack(np.meshgrid(*[np.arange(2, 6)] * 3, indexing="ij"), -1).reshape(-1, 3)
    v, t, _ = _analytic_mesh(p, 3, lambda x: np.abs(x - 4.0).max(1) - 1.5)       # a cube whose faces pass through lattice vertices
    _, ucount, dmax = ref.edge_census(t)
    assert (ucount == 2).all() and dmax == 1 and ref.euler(v, t) == 2
    tri = v[t]
    area = np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    assert (area == 0).any() and ref.signed_volume(v, t) > 0


def test_the_combinatorial_winding_is_the_geometric_one_in_all_6_x_14_cases():
    seen = 0
    for pi in ref.PERMS:
        tc = ref.tet_corners(pi).astype(np.float64)
        assert np.sign(np.linalg.det(tc[1:] - tc[0])) == ref.perm_sign(pi)
        for mask in range(1, 15):
            inside = [(mask >> i) & 1 for i in range(4)]
            f = np.array([-(0.3 + 0.1 * i) if inside[i] else 0.4 + 0.15 * i for i in range(4)])
            tris = ref.tet_triangles(pi, mask)
            assert len(tris) == (2 if sum(inside) == 2 else 1)
            out_dir = tc[[i for i in range(4) if not inside[i]]].mean(0) - tc[[i for i in range(4) if inside[i]]].mean(0)
            for tri in tris:
                q = []
                for a, b in tri:
                    assert a < b and inside[a] != inside[b]
                    q.append(tc[a] + f[a] / (f[a] - f[b]) * (tc[b] - tc[a]))
                normal = np.cross(q[1] - q[0], q[2] - q[0])
                assert normal @ out_dir > 1e-6, (pi, mask)              # counter-clockwise seen from the f >= 0 side
            seen += 1
    assert seen == 84


def test_the_device_copy_of_the_rule_is_the_reference(tmp_path):
    exe = str(tmp_path / "surface_tets_check")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(HERE, "surface_tets_check.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    lines = subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.splitlines()
    assert len(lines) == 257
    bit = lambda c: int(c[0]) << 2 | int(c[1]) << 1 | int(c[2])
    for inside in range(256):
        want = []
        for pi in ref.PERMS:
            tc = ref.tet_corners(pi)
            mask = sum(((inside >> bit(tc[i])) & 1) << i for i in range(4))
            for tri in ref.tet_triangles(pi, mask):
                want += [bit(tc[a]) << 3 | bit(tc[b]) for a, b in tri]
        assert [int(x) for x in lines[inside].split()] == [inside] + want
    dirs = [bit(d) for d in ref.DIRS]
    assert lines[256].split() == ["dir"] + [str(dirs.index(d)) for d in range(1, 8)] + [str(d) for d in dirs]


# ---------------------------------------------------------------------------- orientation
S75 = np.float32(np.sqrt(0.75))


def test_a_doubtful_link_waits_for_the_stage_to_relax_and_the_stage_resets():
    p = np.array([[x, 0, 0] for x in range(5)], np.int32)
    tilted = (0, S75, 0.5)
    nr = np.array([(0, 0, -1), (0, 0, 1), tilted, (0, 0, 1), (0, 0, 1)], np.float32)
    # seed 4; round 1 sets 3; round 2 nothing (c = 0.5 < 0.9); round 3 sets 2; round 4 nothing again: the stage went back to 0;
    # round 5 sets 1; round 6 sets 0 against its neighbour
    sign, rounds = ref.orient(p, nr, 3)
    assert sign.tolist() == [-1, 1, 1, 1, 1] and rounds == 6
    assert ref.orient(p, nr, 3, tau=(0.0,))[1] == 4                      # nothing waits
    assert ref.orient(p, nr, 3, tau=(0.9, 0.6, 0.0))[1] == 8             # two relaxations per doubtful link
    order = np.array([3, 0, 4, 2, 1])
    sign, rounds = ref.orient(p[order], nr[order], 3)
    assert sign.tolist() == [1, -1, 1, 1, 1] and rounds == 6


def test_a_tie_goes_to_the_smaller_key():
    p = np.array([[4, 1, 0], [3, 0, 0], [3, 2, 0], [2, 1, 0]], np.int32)  # seed, j1, j2 (not linked to each other), i
    for flip in (1, -1):
        nr = np.array([(0, 0, 1), (0.6 * flip, 0, 0.8), (-0.6 * flip, 0, 0.8), (1, 0, 0)], np.float32)
        sign, rounds = ref.orient(p, nr, 3, tau=(0.0,))
        assert rounds == 2 and sign.tolist() == [1, 1, 1, flip]          # c = +-0.6 from j1, -+0.6 from j2: j1 has the smaller key
    with pytest.raises(ValueError, match="last"):
        ref.orient(p, nr, 3, tau=(0.5,))


def test_every_component_has_its_own_seed_and_a_gap_bridges():
    p = np.array([[1, 1, 1], [1, 1, 2], [6, 6, 6], [6, 5, 6]], np.int32)
    nr = np.array([(1, 0, 0), (-1, 0, 0), (1, 0, 0), (-1, 0, 0)], np.float32)
    sign, rounds = ref.orient(p, nr, 3)
    assert sign.tolist() == [1, -1, 1, -1] and rounds == 1               # seeds: (1,1,2) with nx < 0, (6,6,6) with nx > 0
    np.testing.assert_array_equal(ref.oriented(nr, sign)[:, 0], [1, 1, 1, 1])    # every seed is turned towards +x, its component with it
    p = np.array([[0, 0, 0], [2, 0, 0]], np.int32)
    nr = np.array([(-0.6, 0.8, 0), (0.6, 0.8, 0)], np.float32)
    assert ref.orient(p, nr, 3, gap=1) == (pytest.approx([-1, 1]), 0)
    sign, rounds = ref.orient(p, nr, 3, gap=2)                           # one component: c = 0.28 is taken at the second stage
    assert sign.tolist() == [1, 1] and rounds == 2


def test_labels_are_the_component_rules():
    rng = np.random.default_rng(5)
    p = np.unique(rng.integers(0, 16, (300, 3)), axis=0)
    for gap in (1, 2, 3):
        want = components_ref.components(p, 4, gap)
        got = ref.components(p, 4, gap)
        np.testing.assert_array_equal(got[0], want[0])
        assert got[1] == want[2] and (gap > 1 or got[1] > 1)


def test_view_and_given():
    p = np.array([[1, 2, 3], [5, 5, 5], [7, 0, 2]], np.int32)
    nr = np.array([(1, 0, 0), (0, -1, 0), (0, 0, 1)], np.float32)
    assert ref.orient(p, nr, 3, "given") == (pytest.approx([1, 1, 1]), 0)
    sign, rounds = ref.orient(p, nr, 3, "view", view=(0.0, 0.0, 2.0))
    assert sign.tolist() == [-1, 1, 1] and rounds == 0                   # the third is at a right angle: not < 0, so +1
    np.testing.assert_array_equal(ref.oriented(nr, sign), nr.astype(np.float64) * np.array([[-1], [1], [1]]))


# ---------------------------------------------------------------------------- the signed distance
def test_the_signed_distance_of_a_plane_is_the_height_above_it():
    p = np.stack(np.meshgrid(np.arange(16), np.arange(16), [5], indexing="ij"), -1).reshape(-1, 3)
    N = np.tile([0.0, 0.0, 1.0], (len(p), 1))
    for R in (3, 5, 8):
        keys, f = ref.implicit(p, N, 4, R)
        k = ref.vertex_of_key(keys, 4)
        assert (np.diff(keys) > 0).all() and k.min() == -2 and k[:, 2].min() == 3 and k[:, 2].max() == 6
        np.testing.assert_allclose(f, k[:, 2] + 0.5 - 5, rtol=0, atol=1e-12)
    for R in (2, 9):
        with pytest.raises(ValueError, match="radius"):
            ref.implicit(p, N, 4, R)


def test_cells_and_vertices_leave_the_grid():
    cells, k = ref.cells_and_vertices(np.array([[0, 0, 0], [7, 7, 7]]), 3)
    assert len(cells) == 54 and cells.min() == -1 and cells.max() == 8
    assert len(k) == 128 and k.min() == -2 and k.max() == 8


# ---------------------------------------------------------------------------- specs
def test_orient_specs():
    assert surface.parse_orient("given") == surface.Orient("given")
    assert surface.parse_orient("propagate") == surface.Orient("propagate", 1)
    assert surface.parse_orient("propagate:8").gap == 8
    assert surface.parse_orient("view:1,-2.5,3e2").view == (1.0, -2.5, 300.0)
    assert repr(surface.parse_orient("view:0,0,0")) == "Orient('view:0,0,0')"
    for bad, what in (("propagate:0", "gap"), ("propagate:9", "gap"), ("propagate:x", "integer"), ("view", "none of"), ("view:1,2", "three"),
                      ("view:1,2,nan", "three"), ("view:a,b,c", "three"), ("given:1", "none of"), ("hoppe", "none of"), ("", "none of")):
        with pytest.raises(ValueError, match=what):
            surface.parse_orient(bad)
    assert surface.check_tau([0.5, 0]) == (0.5, 0.0)
    for bad, what in (((0.9, 0.1), "last"), ((), "1 to 8"), ((1.5, 0.0), "within"), ((0.0,) * 9, "1 to 8")):
        with pytest.raises(ValueError, match=what):
            surface.check_tau(bad)
    for bad in (2, 9, 3.5):
        with pytest.raises(ValueError, match="radius"):
            surface.check_radius(bad)
    assert [surface.check_radius(r) for r in (3, 8)] == [3, 8]
    for bad in (0, 13):
        with pytest.raises(ValueError, match="bits"):
            surface.check_bits(bad)


def test_argument_errors_come_before_any_file_is_read(capsys):
    for argv, what in ((["--radius", "9"], "radius"), (["--orient", "propagate:9"], "gap"), (["--orient", "view:1"], "three")):
        with pytest.raises(SystemExit):
            surface.main(["--input", "no_such.ply", "--output", "x.obj"] + argv)
        assert what in capsys.readouterr().err
    with pytest.raises(SystemExit):
        surface.main(["--input", "no_such.ply", "--output", "x.stl"])
    assert ".obj or .off" in capsys.readouterr().err
    args = surface.parse_args(["--input", "a.ply", "--output", "a.off", "--orient", "view:1,2,3", "--radius", "5"])
    assert args.orient.view == (1.0, 2.0, 3.0) and args.radius == 5 and not args.estimate_normals and args.frame == ""


# ---------------------------------------------------------------------------- files
@pytest.mark.parametrize("ext", [".obj", ".off"])
def test_write_mesh_then_read_triangle_mesh_is_exact(tmp_path, ext):
    rng = np.random.default_rng(9)
    v = np.r_[rng.normal(size=(40, 3)) * 10.0 ** rng.integers(-8, 9, (40, 1)), [[0.1 + 0.2, 1e-300, -1.5e300], [1 / 3, 2.0 ** -1060, 123456789.125]]]
    t = rng.integers(0, len(v), (70, 3)).astype(np.int32)
    name = str(tmp_path / ("m" + ext))
    surface.write_mesh(name, v, t)
    got_v, got_t = read_triangle_mesh(name)
    assert got_v.dtype == np.float64 and got_t.dtype == np.int32
    assert got_v.tobytes() == v.tobytes() and got_t.tobytes() == t.tobytes()
    with pytest.raises(ValueError, match="obj or .off"):
        surface.write_mesh(str(tmp_path / "m.ply"), v, t)
    with pytest.raises(ValueError, match="outside"):
        surface.write_mesh(name, v, t + len(v))


def test_canonical_and_boundary_edges():
    t = np.array([[5, 1, 3], [2, 0, 1], [3, 2, 1]])
    assert surface.canonical(t).tolist() == [[0, 1, 2], [1, 3, 2], [1, 3, 5]]
    assert surface.boundary_edges(np.array([[0, 1, 2], [0, 2, 3]])) == 4
    tet = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]])
    assert surface.boundary_edges(tet) == 0 and ref.boundary_loops(tet) == (0, 0) and ref.euler(np.zeros((4, 3)), tet) == 2
    assert ref.boundary_loops(np.array([[0, 1, 2], [0, 2, 3]])) == (1, 4)
