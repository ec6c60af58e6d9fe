"""The simplification rule on the CPU (tests/_simplify_ref.py): the device's copy of the quadric and its solve
(csrc/surface_quadric.h, compiled here with g++) bit for bit, the rule on the reference's mesh of the golden 5-bit sphere with its
counts pinned, the balance of the edges on closed and open meshes, independence of the input order, the edge cases, and the
arguments and text of the command lines.

The counts below are the reference's own (_simplify_ref on _surface_ref's mesh, on the CPU), not the device's: the device is
held to the reference in tests/test_gpu_simplify.py."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _simplify_ref as sref                                            # noqa: E402
import _surface_ref as ref                                              # noqa: E402
from pcgcv1_amd import surface                                          # noqa: E402
from pcgcv1_amd.dataprocess.mesh2pc_open3d import read_triangle_mesh    # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "surface_sphere5_normals.npz")


@functools.lru_cache(maxsize=None)
def sphere_mesh():
    gold = np.load(GOLDEN)
    v, t, _ = ref.reconstruct(gold["points"], gold["normals"], 5, 3)
    return v, t


@functools.lru_cache(maxsize=None)
def analytic_mesh(name):
    """closed and open meshes without normal estimation: marching tetrahedra of an analytic signed distance"""
    if name == "torus":
        p, c = ref.torus(), np.array([15.5, 15.5, 15.5])
        f_of = lambda x: np.hypot(np.hypot(x[:, 0] - c[0], x[:, 1] - c[1]) - 9.0, x[:, 2] - c[2]) - 4.2
    else:
        p = ref.paraboloid()
        f_of = lambda x: x[:, 2] - (8.0 + ((x[:, 0] - 15.5) ** 2 + (x[:, 1] - 15.5) ** 2) / 24.0)
    cells, k = ref.cells_and_vertices(p, 5)
    v, t, _ = ref.marching_tetrahedra(cells, ref.vertex_keys(k, 5), f_of(k + 0.5), 5)
    return v, t


# ---------------------------------------------------------------------------- the header is the rule
def _hex(values):
    return " ".join(float(x).hex() for x in np.asarray(values, np.float64).reshape(-1))


def _plane_cluster(normal, offset, o, rng, n=6):
    """n triangles in the plane normal . (x - o) = offset, near the centre o"""
    normal = np.asarray(normal, np.float64) / np.linalg.norm(normal)
    u = np.cross(normal, [0.3, 0.5, 0.8])
    u /= np.linalg.norm(u)
    w = np.cross(normal, u)
    ab = rng.uniform(-0.9, 0.9, (n, 3, 2))
    return o + offset * normal + ab[..., :1] * u + ab[..., 1:] * w


def _clusters():
    rng = np.random.default_rng(11)
    o = np.array([7.0, 9.0, 11.0])                                       # the centre of cell (4, 5, 6) at cell 2
    items, kinds = [], []
    # one plane: rank 1
    n1 = np.array([1.0, 2.0, -0.5])
    tri = _plane_cluster(n1, 0.3, o, rng)
    items.append((2, o, tri.reshape(-1, 3), tri))
    kinds.append(("plane", n1 / np.linalg.norm(n1), 0.3))
    # two planes: rank 2, a crease
    n2 = np.array([-1.0, 0.4, 0.2])
    tri = np.r_[_plane_cluster(n1, 0.3, o, rng), _plane_cluster(n2, -0.2, o, rng)]
    items.append((2, o, tri.reshape(-1, 3), tri))
    kinds.append(("crease", (n1 / np.linalg.norm(n1), 0.3), (n2 / np.linalg.norm(n2), -0.2)))
    # the three planes of a cube corner: rank 3
    corner = o + np.array([0.25, -0.5, 0.125])
    tri = np.concatenate([_plane_cluster(e, e @ (corner - o), o, rng, 4) for e in np.eye(3)])
    items.append((2, o, tri.reshape(-1, 3), tri))
    kinds.append(("corner", corner))
    # three planes whose common point lies outside the cube: fallback
    far = o + np.array([1.5, 0.2, -0.3])
    tri = np.concatenate([_plane_cluster(e, e @ (far - o), o, rng, 4) for e in (np.array([1.0, 0.1, 0.0]), np.array([0.0, 1.0, 0.2]), np.eye(3)[2])])
    items.append((2, o, (o + rng.uniform(-0.9, 0.9, (5, 3))), tri))
    kinds.append(("outside",))
    # no triangle at all, and triangles of zero area: an all-zero quadric, fallback
    vs = o + rng.uniform(-0.9, 0.9, (4, 3))
    items.append((2, o, vs, np.zeros((0, 3, 3))))
    kinds.append(("zero",))
    items.append((3, o + 0.5, vs, np.stack([np.stack([vs[0], vs[1], vs[1]]), np.stack([vs[2], vs[2], vs[2]])])))
    kinds.append(("zero",))
    return items, kinds


def test_the_device_copy_of_the_quadric_is_the_reference(tmp_path):
    exe = str(tmp_path / "surface_quadric_check")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", os.path.join(HERE, "surface_quadric_check.cpp"),
                            "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    items, kinds = _clusters()
    sv, st = sphere_mesh()
    keys, rank, centre = sref.clusters(sv, 5, 3)                         # and every cluster of the sphere at cell 3
    ct = sref.canonical(st)
    for k in range(len(keys)):
        items.append((3, centre[k], sv[rank == k], sv[ct[(rank[ct] == k).any(1)]]))
    text = ["%d" % len(items)]
    for cell, o, vs, ts in items:
        vs, ts = np.asarray(vs).reshape(-1, 3), np.asarray(ts).reshape(-1, 3, 3)
        text += ["%d %d %d" % (cell, len(vs), len(ts)), _hex(o)] + [_hex(r) for r in vs] + [_hex(r) for r in ts]
    run = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stderr
    lines = run.stdout.splitlines()
    assert len(lines) == len(items)
    got = np.array([[float.fromhex(x) for x in ln.split()[:3]] for ln in lines])
    got_fb = np.array([int(ln.split()[3]) for ln in lines], bool)
    want, want_fb = sref.place_clusters(items)
    assert got.tobytes() == want.tobytes()                               # bit for bit
    np.testing.assert_array_equal(got_fb, want_fb)
    # the sphere's clusters through the whole rule give the same vertices (the test's own gather is the rule's)
    sv3, _, rep3 = sref.simplify(sv, st, 5, 3)
    assert got[len(kinds):].tobytes() == sv3.tobytes() and int(got_fb[len(kinds):].sum()) == rep3["fallback"]
    # and they are what the cases say
    for (cell, o, vs, ts), kind, x, fb in zip(items, kinds, got, got_fb):
        m = np.asarray(vs).reshape(-1, 3).mean(0)
        if kind[0] == "plane":
            _, normal, offset = kind
            assert not fb and abs(normal @ (x - o) - offset) < 1e-12
            move = x - m
            np.testing.assert_allclose(move - (move @ normal) * normal, 0, atol=1e-12)       # the mean moves only along the normal
        elif kind[0] == "crease":
            assert not fb
            for normal, offset in kind[1:]:
                assert abs(normal @ (x - o) - offset) < 1e-12
        elif kind[0] == "corner":
            assert not fb
            np.testing.assert_allclose(x, kind[1], rtol=0, atol=1e-12)
        else:
            assert fb
            np.testing.assert_allclose(x, m, rtol=0, atol=1e-14)


# ---------------------------------------------------------------------------- the rule on the reference mesh
# cell: (vertices, triangles, fallback, degenerate) of _simplify_ref on _surface_ref's mesh of the golden sphere (6 086 vertices,
# 12 168 triangles): the reference's own figures
SPHERE_COUNTS = {1: (1641, 3278, 3, 8890), 2: (458, 912, 18, 11256), 3: (227, 450, 10, 11718), 4: (122, 240, 9, 11928)}


@pytest.mark.parametrize("cell", [1, 2, 3, 4])
def test_the_rule_on_the_golden_sphere(cell):
    v, t = sphere_mesh()
    assert (len(v), len(t)) == (6086, 12168)
    volume = ref.signed_volume(v, t)
    sv, st, rep = sref.simplify(v, t, 5, cell)
    assert sv.dtype == np.float64 and st.dtype == np.int32 and tuple(rep) == sref.REPORT_KEYS
    print("cell %d: %s, volume %.6g of %.6g" % (cell, rep, ref.signed_volume(sv, st), volume))
    assert (len(sv), len(st), rep["fallback"], rep["degenerate"]) == SPHERE_COUNTS[cell]
    assert (rep["cell"], rep["clusters"], rep["vertices_in"], rep["triangles_in"]) == (cell, len(sv), 6086, 12168)
    assert rep["folded"] == 0 and rep["cancelled"] == 0 and rep["unused"] == 0
    assert rep["degenerate"] + len(st) + rep["merged"] <= len(t)
    _, balance, count = sref.edge_balance(st)
    assert (balance == 0).all() and (count == 2).all()
    assert ref.euler(sv, st) == 2
    lo_hi = np.sort(st[:, 1:], 1)
    order = np.lexsort((lo_hi[:, 1], lo_hi[:, 0], st[:, 0]))
    assert (order == np.arange(len(st))).all() and (st[:, 0] < lo_hi[:, 0]).all()           # ascending (a, lo, hi), a the smallest
    mv, mt, _ = sref.simplify(v, t, 5, cell, "mean")
    np.testing.assert_array_equal(mt, st)
    assert abs(ref.signed_volume(sv, st) - volume) < abs(ref.signed_volume(mv, mt) - volume)
    assert np.abs(sv - (sref.clusters(v, 5, cell)[2])).max() <= cell / 2.0                  # every vertex inside its cube


# ---------------------------------------------------------------------------- balance and boundary
def test_the_torus_at_cell_8_stays_balanced():
    v, t = analytic_mesh("torus")
    _, balance, count = sref.edge_balance(t)
    assert (balance == 0).all() and (count == 2).all() and ref.euler(v, t) == 0
    for cell in (2, 8):
        sv, st, rep = sref.simplify(v, t, 5, cell)
        _, balance, count = sref.edge_balance(st)
        print("torus, cell %d: %s, %d edges not in two triangles" % (cell, rep, int((count != 2).sum())))
        assert rep["folded"] == 0 and len(st) > 0
        assert (balance == 0).all()                                      # also where an edge is not in exactly two triangles
        assert (count % 2 == 0).all() and (count != 2).any() == (cell == 8)


def test_the_open_patch_keeps_the_image_of_its_boundary():
    v, t = analytic_mesh("patch")
    und, balance, count = sref.edge_balance(t)
    assert ref.boundary_loops(t)[0] == 1 and (np.abs(balance) == (count == 1)).all()
    sv, st, rep, to = sref.simplify(v, t, 5, 2, vertex_map=True)
    assert rep["folded"] == 0
    # the image of the input's boundary chain: its directed edges under the vertex map, the net flow per undirected edge
    a, b, direction = to[und[balance != 0, 0]], to[und[balance != 0, 1]], balance[balance != 0]
    assert a.min() >= 0 and b.min() >= 0                                 # no boundary vertex lost its cluster
    flow = {}
    for x, y, s in zip(a.tolist(), b.tolist(), direction.tolist()):
        if x != y:
            lo, hi, s = (x, y, s) if x < y else (y, x, -s)
            flow[(lo, hi)] = flow.get((lo, hi), 0) + s
    want = {k: s for k, s in flow.items() if s}
    und2, balance2, _ = sref.edge_balance(st)
    got = {(int(x), int(y)): int(s) for (x, y), s in zip(und2, balance2) if s}
    assert got == want and len(got) > 10


# ---------------------------------------------------------------------------- order independence and edge cases
def test_permuted_and_rotated_triangles_give_the_same_bytes():
    v, t = sphere_mesh()
    rng = np.random.default_rng(3)
    perm = rng.permutation(len(t))
    shift = rng.integers(0, 3, len(t))
    t2 = np.stack([t[perm, (shift + s) % 3] for s in range(3)], 1)
    assert not np.array_equal(t2, t)
    for cell in (2, 16):
        a, b = sref.simplify(v, t, 5, cell), sref.simplify(v, t2, 5, cell)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]


def test_edge_cases():
    v, t = sphere_mesh()
    sv, st, rep = sref.simplify(v, t, 5, 64)                             # everything in one cluster
    assert sv.shape == (0, 3) and st.shape == (0, 3) and st.dtype == np.int32
    assert rep["clusters"] == 1 and rep["degenerate"] == len(t) and rep["unused"] == 1
    sv, st, rep = sref.simplify(v, np.zeros((0, 3), np.int32), 5, 2)     # no triangle
    assert sv.shape == (0, 3) and st.shape == (0, 3) and rep["unused"] == rep["clusters"] == 458 and rep["fallback"] == 458
    one_v = np.array([[0.5, 0.5, 0.5], [5.5, 0.5, 0.25], [0.5, 7.5, 1.5], [0.75, 0.5, 0.5]])
    sv, st, rep = sref.simplify(one_v, np.array([[2, 0, 1]]), 3, 2)      # a single triangle
    assert st.tolist() == [[0, 2, 1]] and rep["clusters"] == 3 and rep["fallback"] == 0
    normal = np.cross(one_v[1] - one_v[0], one_v[2] - one_v[0])
    np.testing.assert_allclose((sv - one_v[0]) @ normal, 0, atol=1e-9)   # every placed vertex in the triangle's plane
    np.testing.assert_allclose(sv[1:], one_v[[2, 1]], atol=1e-12)        # a lone vertex stays where it is; ascending key: x first
    a, b, c = sv[st[0]]
    np.testing.assert_allclose(np.cross(b - a, c - a) @ normal / (normal @ normal), 1, atol=0.2)   # the same side up
    sv, st, rep = sref.simplify(one_v, np.array([[0, 1, 2], [0, 2, 1]]), 3, 2)           # a pillow cancels
    assert st.shape == (0, 3) and rep["cancelled"] == 1 and rep["merged"] == 1 and rep["unused"] == 3
    sv, st, rep = sref.simplify(one_v, np.array([[0, 1, 2], [3, 1, 2]]), 3, 2)           # twice the same triple: folded
    assert st.tolist() == [[0, 2, 1]] and rep["folded"] == 1 and rep["merged"] == 1
    for bad in (0, 65, 2.5):
        with pytest.raises(ValueError, match="cell"):
            sref.simplify(one_v, np.array([[0, 1, 2]]), 3, bad)
        with pytest.raises(ValueError, match="cell"):
            surface.check_cell(bad)
    assert surface.check_cell(64) == 64 and surface.MAX_CELL == sref.MAX_CELL
    for bad_v in (np.array([[np.nan, 0, 0]]), np.array([[10.0, 0, 0]]), np.array([[0, -2.5, 0]])):
        with pytest.raises(ValueError, match="vertex"):
            sref.simplify(bad_v, np.zeros((0, 3)), 3, 2)
    with pytest.raises(ValueError, match="names a vertex"):
        sref.simplify(one_v, np.array([[0, 1, 4]]), 3, 2)


# ---------------------------------------------------------------------------- errors and text
def test_argument_errors_come_before_any_file_is_read(capsys):
    for cell in ("0", "65"):
        with pytest.raises(SystemExit):
            surface.main(["--input", "no_such.ply", "--output", "x.obj", "--simplify", cell])
        assert "cell = %s outside 1..64" % cell in capsys.readouterr().err
    with pytest.raises(SystemExit):
        surface.main(["--input", "no_such.ply", "--output", "x.obj", "--simplify", "two"])
    assert "--simplify" in capsys.readouterr().err
    args = surface.parse_args(["--input", "a.ply", "--output", "a.off", "--simplify", "3"])
    assert args.simplify == 3 and surface.parse_args(["--input", "a.ply", "--output", "a.off"]).simplify is None
    from pcgcv1_amd import test as cli
    for cell in ("0", "65"):
        with pytest.raises(SystemExit):
            cli.main(["decompress", "no_such", "out.ply", "--mesh", "x.obj", "--mesh_simplify", cell])
        assert "cell = %s outside 1..64" % cell in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.main(["decompress", "no_such", "out.ply", "--mesh_simplify", "2"])
    assert "give --mesh" in capsys.readouterr().err
    assert not os.path.exists("out.ply")


def test_the_summary_gains_a_second_line():
    report = dict(voxels=1722, components=1, rounds=19, vertices=458, triangles=912, boundary_edges=0)
    first = "surface: 1722 voxels, 1 components, 19 rounds, 458 vertices, 912 triangles, 0 boundary edges"
    assert surface.summary_line(report) == first
    report["simplify"] = dict(cell=2, clusters=458, vertices_in=6086, triangles_in=12168, degenerate=11256, cancelled=0, merged=0, folded=0,
                              fallback=18, unused=0)
    assert surface.summary_line(report) == first + "\nsimplify: cell 2, 6086 vertices and 12168 triangles -> 458 and 912, " \
                                                   "18 of 458 clusters placed at their mean"


@pytest.mark.parametrize("ext", [".obj", ".off"])
def test_a_simplified_mesh_through_a_file_is_exact(tmp_path, ext):
    v, t = sphere_mesh()
    sv, st, _ = sref.simplify(v, t, 5, 3)
    name = str(tmp_path / ("m" + ext))
    surface.write_mesh(name, sv, st)
    got_v, got_t = read_triangle_mesh(name)
    assert got_v.tobytes() == sv.tobytes() and got_t.tobytes() == st.tobytes() and got_t.dtype == np.int32
