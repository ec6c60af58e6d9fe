"""The point-to-mesh search (csrc/meshdist.hip through pcgcv1_amd/metrics.py: mesh_error) against the rule in numpy by brute
force over every triangle (tests/_mesh_error_ref.py): best bit for bit, nearest equal as arrays, the counts exactly, mse against
math.fsum of the reference's best within a relative N * 2^-53 (the bound for any order of a sum of non-negative terms), and
between two device runs bit for bit.  The meshes are the reference's own (tests/_surface_ref.py, tests/_simplify_ref.py), so no
device code stands between the test and its input; every mesh and every brute-force result is computed once per module, and no
comparison is above about 3 M pairs.

What the figures do and do not depend on: best and nearest are a function of each point and the triangle list, so they are
compared bit for bit across cell edges, across the internal order of the points and, permuted along, across the caller's order of
the points.  mse is summed in the caller's point order (include/pcgc.h): it is compared bit for bit across cell edges, the
internal order and the order of the triangles, and against the fsum bound where the caller permutes the points."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _mesh_error_ref as mref                                           # noqa: E402
import _simplify_ref as sref                                             # noqa: E402
import _surface_ref as ref                                               # noqa: E402
from pcgcv1_amd import _lib, ingest, metrics, surface                    # noqa: E402
from pcgcv1_amd import mesh_error as cli                                 # noqa: E402
from pcgcv1_amd.dataprocess import inout_points as iop                   # noqa: E402
from pcgcv1_amd.dataprocess import mesh2pc_open3d as m2p                 # noqa: E402
from _mesh_error_cases import A, B, C, DEGENERATE_POINTS, REGIONS, U, V_   # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "surface_sphere5_normals.npz")
C5 = (15.5, 15.5, 15.5)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _lib.require_gpu()


@functools.lru_cache(maxsize=None)
def cloud(name):
    if name == "sphere":
        return np.load(GOLDEN)["points"]
    if name == "torus":
        return ref.torus()
    ca, cb = (15.5, 15.5, 15.5), (45.5, 40.5, 40.5)
    return np.r_[ref.sphere(ca, 9.0), ref.sphere(cb, 11.0, seed=4)]


@functools.lru_cache(maxsize=None)
def mesh(name, cell=None):
    """(vertices, triangles) of the rule's mesh of a shape, its normals given; cell: simplified by the rule"""
    if cell is not None:
        v, t = mesh(name)
        return sref.simplify(v, t, 6 if name == "two" else 5, cell)[:2]
    p = cloud(name)
    if name == "sphere":
        v, t, _ = ref.reconstruct(p, np.load(GOLDEN)["normals"], 5, 3)
        return v, t
    if name == "torus":
        d = p - np.array(C5)
        rho = np.hypot(d[:, 0], d[:, 1])
        n = d - np.stack([d[:, 0] / rho * 9.0, d[:, 1] / rho * 9.0, 0 * rho], 1)
        nr, bits = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32), 5
    else:
        ca, cb = (15.5, 15.5, 15.5), (45.5, 40.5, 40.5)
        a = ref.sphere(ca, 9.0)
        nr, bits = np.r_[ref.sphere_normals(a, ca), ref.sphere_normals(p[len(a):], cb)], 6
    v, t, _ = ref.reconstruct(p, nr, bits, 3, mode="given")
    return v, t


_BRUTE = {}


def brute(key, points, v, t, max_dist=None):
    """the reference, once per key (the arrays are the key's own)"""
    if key not in _BRUTE:
        assert len(points) * len(t) <= 3_100_000
        best, nearest = mref.brute(points, v, t)
        best.setflags(write=False)
        nearest.setflags(write=False)
        _BRUTE[key] = (best, nearest)
    best, nearest = _BRUTE[key]
    if max_dist is not None:
        far = best > np.float64(max_dist) * np.float64(max_dist)
        best, nearest = np.where(far, np.inf, best), np.where(far, -1, nearest).astype(np.int32)
    return best, nearest


def _figures_match(fig, want_best):
    n, far, mse, top = mref.figures(want_best)
    assert (fig["points"], fig["far"]) == (n, far)
    if far == n:
        assert math.isnan(fig["mse (p2mesh)"]) and math.isnan(fig["rms (p2mesh)"]) and math.isnan(fig["h. (p2mesh)"])
    else:
        print("mse %r against fsum %r, %d points" % (fig["mse (p2mesh)"], mse, n - far))
        assert abs(fig["mse (p2mesh)"] - mse) <= (n - far) * 2.0 ** -53 * mse
        assert fig["h. (p2mesh)"] == top and fig["rms (p2mesh)"] == math.sqrt(fig["mse (p2mesh)"])


def check(key, points, v, t, max_dist=None, **kw):
    """one device run against the reference -> (figures, best, nearest)"""
    want_best, want_nearest = brute(key, points, v, t, max_dist)
    fig, (best, nearest) = metrics.mesh_error(points, v, t, max_dist, per_point=True, **kw)
    assert best.dtype == np.float64 and nearest.dtype == np.int32 and best.shape == nearest.shape == (len(points),)
    differ = int((best != want_best).sum())
    assert best.tobytes() == want_best.tobytes(), "%d of %d distances differ" % (differ, len(best))
    np.testing.assert_array_equal(nearest, want_nearest)
    _figures_match(fig, want_best)
    assert tuple(fig) == ("points", "far", "mse (p2mesh)", "rms (p2mesh)", "h. (p2mesh)", "edge", "pairs")
    return fig, best, nearest


# ---------------------------------------------------------------------------- 1, 2: one triangle, degenerate triangles
def test_one_triangle_and_the_same_triangle_twice():
    points = np.array([p for p, _ in REGIONS])
    v = np.stack([A, B, C])
    fig, best, nearest = check("regions", points, v, np.array([[0, 1, 2]]))
    assert best.tolist() == [w for _, w in REGIONS] and (nearest == 0).all() and fig["pairs"] == mref.pair_count(v, [[0, 1, 2]], 1.0)
    _, best2, nearest2 = check("regions twice", points, v, np.array([[0, 1, 2], [0, 1, 2]]))
    assert best2.tobytes() == best.tobytes() and (nearest2 == 0).all()
    _, best3, nearest3 = check("regions relabelled", points, v, np.array([[1, 2, 0], [0, 1, 2]]))     # equal to the last bit here: index 0
    assert best3.tolist() == best.tolist() and (nearest3 == 0).all()


def test_degenerate_triangles_alone_and_tied_with_a_regular_one():
    points = np.array(DEGENERATE_POINTS)
    v = np.stack([U, V_, (U + V_) / 2, np.array([1.0, 9.0, 3.0])])
    lone = np.array([[0, 0, 1], [0, 1, 1], [1, 0, 1], [0, 0, 0], [0, 2, 1], [2, 1, 0]])
    for k in range(len(lone)):
        check(("degenerate", k), points, v, lone[k: k + 1])
    _, _, nearest = check("degenerate all", points, v, lone)
    assert (nearest >= 0).all()
    # a regular triangle with the side U V_: a point nearest to that side ties with the segment (U, U, V_), whichever comes first
    mixed = np.array([[0, 1, 3], [0, 0, 1]])
    _, best, nearest = check("degenerate mixed", points, v, mixed)
    _, best2, nearest2 = check("degenerate mixed, swapped", points, v, mixed[::-1].copy())
    assert best.tobytes() == best2.tobytes()
    tie = mref.d2(points, U, V_, v[3]) == mref.d2(points, U, U, V_)
    assert tie.sum() >= 3 and (nearest[tie] == 0).all() and (nearest2[tie] == 0).all()       # the smallest index wins
    assert np.array_equal(nearest[~tie], 1 - nearest2[~tie])


# ---------------------------------------------------------------------------- 3, 4: the golden sphere and its simplified meshes
def test_the_golden_sphere_against_its_full_mesh():
    v, t = mesh("sphere")
    assert len(t) == 12168
    points = cloud("sphere")[::8]
    fig, _, _ = check("sphere full", points, v, t)
    assert (fig["edge"], fig["pairs"]) == (1, 36182)
    fig, _, _ = check("sphere full", points, v, t, max_dist=0.75)         # the gate takes some of them
    assert 0 < fig["far"] < len(points)


@pytest.mark.parametrize("cell,edge,pairs", [(2, 1, 13786), (4, 2, 3331), (16, 4, 312)])
def test_the_simplified_spheres_whose_triangles_span_many_cells(cell, edge, pairs):
    v, t = mesh("sphere", cell)
    points = cloud("sphere")
    assert len(points) == 1954
    key = ("sphere", cell)
    fig, best, nearest = check(key, points, v, t)
    assert (fig["edge"], fig["pairs"]) == (edge, pairs)
    mse = fig["mse (p2mesh)"]
    for forced in (1, 2, 8, 32):                                          # the cells do not show
        f, _, _ = check(key, points, v, t, _edge=forced)
        assert f["edge"] == forced and f["pairs"] == mref.pair_count(v, t, float(forced))
        assert f["mse (p2mesh)"] == mse and f["h. (p2mesh)"] == fig["h. (p2mesh)"]
    f, _, _ = check(key, points, v, t, _sort_points=False)                # nor does the internal order of the points
    assert f["mse (p2mesh)"] == mse
    f, _, _ = check(key, points, v, t)                                    # two runs, the same bytes
    assert f == fig
    rng = np.random.default_rng(cell)
    perm = rng.permutation(len(points))                                   # the caller's order: the per-point arrays go along
    f, (b, n) = metrics.mesh_error(points[perm], v, t, per_point=True)
    assert b.tobytes() == best[perm].tobytes() and np.array_equal(n, nearest[perm])
    _figures_match(f, best)
    assert f["h. (p2mesh)"] == fig["h. (p2mesh)"]
    tperm = rng.permutation(len(t))                                       # triangle tperm[k] becomes triangle k
    f, (b, n) = metrics.mesh_error(points, v, t[tperm], per_point=True)
    assert b.tobytes() == best.tobytes() and f["mse (p2mesh)"] == mse
    back = tperm[n]                                                       # a tie may pick another triangle, at the same distance
    moved = back != nearest
    if moved.any():
        vt = v[t]
        again = mref.d2(points[moved], vt[back[moved], 0], vt[back[moved], 1], vt[back[moved], 2])
        assert again.tobytes() == best[moved].tobytes()
        inverse = np.argsort(tperm)
        assert (inverse[back[moved]] <= inverse[nearest[moved]]).all()    # and then the one that comes first in the new list


# ---------------------------------------------------------------------------- 5: points outside the grid, the gate
def test_points_outside_the_grid_and_the_gate():
    v = np.stack([A, B, C, A + [0.5, 0.5, 1.0]])
    t = np.array([[0, 1, 2], [0, 1, 3]])
    points = np.array([[-3.5, -2.0, -7.0], [-0.25, 1.0, 1.0], [9.0, 1.0, 1.0], [1.0, 9.0, 1.0], [1.0, 1.0, 9.5], [1.0, -6.0, 1.0],
                       [1.0, 1.0, -6.0], [-6.0, 1.0, 1.5], [1.0, 1.0, 4.0], [1.0, 1.0, 1.0], [1000.5, 2.0, 1.0], [-1000.0, -1000.0, -1000.0],
                       [0.5, 0.5, 1.75], [12.0, 13.0, 14.0]])
    fig, best, _ = check("outside", points, v, t)
    assert fig["far"] == 0 and fig["edge"] == 1
    assert best[9] == 0.0 and best[10] == 996.5 ** 2 + 4.0
    for gate in (3.0, 0.5, 8.5, 1e-3):
        f, b, n = check("outside", points, v, t, max_dist=gate)
        assert f["far"] == int((best > gate * gate).sum()) and 0 < f["far"] < len(points)
    one = np.array([[0, 1, 2]])
    f, b, n = check("outside, one", np.array([[1.0, 1.0, 4.0], [1.0, 1.0, 4.5], [1.0, 1.0, 1.0]]), v, one, max_dist=3.0)
    assert b.tolist() == [9.0, np.inf, 0.0] and n.tolist() == [0, -1, 0] and f["far"] == 1        # best == max_dist^2 is not far
    f, b, n = check("outside, one", np.array([[1.0, 1.0, 4.0], [1.0, 1.0, 4.5], [1.0, 1.0, 1.0]]), v, one, max_dist=2.0 ** -20)
    assert f["far"] == 2
    # every point far: no mean, and no division by zero reported as a figure
    f, b, n = check("all far", points[[0, 2, 3, 10]], v, t, max_dist=1.0)
    assert f["far"] == f["points"] == 4 and np.isinf(b).all() and (n == -1).all()
    assert all(math.isnan(f[k]) for k in ("mse (p2mesh)", "rms (p2mesh)", "h. (p2mesh)"))
    # negative coordinates throughout: a mesh and a cloud left of zero, cells with negative origins
    shift = np.array([-40.0, -70.5, -3.25])
    f, b, n = check("outside, shifted", points + shift, v + shift, t)
    assert f["far"] == 0


# ---------------------------------------------------------------------------- 6: sizes around the launch shapes
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_point_counts_around_a_workgroup(n):
    v, t = mesh("sphere", 4)
    rng = np.random.default_rng(n)
    points = rng.uniform(-4.0, 36.0, (n, 3))                              # off the grid of voxels, inside and outside the mesh's box
    check(("counts", n), points, v, t)
    check(("counts, one triangle", n), points, v, t[5:6])


@pytest.mark.parametrize("n_pairs", [1, 256, 257])
def test_pair_counts_around_a_workgroup(n_pairs):
    rng = np.random.default_rng(n_pairs)
    corner = rng.integers(0, 12, (n_pairs, 1, 3)).astype(np.float64)      # every triangle inside one cell of edge 1
    v = (corner + rng.uniform(0.05, 0.95, (n_pairs, 3, 3))).reshape(-1, 3)
    t = np.arange(3 * n_pairs).reshape(-1, 3)
    points = rng.uniform(-2.0, 14.0, (300, 3))
    fig, _, _ = check(("pairs", n_pairs), points, v, t)
    assert (fig["edge"], fig["pairs"]) == (1, n_pairs)


@pytest.mark.parametrize("name", ["torus", "two"])
def test_the_torus_and_the_two_spheres(name):
    v, t = mesh(name)
    step = -(-len(cloud(name)) * len(t) // 3_000_000)                     # a subset: at most 3 M pairs for the brute force
    points = cloud(name)[::step]
    assert len(points) > 50
    fig, _, _ = check(name, points, v, t)
    assert fig["edge"] == 1 and fig["far"] == 0
    if name == "two":
        assert len(v) > 10000 and v.max() > 32                            # 6 bits


# ---------------------------------------------------------------------------- 7: the opposite direction
def test_samples_are_the_three_existing_calls():
    v, t = mesh("sphere", 2)
    points = cloud("sphere")
    dev = _lib.require_gpu()
    fig = metrics.mesh_error(points, v, t, samples=5000, seed=11)
    plain = metrics.mesh_error(points, v, t)
    assert {k: fig[k] for k in plain} == plain
    s = m2p.sample_points_uniformly(v, t.astype(np.int32), 5000, 11, device=True).to(torch.float32).contiguous()
    target = metrics._OffgridTarget(points.astype(np.float32), s.cpu().numpy(), dev)
    ws = torch.empty(int(_lib.hip().pcgc_offgrid_workspace_bytes(target.res, len(points))), dtype=torch.uint8, device=dev)
    mse, top, _, _ = metrics._offgrid_mse(s, target, None, ws)
    assert (fig["mse (mesh2p)"], fig["h. (mesh2p)"]) == (mse, top) and fig["h. (sym)"] == max(top, plain["h. (p2mesh)"])
    assert 0.0 < mse < 2.0                                                # the floor: samples fall between the voxels
    assert metrics.mesh_error(points, v, t, samples=5000, seed=11) == fig
    assert metrics.mesh_error(points, v, t, samples=5000, seed=12)["mse (mesh2p)"] != mse


# ---------------------------------------------------------------------------- 8, 9: end to end
def test_reconstruct_reports_the_error_of_the_mesh_it_returns():
    gold = np.load(GOLDEN)
    p, nr = gold["points"], gold["normals"]
    v0, t0, plain = surface.reconstruct(p, nr, 5, simplify=4)
    v, t, report = surface.reconstruct(p, nr, 5, simplify=4, error=True)
    assert "error" not in plain and v.tobytes() == v0.tobytes() and t.tobytes() == t0.tobytes()
    assert {k: x for k, x in report.items() if k not in ("error", "sign")} == {k: x for k, x in plain.items() if k != "sign"}
    assert report["error"] == metrics.mesh_error(p, v, t)
    assert report["error"]["points"] == len(p) and report["error"]["far"] == 0
    lines = surface.summary_line(report).splitlines()
    assert len(lines) == 3 and lines[:2] == surface.summary_line(plain).splitlines()
    e = report["error"]
    assert lines[2] == "error: rms %.3f, max %.3f voxels over %d points (cell edge %d, %d pairs)" % (
        e["rms (p2mesh)"], math.sqrt(e["h. (p2mesh)"]), len(p), e["edge"], e["pairs"])
    # with a frame the mesh is measured before it is rescaled: the same figures in voxels
    frame = ingest.Frame((1.0, -2.0, 0.5), 0.25, 5)
    fv, ft, framed = surface.reconstruct(p, nr, None, frame=frame, simplify=4, error=True)
    assert framed["error"] == report["error"] and fv.tobytes() == ingest.apply_frame(v, frame).tobytes()
    _, _, unsimplified = surface.reconstruct(p, nr, 5, error=True)
    assert unsimplified["error"]["pairs"] == 36182 and "simplify" not in unsimplified


def test_both_command_lines(tmp_path, monkeypatch, capsys):
    gold = np.load(GOLDEN)
    monkeypatch.chdir(tmp_path)
    iop.write_ply_normals("ball.ply", gold["points"], gold["normals"])
    surface.main(["--input", "ball.ply", "--output", "ball.obj", "--simplify", "4", "--error"])
    said = capsys.readouterr().out.splitlines()
    v, t = m2p.read_triangle_mesh("ball.obj")
    want = metrics.mesh_error(gold["points"], v, t)
    assert len(said) == 4 and said[1].startswith("simplify: cell 4") and said[3] == "wrote ball.obj"
    assert said[2] == "error: rms %.3f, max %.3f voxels over 1954 points (cell edge %d, %d pairs)" % (
        want["rms (p2mesh)"], math.sqrt(want["h. (p2mesh)"]), want["edge"], want["pairs"])
    cli.main(["--cloud", "ball.ply", "--mesh", "ball.obj"])
    said = capsys.readouterr().out.splitlines()
    assert said == cli.figure_lines(want)
    cli.main(["--cloud", "ball.ply", "--mesh", "ball.obj", "--max_dist", "0.5", "--samples", "2000", "--seed", "3"])
    said = capsys.readouterr().out.splitlines()
    gated = metrics.mesh_error(gold["points"], v, t, 0.5, 2000, 3)
    assert said == cli.figure_lines(gated) and gated["far"] > 0 and len(said) == 6
    # a mesh written in the scan's units comes back to voxel units through the same frame
    frame = ingest.Frame((-1.5, 2.0, 0.25), 0.125, 5)                     # a power-of-two step and an origin of few bits: exact both ways
    ingest.write_frame("ball.frame", frame)
    surface.main(["--input", "ball.ply", "--output", "scan.off", "--simplify", "4", "--frame", "ball.frame"])
    capsys.readouterr()
    sv, st = m2p.read_triangle_mesh("scan.off")
    assert np.abs(sv - ingest.apply_frame(v, frame)).max() < 1e-12 and np.array_equal(st, t)
    cli.main(["--cloud", "ball.ply", "--mesh", "scan.off", "--frame", "ball.frame", "--render", "ball.png", "--vmax", "1.5", "--size", "200", "120"])
    said = capsys.readouterr().out.splitlines()
    back = metrics.mesh_error(gold["points"], cli.unapply_frame(sv, frame), st)
    assert said[:-1] == cli.figure_lines(back, frame.step) and "in scan units" in said[1]
    assert abs(back["rms (p2mesh)"] - want["rms (p2mesh)"]) < 1e-9
    assert said[-1] == "ball.png: 200 x 120 png of 1954 points"
    data = open("ball.png", "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n" and int.from_bytes(data[16:20], "big") == 200 and int.from_bytes(data[20:24], "big") == 120


# ---------------------------------------------------------------------------- 10: errors
def test_python_refuses_what_the_rule_excludes():
    v, t = mesh("sphere", 4)
    points = cloud("sphere")[:50]
    bad_t = t.copy()
    bad_t[11, 2] = len(v)
    with pytest.raises(ValueError, match="triangle row 11.*outside 0..%d" % (len(v) - 1)):
        metrics.mesh_error(points, v, bad_t)
    bad_t[11, 2] = -1
    with pytest.raises(ValueError, match="triangle row 11"):
        metrics.mesh_error(points, v, bad_t)
    bad = v.copy()
    bad[17, 1] = np.nan
    with pytest.raises(ValueError, match="vertex row 17"):
        metrics.mesh_error(points, bad, t)
    bad[17, 1] = 2.0 ** 20
    with pytest.raises(ValueError, match="vertex row 17.*2\\^20"):
        metrics.mesh_error(points, bad, t)
    bad[17, 1] = -np.inf
    with pytest.raises(ValueError, match="vertex row 17"):
        metrics.mesh_error(points, bad, t)
    far_p = points.astype(np.float64)
    far_p[3, 0] = -(2.0 ** 20)
    with pytest.raises(ValueError, match="point row 3"):
        metrics.mesh_error(far_p, v, t)
    far_p[3, 0] = np.nan
    with pytest.raises(ValueError, match="point row 3"):
        metrics.mesh_error(far_p, v, t)
    with pytest.raises(ValueError, match="no triangles"):
        metrics.mesh_error(points, v, np.zeros((0, 3), np.int32))
    with pytest.raises(ValueError, match="no points"):
        metrics.mesh_error(np.zeros((0, 3)), v, t)
    for gate in (0, -2.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="max_dist"):
            metrics.mesh_error(points, v, t, max_dist=gate)
    for samples in (-1, 2.5):
        with pytest.raises(ValueError, match="samples"):
            metrics.mesh_error(points, v, t, samples=samples)
    with pytest.raises(ValueError, match="power of two"):
        metrics.mesh_error(points, v, t, _edge=3)
    # the largest coordinates the rule takes, on both sides: a far point and a far mesh
    edge = np.nextafter(2.0 ** 20, 0.0)
    check("extremes", np.array([[edge, -edge, 0.0], [0.0, 0.0, 0.0]]), np.array([[-edge, -edge, -edge], [-edge + 8, -edge, -edge], [-edge, -edge + 8, -edge]]),
          np.array([[0, 1, 2]]))


def test_tensors_and_integer_voxels_go_in_as_they_are():
    v, t = mesh("sphere", 4)
    points = cloud("sphere")
    dev = _lib.require_gpu()
    want = metrics.mesh_error(points, v, t, per_point=True)
    got = metrics.mesh_error(torch.from_numpy(points.astype(np.int32)).to(dev), torch.from_numpy(v).to(dev), torch.from_numpy(t.astype(np.int32)).to(dev),
                             per_point=True)
    assert got[0] == want[0] and got[1][0].tobytes() == want[1][0].tobytes() and np.array_equal(got[1][1], want[1][1])
