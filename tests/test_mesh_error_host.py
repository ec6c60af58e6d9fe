"""The point-to-mesh rule on the CPU (tests/_mesh_error_ref.py): the device's copy of the point-triangle function
(csrc/point_triangle.h, compiled here with g++) bit for bit, the reference against geometry, the choice of the cell edge on the
reference's meshes of the golden 5-bit sphere, and the arguments and text of the command lines.

The pair counts and figures below are the reference's own (on _surface_ref's and _simplify_ref's meshes, on the CPU), not the
device's: the device is held to the reference in tests/test_gpu_mesh_error.py."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _mesh_error_ref as mref                                           # noqa: E402
from _mesh_error_cases import A, B, C, DEGENERATE, DEGENERATE_POINTS, M_, REGIONS, U, V_   # noqa: E402
import _simplify_ref as sref                                             # noqa: E402
import _surface_ref as ref                                               # noqa: E402
from pcgcv1_amd import mesh_error as cli                                 # noqa: E402
from pcgcv1_amd import metrics, surface                                  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "surface_sphere5_normals.npz")

@functools.lru_cache(maxsize=None)
def sphere():
    gold = np.load(GOLDEN)
    v, t, _ = ref.reconstruct(gold["points"], gold["normals"], 5, 3)
    return gold["points"], v, t


@functools.lru_cache(maxsize=None)
def simplified(cell):
    _, v, t = sphere()
    return sref.simplify(v, t, 5, cell)[:2]


def random_pairs(n, seed=5):
    """points and triangles on a grid of 1/1024 within +-64, some of them slivers, some points in the triangle's plane"""
    rng = np.random.default_rng(seed)
    q = rng.integers(-65536, 65537, (n, 4, 3)) / 1024.0
    q[: n // 8, 3] = q[: n // 8, 1] + (q[: n // 8, 2] - q[: n // 8, 1]) * 0.5 + rng.integers(-2, 3, (n // 8, 3)) / 1024.0       # slivers
    w = rng.integers(-1, 4, (n // 8, 2)) / 4.0                            # in the triangle's plane, inside and outside
    k = slice(n // 8, n // 4)
    q[k, 0] = (w[:, :1] * q[k, 1] + w[:, 1:] * q[k, 2]) + (1.0 - w[:, :1] - w[:, 1:]) * q[k, 3]
    return q[:, 0], q[:, 1], q[:, 2], q[:, 3]


# ---------------------------------------------------------------------------- the header is the rule
def _hex(values):
    return " ".join(float(x).hex() for x in np.asarray(values, np.float64).reshape(-1))


def test_the_device_copy_of_the_rule_is_the_reference(tmp_path):
    exe = str(tmp_path / "point_triangle_check")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", os.path.join(HERE, "point_triangle_check.cpp"),
                            "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    rows = [(p, A, B, C) for p, _ in REGIONS] + [(p, C, A, B) for p, _ in REGIONS]
    rows += [(p, *tri) for _, tri in DEGENERATE for p in DEGENERATE_POINTS]
    rows += list(zip(*random_pairs(4000)))
    points, v, t = sphere()
    rows += [(points[7].astype(np.float64), v[a], v[b], v[c]) for a, b, c in t.tolist()]           # every triangle of the sphere's mesh
    p, a, b, c = (np.array([r[k] for r in rows], np.float64) for k in range(4))
    text = "%d\n" % len(rows) + "\n".join(_hex(np.concatenate(r)) for r in zip(p, a, b, c)) + "\n"
    run = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    got = np.array([float.fromhex(x) for x in run.stdout.split()])
    want = mref.d2(p, a, b, c)
    assert len(got) == len(rows) == 2 * len(REGIONS) + 36 + 4000 + 12168
    differ = got != want
    assert got.tobytes() == want.tobytes(), "%d of %d values differ, first at row %d" % (differ.sum(), len(got), int(np.argmax(differ)))
    counts, _ = mref.face(p, a, b, c)
    assert 0.02 < counts[-12168 - 4000: -12168].mean() < 0.98             # the random pairs take both ways


# ---------------------------------------------------------------------------- the reference against geometry
def test_the_regions_of_a_triangle():
    for p, want in REGIONS:
        for tri in ((A, B, C), (B, C, A), (C, A, B), (A, C, B)):
            assert float(mref.d2(np.array(p), *tri)) == want, (p, want)
    best, nearest = mref.brute([p for p, _ in REGIONS], np.stack([A, B, C]), [[0, 1, 2], [0, 1, 2]])
    assert best.tolist() == [w for _, w in REGIONS] and (nearest == 0).all()


def test_a_common_integer_shift_changes_nothing():
    p, a, b, c = random_pairs(2000, seed=6)                              # multiples of 1/1024 below 64: every sum below is exact
    want = mref.d2(p, a, b, c)
    rng = np.random.default_rng(7)
    for _ in range(3):
        s = rng.integers(-100000, 100001, 3).astype(np.float64)
        assert mref.d2(p + s, a + s, b + s, c + s).tobytes() == want.tobytes()


def test_a_degenerate_triangle_is_its_segment_or_its_point():
    for kind, (a, b, c) in DEGENERATE:
        counts, _ = mref.face(np.array(DEGENERATE_POINTS), a, b, c)
        assert not counts.any()                                          # n is exactly zero: no face term
        for p in DEGENERATE_POINTS:
            p = np.array(p)
            got = float(mref.d2(p, a, b, c))
            if kind == "all equal":
                assert got == float(mref.dot(p - a, p - a))
                continue
            # exactly the least of the rule's own segment terms, and the segment U V_ up to the spelling (which corner a
            # segment starts from moves the last bits)
            parts = [float(mref.seg(p, x, y)) for x, y in ((a, b), (b, c), (c, a))]
            assert got == min(parts)
            np.testing.assert_allclose(got, float(mref.seg(p, U, V_)), rtol=1e-14, atol=1e-14)
    assert float(mref.d2(M_, U, M_, V_)) == 0.0 and float(mref.d2(np.array([9.0, 6.0, 11.0]), U, M_, V_)) == 16.0 + 4.0 + 16.0


def test_relabelling_the_corners_moves_the_value_within_rounding():
    """The bound: with S the largest coordinate difference among p, a, b, c, every intermediate vector has components of at most
    S (2 S^2 for n) with an absolute error of a few eps S (eps S^2).  An edge term r.r then carries at most about 30 eps S^2.
    The face term dn dn / nn carries 2 |dn| err(dn) / nn + dn^2 err(nn) / nn^2 with |dn| <= 4 S^3, err(dn) <= 20 eps S^3 and
    err(nn) <= 40 eps S^4: for nn >= 2^-10 S^4 that is below 2^19 eps S^2.  Where rounding turns a side test for one labelling
    and not for another, the foot of p lies within rounding of that side and the two terms differ by less again.  Hence
    |d2 - d2'| <= 2^20 eps S^2 = 2^-32 S^2 for triangles with nn >= 2^-10 S^4; the slivers among the random pairs are left out."""
    p, a, b, c = random_pairs(4000, seed=8)
    S = np.max([np.abs(x - y).max(1) for x in (p, a, b, c) for y in (a, b, c)], 0)
    n = mref.cross(b - a, c - a)
    fair = mref.dot(n, n) >= 2.0 ** -10 * S ** 4
    assert fair.sum() > 3000
    want = mref.d2(p, a, b, c)
    worst = 0.0
    for x, y, z in ((b, c, a), (c, a, b), (a, c, b), (c, b, a), (b, a, c)):
        diff = np.abs(mref.d2(p, x, y, z) - want)[fair] / (S[fair] ** 2)
        worst = max(worst, float(diff.max()))
    print("largest |d2 - d2'| / S^2 = 2^%.1f" % np.log2(max(worst, 1e-300)))
    assert worst <= 2.0 ** -32


def test_brute_force_gate_and_ties():
    v = np.stack([A, B, C, A + [0, 0, 2.0], B + [0, 0, 2.0], C + [0, 0, 2.0]])           # the triangle and a copy 2 above
    t = np.array([[3, 4, 5], [0, 1, 2]])
    p = np.array([[1.0, 1.0, 2.0], [1.0, 1.0, 1.5], [1.0, 1.0, 9.0], [1.0, 1.0, 6.0]])
    best, nearest = mref.brute(p, v, t)
    assert best.tolist() == [1.0, 0.25, 36.0, 9.0] and nearest.tolist() == [0, 1, 0, 0]     # the tie goes to the smaller index
    best, nearest = mref.brute(p, v, t, max_dist=3.0)
    assert best.tolist() == [1.0, 0.25, np.inf, 9.0] and nearest.tolist() == [0, 1, -1, 0]  # best == max_dist^2 is not far
    assert mref.figures(best) == (4, 1, (1.0 + 0.25 + 9.0) / 3, 9.0)
    n, far, mse, top = mref.figures(np.full(3, np.inf))
    assert (n, far) == (3, 3) and np.isnan(mse) and np.isnan(top)


# ---------------------------------------------------------------------------- the choice of the cell edge
# cell: (triangles, pairs at h = 1, 2, 4, the chosen edge): the reference's own figures
EDGES = {None: (12168, (36182, 21793, 16313), 1), 2: (912, (13786, 4112, 2154), 1), 4: (240, (13742, 3331, 1266), 2),
         16: (12, (7226, 1452, 312), 4)}


@pytest.mark.parametrize("cell", [None, 2, 4, 16])
def test_the_chosen_edge_on_the_golden_sphere(cell):
    _, v, t = sphere() if cell is None else (None,) + simplified(cell)
    n_triangles, pairs, edge = EDGES[cell]
    assert len(t) == n_triangles
    assert tuple(mref.pair_count(v, t, h) for h in (1.0, 2.0, 4.0)) == pairs
    lo, hi = mref.bounds(v, t)
    tried = []

    def count(cells):
        tried.append(cells[0])
        assert cells[4] <= 1024 and cells[1:4] == tuple(int(x) for x in np.floor(lo / cells[0]))
        return mref.pair_count(v, t, cells[0])
    cells, got = metrics.choose_mesh_cells(lo, hi, len(t), count)
    assert cells[0] == edge and got == pairs[int(np.log2(edge))] and got <= 32 * len(t)
    assert tried == [2.0 ** k for k in range(int(np.log2(edge)) + 1)]     # one count per edge tried, doubling
    forced, got = metrics.choose_mesh_cells(lo, hi, len(t), count, edge=8)
    assert forced[0] == 8.0 and got == mref.pair_count(v, t, 8.0)
    for bad in (0.5, 3, 0, 2.0 ** 21):
        with pytest.raises(ValueError, match="power of two"):
            metrics.choose_mesh_cells(lo, hi, len(t), count, edge=bad)


def test_the_first_edge_fits_the_grid_and_the_doubling_ends():
    lo, hi = np.array([-3000.5, 0.0, 10.0]), np.array([5000.25, 1.0, 11.0])
    assert metrics.mesh_first_edge(lo, hi) == 8.0                         # 8001 cells of edge 1, 1001 of edge 8
    assert metrics.mesh_cells(lo, hi, 8.0) == (8.0, -376, 0, 1, 1002)
    # one triangle across the whole box is listed in every cell: the edge doubles until 32 cells or fewer are left
    calls = []
    cells, pairs = metrics.choose_mesh_cells(np.zeros(3), np.full(3, 100.0), 1, lambda c: calls.append(c) or c[4] ** 3)
    assert cells == (64.0, 0, 0, 0, 2) and pairs == 8 and len(calls) == 7


# ---------------------------------------------------------------------------- arguments and text
def test_the_summary_gains_a_line_with_error():
    report = dict(voxels=1954, components=1, rounds=19, vertices=122, triangles=240, boundary_edges=0)
    first = "surface: 1954 voxels, 1 components, 19 rounds, 122 vertices, 240 triangles, 0 boundary edges"
    assert surface.summary_line(report) == first
    error = {"points": 1954, "far": 0, "mse (p2mesh)": 0.179776, "rms (p2mesh)": 0.424, "h. (p2mesh)": 1.055 ** 2, "edge": 2, "pairs": 3331}
    report["error"] = error
    last = "error: rms 0.424, max 1.055 voxels over 1954 points (cell edge 2, 3331 pairs)"
    assert surface.summary_line(report) == first + "\n" + last
    report["simplify"] = dict(cell=4, clusters=122, vertices_in=6086, triangles_in=12168, degenerate=11928, cancelled=0, merged=0, folded=0,
                              fallback=9, unused=0)
    lines = surface.summary_line(report).split("\n")
    assert len(lines) == 3 and lines[0] == first and lines[1].startswith("simplify: cell 4") and lines[2] == last
    del report["error"]
    assert surface.summary_line(report).split("\n") == lines[:2]


def test_argument_errors_come_before_any_file_is_read(capsys):
    base = ["--cloud", "no_such.ply", "--mesh", "no_such.obj"]
    for extra, said in ((["--max_dist", "0"], "max_dist"), (["--max_dist", "-1.5"], "max_dist"), (["--max_dist", "inf"], "max_dist"),
                        (["--max_dist", "nan"], "max_dist"), (["--samples", "-3"], "--samples"), (["--render", "x.jpg"], ".png"),
                        (["--render", "x.png", "--vmax", "0"], "--vmax"), (["--render", "x.png", "--size", "0", "10"], "--size")):
        with pytest.raises(SystemExit):
            cli.main(base + extra)
        assert said in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.main(["--cloud", "no_such.ply", "--mesh", "no_such.stl"])
    assert ".obj or .off" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.main(["--cloud", "no_such.ply"])
    assert "--mesh" in capsys.readouterr().err
    args = cli.parse_args(base + ["--max_dist", "2.5", "--samples", "100", "--seed", "3"])
    assert (args.max_dist, args.samples, args.seed, args.render, args.vmax, tuple(args.size)) == (2.5, 100, 3, "", 2.0, (1024, 1024))
    assert surface.parse_args(["--input", "a.ply", "--output", "a.obj", "--simplify", "4", "--error"]).error is True
    assert surface.parse_args(["--input", "a.ply", "--output", "a.obj"]).error is False
    for bad in (0, -1.0, float("inf"), float("nan"), True):
        with pytest.raises(ValueError, match="max_dist"):
            metrics.check_max_dist(bad)
    assert metrics.check_max_dist(None) == float("inf") and metrics.check_max_dist(2) == 2.0


def test_the_printed_figures_and_the_frame():
    from pcgcv1_amd.ingest import Frame, apply_frame
    figures = {"points": 10, "far": 2, "mse (p2mesh)": 0.25, "rms (p2mesh)": 0.5, "h. (p2mesh)": 4.0, "edge": 1, "pairs": 77}
    lines = cli.figure_lines(figures)
    assert lines[0] == "points: 10, of them far: 2" and lines[1] == "cloud to mesh: rms 0.5 voxels, max 2 voxels over 8 points"
    assert lines[-1] == "search: cell edge 1, 77 pairs" and len(lines) == 4
    assert cli.figure_lines(figures, step=0.01)[1] == "cloud to mesh: rms 0.5 voxels = 0.005 in scan units, max 2 voxels = 0.02 in scan units over 8 points"
    figures.update({"mse (mesh2p)": 1.0, "h. (mesh2p)": 9.0, "h. (sym)": 9.0})
    assert len(cli.figure_lines(figures)) == 6 and cli.figure_lines(figures)[3] == "mesh to cloud: rms 1 voxels, max 3 voxels"
    frame = Frame((-1.5, 2.0, 0.25), 0.125, 6)                            # a power-of-two step: the round trip is exact
    q = np.array([[0.0, 1.5, 63.25], [10.0, 20.0, 30.0]])
    assert cli.unapply_frame(apply_frame(q, frame), frame).tobytes() == q.tobytes()
