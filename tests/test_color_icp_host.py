"""The colour metric of the registration without a device: the gradient rule and the loop of tests/_color_icp_ref.py on the
three fixtures (DESIGN.md §7k records their figures), and the host side of pcgcv1_amd/register.py: the joint solve and the
argument errors, which are raised before any device work."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _color_icp_ref as ref                                             # noqa: E402
import _register_ref as rr                                               # noqa: E402
from pcgcv1_amd import register                                          # noqa: E402

# the reference loop as DESIGN.md §7k records it (weight 0.9, radius 3, kmin 6, gates 4, 2, 1): truth error in voxels, steps
RECORDED = {"flat": (0.00433, [4, 1, 1]), "sphere": (0.00456, [5, 2, 3]), "bumpy": (0.01866, [7, 4, 3])}


# ---------------------------------------------------------------------------- the gradient rule
def test_a_linear_ramp_gives_its_tangential_gradient():
    """Y = 1000 x + 2000 y + 100000 on the lattice plane z = x / 2 + y / 4: every offset and every intensity is exact, so the
    fit is the ramp's gradient less its part along the normal, to the 6e-8 by which the float32 normal misses the plane"""
    x, y = (a.reshape(-1) for a in np.meshgrid(np.arange(21) * 0.5, np.arange(21) * 0.5, indexing="ij"))
    g = np.stack([x, y, 0.5 * x + 0.25 * y], 1).astype(np.float32)
    Y = (1000.0 * x + 2000.0 * y + 100000.0).astype(np.int32)
    assert np.array_equal(Y, 1000.0 * x + 2000.0 * y + 100000.0)
    n = np.array([-0.5, -0.25, 1.0]) / np.sqrt(1.3125)
    grad, valid, K, _, _ = ref.gradient(g, np.tile(n, (len(g), 1)).astype(np.float32), Y, 1.5, 6)
    G = np.array([1000.0, 2000.0, 0.0]) / ref.Y_MAX
    want = G - (G @ n) * n
    assert valid.all() and K.min() >= 6
    assert np.abs(grad - want).max() < 1e-9
    assert np.abs(grad @ n).max() < 1e-9                       # in the tangent plane


def _five():
    """a centre with four neighbours in its plane, K = 5 for the centre"""
    g = np.array([[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0]], np.float32)
    return g, np.tile(np.array([0, 0, 1], np.float32), (5, 1)), np.array([1000, 3000, 500, 2000, 100], np.int32)


def test_kmin_is_the_first_count_with_a_gradient():
    g, n, Y = _five()
    grad, valid, K, _, _ = ref.gradient(g, n, Y, 1.25, 5)
    assert K.tolist() == [5, 2, 2, 2, 2] and valid.tolist() == [1, 0, 0, 0, 0]
    assert np.allclose(grad[0] * ref.Y_MAX, [1250.0, 950.0, 0.0], rtol=1e-12, atol=0) and not grad[1:].any()
    assert not ref.gradient(g, n, Y, 1.25, 6)[1].any()          # K = kmin - 1


def test_collinear_neighbours_and_a_zero_normal_have_no_gradient():
    line = np.zeros((9, 3), np.float32)
    line[:, 0] = np.arange(9) * 0.5
    up = np.tile(np.array([0, 0, 1], np.float32), (9, 1))
    grad, valid, K, _, _ = ref.gradient(line, up, np.arange(9, dtype=np.int32) * 1000, 2.0, 3)
    assert K.min() >= 5 and not valid.any() and not grad.any()
    g, n, Y = _five()
    for bad in ([0, 0, 0], [np.nan, 0, 1], [0, np.inf, 0]):
        nb = n.copy()
        nb[0] = bad
        grad, valid = ref.gradient(g, nb, Y, 1.25, 5)[:2]
        assert not valid.any() and not grad.any()


def test_intensity_is_bt709_in_integers():
    col = np.array([[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255], [12, 34, 56]], np.uint8)
    want = [0, 2550000, 2126 * 255, 7152 * 255, 722 * 255, 2126 * 12 + 7152 * 34 + 722 * 56]
    assert ref.intensity(col).tolist() == want and register.intensity(col, 6, "source").tolist() == want
    assert register.intensity(col.astype(np.float64), 6, "source").dtype == np.int32
    for bad in (col.astype(np.float64) + 0.5, col.astype(np.int32) - 1, col.astype(np.int32) + 1, np.full((6, 3), np.nan)):
        with pytest.raises(ValueError, match="whole numbers in 0..255"):
            register.intensity(bad, 6, "source")


# ---------------------------------------------------------------------------- the step and the solve
def test_the_tree_search_of_the_reference_step_equals_brute_force():
    d = ref.fixture("bumpy")
    Yp, Yq = ref.intensity(d["source_colors"]), ref.intensity(d["target_colors"])
    unit = ref.unit_normals(d["target_normals"])
    grad, valid = ref.gradient(d["target"], unit, Yq, 3.0, 70)[:2]
    assert 0.05 < valid.mean() < 0.95                          # a kmin about the mean count: some pairs have a gradient, some none
    c = np.array([16.0, 16.0, 16.0])
    a = ref.step(d["source"], Yp, d["target"], unit, Yq, grad, valid, np.eye(3), np.zeros(3), c, 2.0, brute=True)
    b = ref.step(d["source"], Yp, d["target"], unit, Yq, grad, valid, np.eye(3), np.zeros(3), c, 2.0, brute=False)
    assert all(a[k].tobytes() == b[k].tobytes() for k in ("S", "abs", "terms", "best", "ties")) and a["S"][0] > 100
    # the geometric block is the point-to-plane block of the plain step, term for term
    plain = rr.step(d["source"], d["target"], unit, np.eye(3), np.zeros(3), c, 2.0)
    assert a["S"][0] == plain["S"][0] and a["S"][1] == plain["S"][1] and np.array_equal(a["S"][2:30], plain["S"][17:45])
    assert a["S"][30] <= a["S"][0] and a["S"][58] > 0


def test_solve_color_mixes_the_two_systems_and_rejects_the_ends():
    rng = np.random.default_rng(3)
    S = np.zeros(59)
    for block in (2, 31):
        J = rng.normal(size=(40, 6))
        r = rng.normal(size=40) * 0.1
        S[block:block + 21] = (J.T @ J)[np.triu_indices(6)]
        S[block + 21:block + 27] = J.T @ r
        S[block + 27] = r @ r
    S[0], S[30] = 40, 40
    for lam in (0.1, 0.5, 0.9):
        A, g = register.color_system(S, lam)
        Ag, gg = rr.plane_system(np.concatenate([np.zeros(17), S[2:30]]))
        Ac, gc = rr.plane_system(np.concatenate([np.zeros(17), S[31:59]]))
        assert np.allclose(A, (1 - lam) * Ag + lam * Ac, rtol=1e-15) and np.allclose(g, (1 - lam) * gg + lam * gc, rtol=1e-15)
        dR, dt = register.solve_color(S, lam)
        wR, wt = ref.solve_color(S, lam)
        assert np.array_equal(dR, wR) and np.array_equal(dt, wt)
        assert np.allclose(dR @ dR.T, np.eye(3), atol=1e-14)  # the exact rotation
    for lam in (0.0, 1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="color_weight must lie strictly between 0 and 1"):
            register.solve_color(S, lam)
    flat = S.copy()
    flat[31:59] = 0.0
    flat[2:23] = 0.0
    flat[2] = 1.0                                              # one motion fixed of six
    with pytest.raises(ValueError, match="joint point-to-plane and colour system is singular"):
        register.solve_color(flat, 0.9)


# ---------------------------------------------------------------------------- argument errors, before any device work
def test_argument_errors_come_before_any_work():
    d = ref.fixture("bumpy")
    s, t, n, cs, ct = d["source"], d["target"], d["target_normals"], d["source_colors"], d["target_colors"]
    assert register.MIN_PAIRS["color"] == 6
    with pytest.raises(ValueError, match="metric must be"):
        register.icp(s, t, n, metric="colour", source_colors=cs, target_colors=ct)
    with pytest.raises(ValueError, match="metric='color' needs the target's normals"):
        register.icp(s, t, None, metric="color", source_colors=cs, target_colors=ct)
    for kw, what in ((dict(target_colors=ct), "source_colors is missing"), (dict(source_colors=cs), "target_colors is missing"),
                     (dict(), "both are missing")):
        with pytest.raises(ValueError, match=what):
            register.icp(s, t, n, metric="color", **kw)
    with pytest.raises(ValueError, match=r"%d source colours for %d source points" % (len(s) - 1, len(s))):
        register.icp(s, t, n, metric="color", source_colors=cs[:-1], target_colors=ct)
    with pytest.raises(ValueError, match=r"%d target colours for %d target points" % (len(t) + 1, len(t))):
        register.icp(s, t, n, metric="color", source_colors=cs, target_colors=np.concatenate([ct, ct[:1]]))
    for kw, what in ((dict(color_weight=0.0), "color_weight"), (dict(color_weight=1.0), "color_weight"),
                     (dict(color_weight=float("nan")), "color_weight"), (dict(color_radius=0.0), "color_radius"),
                     (dict(color_radius=16.5), "color_radius"), (dict(color_kmin=2), "color_kmin"), (dict(color_kmin=2 ** 20 + 1), "color_kmin")):
        with pytest.raises(ValueError, match=what):
            register.icp(s, t, n, metric="color", source_colors=cs, target_colors=ct, **kw)
    scans = [(s.astype(np.float64), cs, None), (t.astype(np.float64), None, None)]
    with pytest.raises(ValueError, match="metric='color' needs the colours of every scan, and scan 1 has none"):
        register.register_scans(scans, bits=8, metric="color", estimate_normals=True)
    with pytest.raises(ValueError, match="metric='color' needs the target's normals"):
        register.register_scans([scans[0], (t.astype(np.float64), ct, None)], bits=8, metric="color")


def test_the_command_line_refuses_colourless_scans_before_parsing_them(tmp_path, capsys):
    """the headers alone decide: the bodies are not ply data at all"""
    names = []
    for k, props in enumerate(("property uchar red\nproperty uchar green\nproperty uchar blue\n", "")):
        names.append(str(tmp_path / ("scan%d.ply" % k)))
        with open(names[-1], "w") as f:
            f.write("ply\nformat ascii 1.0\nelement vertex 2\nproperty float x\nproperty float y\nproperty float z\n" + props +
                    "end_header\nthis is not a vertex\n")
    assert register._ply_has_colors(names[0]) and not register._ply_has_colors(names[1]) and not register._ply_has_colors(str(tmp_path / "none.ply"))
    common = ["--output", str(tmp_path / "out.ply"), "--bits", "8", "--estimate_normals", "--metric", "color"]
    with pytest.raises(SystemExit):
        register.parse_args(["--input"] + names + common)
    assert "--metric=color needs colours: %s has no red green blue" % names[1] in capsys.readouterr().err
    for flag, value in (("--color_weight", "1"), ("--color_radius", "17"), ("--color_kmin", "2")):
        with pytest.raises(SystemExit):
            register.parse_args(["--input", names[0], names[0]] + common + [flag, value])
        assert flag in capsys.readouterr().err
    args = register.parse_args(["--input", names[0], names[0]] + common)
    assert (args.metric, args.color_weight, args.color_radius, args.color_kmin) == ("color", 0.9, 3.0, 6)


# ---------------------------------------------------------------------------- the reference loop on the fixtures
@pytest.mark.parametrize("name", sorted(RECORDED))
def test_the_reference_loop_finds_the_truth_with_colour(name):
    """within twice the error DESIGN.md §7k records for it; the margin covers nothing but a later reseeding"""
    d = ref.fixture(name)
    r = ref.reference_loop(name)
    err = ref.truth_error(r, d)
    print("%s: truth error %.5f voxel, steps %s, colour rmse %.4f, colour fitness %.3f" % (name, err, r["iterations"], r["color_rmse"],
                                                                                         r["color_fitness"]))
    assert r["converged"] and err <= 2.0 * RECORDED[name][0]
    assert r["iterations"] == RECORDED[name][1]


def test_geometry_alone_is_singular_on_the_flat_square():
    d = ref.fixture("flat")
    with pytest.raises(ValueError, match="degenerate"):
        ref.icp(d["source"], d["source_colors"], d["target"], d["target_normals"], d["target_colors"], weight=None)
    with pytest.raises(ValueError, match="degenerate"):       # and so says the plain reference loop
        rr.icp(d["source"][:500], d["target"][:500], ref.unit_normals(d["target_normals"][:500]), "plane")


def test_geometry_alone_leaves_the_sphere_turned():
    """10 steps per stage, not 50: no stage ends by the stopping rule either way (50 steps: 2.12 voxels off)"""
    d = ref.fixture("sphere")
    r = ref.icp(d["source"], d["source_colors"], d["target"], d["target_normals"], d["target_colors"], weight=None, iters=10)
    err = ref.truth_error(r, d)
    print("sphere, geometry only: truth error %.3f voxel, steps %s" % (err, r["iterations"]))
    assert err >= 1.0 and not r["converged"]
