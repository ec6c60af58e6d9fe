"""The host side of the plane filter (pcgcv1_amd/clean.py: plane:D[:FRAC[:DRAWS[:SEED]]]): the spec strings, the integer form of
the distance test against Python's big integers, the host steps of the rule (clean.draw_planes, clean.refit_plane) against
their restatement in tests/_plane_ref.py and cases worked out by hand, the rule itself on a table with a sphere on it, and what
the three command lines accept and refuse.  No GPU."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _plane_ref as ref                                                 # noqa: E402
from pcgcv1_amd import clean, ingest                                     # noqa: E402
from pcgcv1_amd import test as cli                                       # noqa: E402


# ---------------------------------------------------------------------------- parsing
def test_parse_spec_defaults_and_fields():
    s = clean.parse_spec("plane:1.5")
    assert (s.kind, s.dist2, s.frac, s.draws, s.seed, s.text) == ("plane", 3, 0.05, 1024, 0, "plane:1.5") and repr(s) == "Spec('plane:1.5')"
    s = clean.parse_spec("plane:0.5:1:65536:2147483647")
    assert (s.dist2, s.frac, s.draws, s.seed) == (1, 1.0, 65536, 2 ** 31 - 1)
    s = clean.parse_spec("plane:32:0.9:1")
    assert (s.dist2, s.frac, s.draws, s.seed) == (64, 0.9, 1, 0) and clean.parse_spec(s) is s
    assert clean.parse_spec("plane:4:0.25").dist2 == 8 and clean.parse_spec("plane:4:0.25").frac == 0.25
    assert clean.parse_spec("plane:1.5") == clean.parse_spec("plane:1.50:0.05:1024:0")
    for other in ("plane:2", "plane:1.5:0.06", "plane:1.5:0.05:1023", "plane:1.5:0.05:1024:1"):
        assert clean.parse_spec("plane:1.5") != clean.parse_spec(other)
    assert ref.parse_spec("plane:1.5") == ("plane", 3, 0.05, 1024, 0) and ref.parse_spec("plane:4:0.9:7:3") == ("plane", 8, 0.9, 7, 3)
    # the new fields come last and have defaults: the older kinds are built and compared as before
    old = clean.Spec("stat", 8, 20, 2.0, 0, "stat:20:2.0")
    assert old == clean.parse_spec("stat:20:2.0") and (old.gap, old.dist2, old.frac, old.draws, old.seed) == (1, 0, 0.05, 1024, 0)
    assert clean.parse_specs(["stat:20:2.0", "plane:1.5", "largest:2"])[1].kind == "plane"


@pytest.mark.parametrize("text, field", [
    ("plane", "fields"), ("plane:1:0.1:5:0:9", "fields"),
    ("plane:0.7", "D = '0.7'"), ("plane:0", "D = '0'"), ("plane:32.5", "D = '32.5'"), ("plane:-1", "D = '-1'"), ("plane:x", "D = 'x'"),
    ("plane:nan", "D = 'nan'"), ("plane:inf", "D = 'inf'"), ("plane:0.25", "D = '0.25'"),
    ("plane:1:0", "FRAC = '0'"), ("plane:1:1.01", "FRAC = '1.01'"), ("plane:1:-0.1", "FRAC = '-0.1'"), ("plane:1:nan", "FRAC = 'nan'"),
    ("plane:1:half", "FRAC = 'half'"),
    ("plane:1:0.1:0", "DRAWS = 0"), ("plane:1:0.1:65537", "DRAWS = 65537"), ("plane:1:0.1:1.5", "DRAWS = '1.5'"),
    ("plane:1:0.1:5:-1", "SEED = -1"), ("plane:1:0.1:5:%d" % 2 ** 31, "SEED = %d" % 2 ** 31), ("plane:1:0.1:5:x", "SEED = 'x'"),
])
def test_parse_spec_refuses(text, field):
    with pytest.raises(ValueError) as e:
        clean.parse_spec(text)
    assert field in str(e.value) and "--clean " + text in str(e.value)


def test_an_unknown_kind_names_all_five():
    with pytest.raises(ValueError) as e:
        clean.parse_spec("planes:1.5")
    for word in ("neither", "'radius'", "'stat'", "'component'", "'largest'", "'plane'", "--clean planes:1.5"):
        assert word in str(e.value)


# ---------------------------------------------------------------------------- the threshold form
def test_the_threshold_form_is_the_rule():
    """10 000 triples at bits = 12 among 64 points that hold the grid's eight corners, D2 from 1 to 64: |s| <= isqrt(D2^2 nn) // 2
    against 4 s^2 <= D2^2 nn in Python's integers, for a point anywhere, the points nearest the plane above and below it, and a
    corner; every intermediate inside the bounds include/pcgc.h states"""
    rng = np.random.default_rng(12)
    corners = np.stack(np.meshgrid(*[[0, 4095]] * 3, indexing="ij"), -1).reshape(-1, 3)
    cloud = np.r_[corners, rng.integers(0, 4096, (56, 3))]
    n_draws, seen_true, seen_false = 2500, 0, 0
    for D2 in (1, 64, 3, 17):
        planes = clean.draw_planes(lambda rows: cloud[rows], D2, n_draws, D2, len(cloud))
        assert planes.dtype == np.int64 and planes.shape == (n_draws, 5)
        np.testing.assert_array_equal(planes, ref.draw_planes(cloud, D2, n_draws, D2))
        tri = np.random.default_rng(D2).integers(0, len(cloud), (n_draws, 3))
        where = rng.integers(0, 4096, (n_draws, 3))
        for h in range(n_draws):
            a, b, c, d, T = [int(v) for v in planes[h]]
            nn = a * a + b * b + c * c
            p0, p1, p2 = [[int(v) for v in cloud[i]] for i in tri[h]]
            u, v = [p1[k] - p0[k] for k in range(3)], [p2[k] - p0[k] for k in range(3)]
            assert (a, b, c) == (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])
            assert d == a * p0[0] + b * p0[1] + c * p0[2]
            if nn == 0:
                assert T == -1
                continue
            assert max(abs(a), abs(b), abs(c)) < 2 ** 26 and nn < 2 ** 52 and D2 * D2 * nn < 2 ** 64
            assert T == math.isqrt(D2 * D2 * nn) // 2 and 0 <= T < 2 ** 31
            assert 4 * T * T <= D2 * D2 * nn < 4 * (T + 1) * (T + 1)     # the last s inside and the first outside
            x, y, z = [int(w) for w in where[h]]
            tests = [(x, y, z), tuple(int(w) for w in corners[h % 8])]
            if c:                                                        # the cells of column (x, y) around the plane
                z0 = (d - a * x - b * y) // c
                tests += [(x, y, min(4095, max(0, z0 + k))) for k in (-D2, -1, 0, 1, 2, D2)]
            for q in tests:
                s = a * q[0] + b * q[1] + c * q[2] - d
                assert abs(s) < 2 ** 40
                assert (abs(s) <= T) == (4 * s * s <= D2 * D2 * nn)
                seen_true += abs(s) <= T
                seen_false += abs(s) > T
    assert seen_true > 5000 and seen_false > 5000


def test_plane_threshold_at_exact_squares():
    # |n| = 5, D2 = 3: 2 |s| <= 15, so |s| <= 7; D2 = 2: |s| <= 5 exactly
    assert clean.plane_threshold(3, 25) == 7 and clean.plane_threshold(2, 25) == 5 and clean.plane_threshold(1, 25) == 2
    assert clean.plane_threshold(1, 1) == 0 and clean.plane_threshold(64, 2 ** 52 - 1) < 2 ** 31
    assert [ref.threshold(D2, nn) for D2, nn in ((3, 25), (2, 25), (1, 1))] == [7, 5, 0]


# ---------------------------------------------------------------------------- an exact plane
@pytest.mark.parametrize("axes", [(0, 1, 2), (2, 0, 1), (1, 2, 0), (0, 2, 1)])
def test_an_exact_plane(axes):
    """bits = 6: every cell of z = 7 and a hundred of z = 8, the axes permuted"""
    rng = np.random.default_rng(7)
    flat = np.stack(np.meshgrid(np.arange(64), np.arange(64), indexing="ij"), -1).reshape(-1, 2)
    above = flat[rng.permutation(len(flat))[:100]]
    cloud = np.r_[np.c_[flat, np.full(len(flat), 7)], np.c_[above, np.full(100, 8)]][:, list(axes)]
    on = np.r_[np.ones(len(flat), bool), np.zeros(100, bool)]
    up = axes.index(2)                                                   # the column that holds the 7s
    # any non-degenerate draw from the plane counts all of it, and at D = 0.5 nothing of the layer above
    planes = clean.draw_planes(lambda rows: cloud[:4096][rows], 1, 64, 3, 4096)
    np.testing.assert_array_equal(planes, ref.draw_planes(cloud[:4096], 1, 64, 3))
    live = planes[:, 4] >= 0
    assert live.sum() > 50 and (planes[live][:, [k for k in range(3) if k != up]] == 0).all()
    score = ref.counts(cloud, 6, planes)
    assert (score[live] == 4096).all() and (score[~live] == 0).all()
    np.testing.assert_array_equal(ref.inliers(cloud, 6, planes[live][0]), on)
    # at D = 1 the layer above is within reach
    assert (ref.counts(cloud, 6, clean.draw_planes(lambda rows: cloud[:4096][rows], 2, 64, 3, 4096))[live] == 4196).all()
    # the refit of the exact plane is the exact plane
    ten = ref.sums(cloud, on)
    assert ten[0] == 4096 and ten[1 + up] == 7 * 4096 and ten[4 + up] == 49 * 4096
    plane, nq = ref.refit(ten, 1)
    assert [abs(v) for v in nq] == [65536 if k == up else 0 for k in range(3)]
    np.testing.assert_array_equal(clean.refit_plane(ten, 1), plane)
    assert abs(int(plane[up])) == 4096 * 65536 and abs(int(plane[3])) == 65536 * 7 * 4096 and plane[4] == 4096 * 65536 // 2
    np.testing.assert_array_equal(ref.inliers(cloud, 6, plane), on)
    # the whole rule, drawing from all the rows
    found, mask, info = ref.segment(cloud, 6, 1, 0.05, 256, 0)
    np.testing.assert_array_equal(mask, on)
    assert info == dict(n=4196, draws=256, best_count=4096, count=4096, dropped=True)
    np.testing.assert_array_equal(ref.keep_mask(cloud, 6, "plane:0.5:0.05:256"), ~on)
    assert ref.keep_mask(cloud, 6, "plane:0.5:0.98:256").all()          # 4096 of 4196 is less than 0.98


def test_sums_by_hand():
    p = np.array([[1, 2, 3], [4, 5, 6], [9, 9, 9]])
    assert ref.sums(p, [True, True, False]).tolist() == [2, 5, 7, 9, 17, 29, 45, 22, 27, 36]


# ---------------------------------------------------------------------------- degenerate draws
def test_degenerate_draws_score_nothing():
    line = np.arange(20)[:, None] * np.array([1, 2, 3])                 # collinear, bits = 6
    for cloud in (line, line[:2], line[:1]):
        planes = clean.draw_planes(lambda rows: cloud[rows], 3, 128, 5, len(cloud))
        np.testing.assert_array_equal(planes, ref.draw_planes(cloud, 3, 128, 5))
        assert (planes[:, 4] == -1).all() and (planes[:, :3] == 0).all()
        assert (ref.counts(cloud, 6, planes) == 0).all()
        plane, mask, info = ref.segment(cloud, 6, 3, 0.05, 128, 5)
        assert plane is None and not mask.any() and info == dict(n=len(cloud), draws=128, best_count=0, count=0, dropped=False)
        assert ref.keep_mask(cloud, 6, "plane:1.5:0.05:128:5").all()
    # a repeated row among three that span a plane otherwise
    cloud = np.array([[0, 0, 0], [5, 0, 0], [0, 5, 0]])
    planes = ref.draw_planes(cloud, 3, 200, 1)
    tri = np.random.default_rng(1).integers(0, 3, (200, 3))
    repeated = np.array([len(set(t)) < 3 for t in tri.tolist()])
    assert 0 < repeated.sum() < 200
    np.testing.assert_array_equal(planes[:, 4] == -1, repeated)
    assert (np.abs(planes[~repeated][:, 2]) == 25).all() and (ref.counts(cloud, 6, planes)[~repeated] == 3).all()
    # T = -1 matches nothing, not even a point with s == 0; nor does anything match outside the grid
    assert not ref.inliers(cloud, 6, [0, 0, 0, 0, -1]).any()
    assert ref.inliers(np.array([[1, 1, 0], [64, 1, 0], [1, -1, 0]]), 6, [0, 0, 1, 0, 0]).tolist() == [True, False, False]


# ---------------------------------------------------------------------------- the scene
@pytest.fixture(scope="module")
def scene():
    vox, is_table = ref.scene()
    assert (len(vox), int(is_table.sum())) == (ref.SCENE_VOXELS, ref.SCENE_TABLE) == (41014, 27247)
    assert vox.dtype == np.int32 and len(np.unique(vox, axis=0)) == len(vox) and vox.min() >= 0 and vox.max() < 128
    return vox, is_table


def test_the_rule_takes_the_table_and_leaves_the_object(scene):
    """conditions on the rule, not tolerances on the device: the rule gives 0.986 and 0.007, then 0.993 and 19 of 27 247 voxels"""
    vox, is_table = scene
    keep = ref.keep_mask(vox, 7, "plane:1.5:0.05:256:0")
    assert (~keep)[is_table].mean() >= 0.98 and (~keep)[~is_table].mean() <= 0.02
    both = ref.keep_mask_all(vox, 7, ["plane:1.5:0.05:256:0", "largest"])
    assert both[~is_table].mean() >= 0.98 and both[is_table].mean() <= 0.005
    assert not (both & ~keep).any()
    # what the four older kinds do with it: the table is dense and touches the object
    assert ref.keep_mask(vox, 7, "largest")[is_table].mean() > 0.99
    # the plane that was found is the table: slopes 0.13 and -0.21, height 0.3 * 128 at the centre (a voxel's coordinate is
    # half a cell below its samples' mean)
    plane, mask, info = ref.segment(vox, 7, 3, 0.05, 256, 0)
    a, b, c, d = [int(v) for v in plane[:4]]
    assert abs(-a / c - 0.13) < 0.005 and abs(-b / c + 0.21) < 0.005 and abs((d - 64 * a - 64 * b) / c + 0.5 - 38.4) < 0.25
    assert info["dropped"] and info["count"] == mask.sum() >= info["best_count"] > 0.9 * is_table.sum()
    # a bound no plane of this scene meets: everything stays
    assert ref.keep_mask(vox, 7, "plane:4:0.9").all()


def test_largest_on_the_dense_grid_is_the_component_rule():
    import _components_ref as components_ref
    p = components_ref.surface()
    for cloud in (p, p[:1500]):
        np.testing.assert_array_equal(ref.largest_mask(cloud, 6), components_ref.keep_mask(cloud, 6, "largest"))


# ---------------------------------------------------------------------------- the report line
def test_plane_line():
    spec = clean.parse_spec("plane:1.5:0.05:256")
    info = dict(n=1000, draws=256, best_count=380, count=400, dropped=True)
    assert clean.plane_line(spec, np.array([0, 0, -20, -140, 30]), info) == (
        "plane: plane:1.5:0.05:256 dropped normal (0.0000 0.0000 1.0000) offset 7.00: 400 of 1000 voxels (best of 256 draws: 380)")
    assert clean.plane_line(spec, np.array([3, -4, 0, 10, 7]), info).startswith("plane: plane:1.5:0.05:256 dropped normal (-0.6000 0.8000 0.0000) offset -2.00: ")
    spec = clean.parse_spec("plane:4:0.9")
    info = dict(n=1000, draws=1024, best_count=700, count=700, dropped=False)
    assert clean.plane_line(spec, np.array([0, 2, 0, 6, 8]), info) == (
        "plane: plane:4:0.9 no plane holds 0.9 of the voxels: the best has normal (0.0000 1.0000 0.0000) offset 3.00: 700 of 1000 voxels "
        "(best of 1024 draws: 700)")
    info = dict(n=2, draws=1024, best_count=0, count=0, dropped=False)
    assert clean.plane_line(clean.parse_spec("plane:1"), None, info) == (
        "plane: plane:1 no plane holds 0.05 of the voxels: none of 1024 draws spans a plane")


# ---------------------------------------------------------------------------- the three command lines
IO = ["--input", "a.ply", "--output", "b.ply"]
BAD = ["plane", "plane:0.7", "plane:0", "plane:33", "plane:1:0", "plane:1:2", "plane:1:0.1:0", "plane:1:0.1:5:-1", "plane:1:0.1:5:0:0"]


def test_the_command_lines_accept(capsys):
    a = clean.parse_args(IO + ["--clean", "stat:20:2.0", "--clean", "plane:1.5", "--clean", "largest:2"])
    assert [s.text for s in a.clean] == ["stat:20:2.0", "plane:1.5", "largest:2"] and a.clean[1].dist2 == 3
    a = ingest.parse_args(IO + ["--bits", "10", "--clean", "plane:2:0.1:4096:7"])
    assert [(s.kind, s.dist2, s.frac, s.draws, s.seed) for s in a.clean] == [("plane", 4, 0.1, 4096, 7)]
    a = cli.parse_args(["compress", "x.ply", "--voxelize", "7", "--clean", "plane:0.5"])
    assert a.clean == [clean.parse_spec("plane:0.5")]
    a = cli.parse_args(["compress", "x.ply", "--clean", "plane:32:1"])
    assert a.clean[0].dist2 == 64
    for parser in (clean.parse_args, ingest.parse_args):
        with pytest.raises(SystemExit) as e:
            parser(["--help"])
        assert e.value.code == 0
        assert "plane:D[:FRAC[:DRAWS[:SEED]]]" in " ".join(capsys.readouterr().out.split())


@pytest.mark.parametrize("text", BAD)
def test_the_command_lines_refuse(text, capsys):
    for parser, argv in ((clean.parse_args, IO), (ingest.parse_args, IO + ["--bits", "10"]), (cli.parse_args, ["compress", "x.ply"])):
        with pytest.raises(SystemExit) as e:
            parser(argv + ["--clean", text])
        assert e.value.code == 2 and "--clean " + text in capsys.readouterr().err
