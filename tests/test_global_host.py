"""The host side of the global alignment (pcgcv1_amd/register.py) without a GPU: the seeded draws, the edge
checks and the batched Kabsch solve against the rule in numpy (tests/_global_ref.py), every error by its message, the
command line's argument checks, and the conditions on the five-sphere fixture, checked on the reference alone."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _global_ref as ref                                                # noqa: E402
from pcgcv1_amd import register                                          # noqa: E402


def _corr(n=400, seed=7, wrong=0.5):
    """correspondences under a known pose, the share `wrong` of them paired at random"""
    rng = np.random.default_rng(seed)
    P = rng.uniform(0.0, 40.0, (n, 3)).astype(np.float32)
    R, t = ref.rodrigues(np.array([0.9, -1.3, 0.4])), np.array([12.5, -30.0, 7.25])
    Q = (P.astype(np.float64) @ R.T + t).astype(np.float32)
    bad = rng.random(n) < wrong
    Q[bad] = rng.uniform(-20.0, 60.0, (int(bad.sum()), 3)).astype(np.float32)
    return P, Q, R, t


def test_constants_are_the_rules():
    assert register.DRAW_BATCH == ref.DRAW_BATCH and register.EDGE_RATIO == ref.EDGE_RATIO
    assert (register.FEATURE_BINS, register.FEATURE_ROW) == (ref.N_BINS, ref.ROW)


def test_same_seed_same_triples():
    """the draws come in batches of DRAW_BATCH from default_rng(seed): the same seed gives the same kept triples and poses as
    the reference, bit for bit, across a batch boundary; another seed gives others"""
    P, Q, _, _ = _corr()
    draws = ref.DRAW_BATCH + 5000
    poses, index = register.draw_hypotheses(P, Q, 6.0, draws, 3)
    again, index2 = register.draw_hypotheses(P, Q, 6.0, draws, 3)
    want, want_index = ref.hypotheses(P, Q, 6.0, draws, 3)
    assert len(poses) > 50 and index.max() >= ref.DRAW_BATCH and np.all(np.diff(index) > 0)
    assert poses.tobytes() == again.tobytes() == want.tobytes() and np.array_equal(index, index2) and np.array_equal(index, want_index)
    first, first_index = register.draw_hypotheses(P, Q, 6.0, ref.DRAW_BATCH, 3)              # a prefix: the batches are the rule
    assert np.array_equal(first_index, index[:len(first_index)]) and first.tobytes() == poses[:len(first)].tobytes()
    other, other_index = register.draw_hypotheses(P, Q, 6.0, draws, 4)
    assert not np.array_equal(other_index[:20], index[:20])
    # the triples themselves
    rng = np.random.default_rng(3)
    tri = rng.integers(0, len(P), size=(ref.DRAW_BATCH, 3))
    keep = register.keep_triples(tri, P.astype(np.float64), Q.astype(np.float64), 6.0)
    assert np.array_equal(keep, ref.keep_triples(tri, P, Q, 6.0)) and np.array_equal(np.nonzero(keep)[0], first_index)


def test_edge_checks():
    """distinct indices, every source edge at least min_edge, every edge pair within a factor of 0.9 either way"""
    P = np.array([[0, 0, 0], [10, 0, 0], [0, 10, 0], [0, 5, 0], [0, 0, 9]], np.float64)
    Q = P.copy()
    Q[4] = [0, 0, 10.1]                                        # edges 9 -> 10.1 from point 0: 9 / 10.1 = 0.891 < 0.9
    tri = np.array([[0, 1, 2], [0, 1, 1], [0, 1, 3], [0, 1, 4], [2, 1, 0]])
    assert register.keep_triples(tri, P, Q, 6.0).tolist() == [True, False, False, False, True]
    assert register.keep_triples(tri, P, Q, 5.0).tolist() == [True, False, True, False, True]      # the edge of exactly min_edge counts
    Q[4] = [0, 0, 10.0]                                        # 9 / 10 = 0.9: kept
    assert register.keep_triples(tri, P, Q, 6.0).tolist() == [True, False, False, True, True]
    P[4] = [0, 0, 10.0]
    Q[4] = [0, 0, 9.0]                                         # the other way round
    assert register.keep_triples(tri, P, Q, 6.0)[3]


def test_batched_kabsch_is_solve_point_on_the_same_pairs():
    """three pairs as solve_point's sums about the origin.  The two form H differently (centred terms against sums minus
    n mu mu^T), so they agree to the round-off of H, about 1e-12 on entries near 1e4, over the triangle's second singular value
    (above 10 for edges of at least 6): 1e-9 on R and, times coordinates up to 60, 1e-7 on t are generous bounds."""
    P, Q, _, _ = _corr(wrong=0.0)
    P64, Q64 = P.astype(np.float64), Q.astype(np.float64)
    rng = np.random.default_rng(1)
    tri = rng.integers(0, len(P), size=(4000, 3))
    tri = tri[register.keep_triples(tri, P64, Q64, 6.0)][:100]
    assert len(tri) == 100
    R, t = register.kabsch(P64[tri], Q64[tri])
    Rr, tr = ref.kabsch(P64[tri], Q64[tri])
    assert R.tobytes() == Rr.tobytes() and t.tobytes() == tr.tobytes()
    for k, (a, b) in enumerate(zip(P64[tri], Q64[tri])):
        S = np.zeros(45)
        S[0], S[2:5], S[5:8], S[8:17] = 3.0, a.sum(0), b.sum(0), (a.T @ b).reshape(9)
        dR, dt = register.solve_point(S)
        assert np.abs(R[k] - dR).max() <= 1e-9 and np.abs(t[k] - dt).max() <= 1e-7, k
        assert abs(np.linalg.det(R[k]) - 1.0) < 1e-12
    # a mirrored triple still gives a proper rotation
    Rm, _ = register.kabsch(P64[tri[:5]], Q64[tri[:5]] * np.array([1.0, 1.0, -1.0]))
    assert np.abs(np.linalg.det(Rm) - 1.0).max() < 1e-12


def test_host_rule_finds_the_pose_among_wrong_pairs():
    """half the pairs wrong: register.ransac with the reference's scorer is the reference's ransac, and both find the pose"""
    P, Q, R, t = _corr()
    got = register.ransac(P, Q, 2.0, 6.0, 20000, 0, 20, scorer=lambda poses: ref.score(poses, P, Q, 2.0))
    want = ref.ransac(P, Q, 2.0, 6.0, 20000, 0, 20)
    assert all(got[k] == want[k] for k in ("inliers", "correspondences", "hypotheses", "draw", "draws", "raw_inliers"))
    assert got["R"].tobytes() == want["R"].tobytes() and got["t"].tobytes() == want["t"].tobytes()
    assert np.abs(got["R"] - R).max() < 1e-5 and np.abs(got["t"] - t).max() < 1e-3 and 150 < got["inliers"] < 260
    mask = register.inlier_mask(np.concatenate([R.reshape(9), t]), P, Q, 2.0)
    assert np.array_equal(mask, ref.inlier_mask(np.concatenate([R.reshape(9), t]), P, Q, 2.0)) and mask.sum() == got["inliers"]


def test_every_error_names_its_cause():
    P, Q, _, _ = _corr()
    numpy_scorer = lambda poses: ref.score(poses, P, Q, 2.0)                                  # noqa: E731
    with pytest.raises(ValueError, match="fewer than 3 valid correspondences \\(2\\)"):
        register.ransac(P[:2], Q[:2])
    with pytest.raises(ValueError, match="fewer than 3 valid correspondences \\(0\\)"):
        register.ransac(P[:0], Q[:0])
    with pytest.raises(ValueError, match="no triple kept: none of 3000 draws among 400 correspondences"):
        register.ransac(P, Q, 2.0, 500.0, 3000, 0, 20)
    with pytest.raises(ValueError, match="has [12][0-9][0-9] inliers of 400 correspondences, below min_inliers = 300"):
        register.ransac(P, Q, 2.0, 6.0, 20000, 0, 300, scorer=numpy_scorer)
    for kw in ({"corr_dist": 0.0}, {"corr_dist": float("nan")}, {"min_edge": -1.0}, {"draws": 0}):
        with pytest.raises(ValueError, match="corr_dist must be positive"):
            register.ransac(P, Q, **kw)
    with pytest.raises(ValueError, match="feature_voxel must be positive"):
        register.keypoints(P, None, 0.0)
    with pytest.raises(ValueError, match="needs more than 12 bits"):
        register.keypoints(P, None, 1e-4)
    with pytest.raises(ValueError, match="radius must be positive"):
        register.feature_cells(P, -1.0)
    assert register.feature_cells(P, 8.0)[0] == 8.0 and register.feature_cells(P, 8.5)[0] == 16.0 and register.feature_cells(P, 0.5)[0] == 1.0
    h, ox, oy, oz, res = register.feature_cells(P * 100.0 - 5000.0, 3.0)
    assert h == 4.0 and ox < 0 and res <= 1024


def test_cell_keys_and_rows_outside_the_cells():
    """the key (x * res + y) * res + z of floor(p / h) - origin (pcgcv1_amd/cells.py): -1 for a row outside the cells or not
    finite, which cell_order sorts first; clamp=True gives such a row the nearest cell's key, a NaN counting as 0"""
    import torch
    from pcgcv1_amd import cells
    assert register.cell_order is cells.cell_order and register.cells_from_bounds is cells.cells_from_bounds
    grid = (2.0, -3, 0, 1, 4)                                  # x in [-6, 2), y in [0, 8), z in [2, 10)
    nan, inf = float("nan"), float("inf")
    p = torch.tensor([[-6.0, 0.0, 2.0], [1.5, 7.5, 9.5], [-0.5, 3.0, 4.0], [2.0, 3.0, 4.0], [-6.5, 3.0, 4.0], [0.0, nan, 4.0],
                      [0.0, 3.0, -inf], [inf, 9.0, 1.0]], dtype=torch.float32)
    inside = [(0 * 4 + 0) * 4 + 0, (3 * 4 + 3) * 4 + 3, (2 * 4 + 1) * 4 + 1]
    assert cells.cell_keys(p, grid).tolist() == inside + [-1] * 5
    assert cells.cell_keys(p, grid, clamp=True).tolist() == inside + [(3 * 4 + 1) * 4 + 1, (0 * 4 + 1) * 4 + 1, (3 * 4 + 0) * 4 + 1,
                                                                     (3 * 4 + 1) * 4 + 0, (3 * 4 + 3) * 4 + 0]
    assert cells.cell_order(p, grid).tolist() == [3, 4, 5, 6, 7, 0, 2, 1]


def test_argument_errors_of_the_command_line(tmp_path, capsys):
    missing = [str(tmp_path / ("scan%d.ply" % k)) for k in range(2)]
    base = ["--input"] + missing + ["--output", str(tmp_path / "merged.ply"), "--bits", "10"]
    poses = str(tmp_path / "start.poses.json")
    register.write_poses(poses, missing, [{"pose": np.eye(4), "iterations": [], "converged": True, "fitness": 1.0, "rmse": 0.0,
                                           "plane_rmse": None}] * 2)
    cases = [
        (base + ["--metric", "point", "--global_init", "--init", poses], "not together with --init"),
        (base + ["--global_init"], "--metric=plane needs normals"),
        (base + ["--metric", "point", "--global_init", "--feature_voxel", "0"], "--feature_voxel must be positive"),
        (base + ["--metric", "point", "--global_init", "--feature_radius", "nan"], "--feature_radius must be positive"),
        (base + ["--metric", "point", "--global_init", "--corr_dist", "-2"], "--corr_dist must be positive"),
        (base + ["--metric", "point", "--global_init", "--draws", "0"], "--draws must be at least 1"),
    ]
    for argv, message in cases:
        with pytest.raises(SystemExit) as e:
            register.parse_args(argv)
        assert e.value.code == 2 and message in capsys.readouterr().err, argv
    args = register.parse_args(base + ["--metric", "point", "--global_init", "--draws", "5000", "--seed", "3"])
    assert args.global_init and args.draws == 5000 and args.seed == 3
    assert (args.feature_voxel, args.feature_radius, args.corr_dist) == (1.0, 8.0, 2.0)
    assert not register.parse_args(base + ["--metric", "point"]).global_init
    assert register.parse_args(base + ["--metric", "point", "--init", poses]).init == poses
    with pytest.raises(SystemExit):
        register.parse_args(["--help"])
    text = capsys.readouterr().out
    assert "--global_init" in text and "first gate" in text and "--corr_dist" in text


def test_poses_file_carries_the_global_block(tmp_path):
    name = str(tmp_path / "merged.poses.json")
    entry = {"pose": np.eye(4), "iterations": [3, 2, 2], "converged": True, "fitness": 0.8, "rmse": 0.4, "plane_rmse": 0.02}
    with_block = dict(entry, **{"global": {"inliers": np.int64(203), "correspondences": 4293, "hypotheses": 1277, "draw": np.int64(67762)}})
    register.write_poses(name, ["a.ply", "b.ply"], [entry, with_block])
    back = register.read_poses(name)
    assert "global" not in back[0]
    assert back[1]["global"] == {"inliers": 203, "correspondences": 4293, "hypotheses": 1277, "draw": 67762}


def test_fixture_conditions_hold_for_the_reference():
    """The five-sphere pair, a turn of 84 .. 162 degrees and tens of voxels apart: the rule in numpy recovers the pose, and the
    winner's count is at least 1.1 times the best count among the hypotheses that leave a source point more than 4 voxels from
    its place (DESIGN.md §7i records the two counts)."""
    fx = ref.fixture()
    assert 4000 < len(fx["source"]) < 5000 and 4500 < len(fx["target"]) < 5500
    angle = np.degrees(np.arccos((np.trace(fx["R"]) - 1.0) / 2.0))
    assert 84.0 <= angle <= 162.0 and np.linalg.norm(fx["source"].astype(np.float64) - fx["source_true"], axis=1).max() > 30.0
    off = fx["source_true"][:, None, :] - ref.CENTRES[None]                # every source normal is its sphere's, turned with the cloud
    sphere = np.abs(np.linalg.norm(off, axis=2) - ref.RADII).argmin(1)
    radial = off[np.arange(len(sphere)), sphere] / ref.RADII[sphere, None]
    assert np.abs(np.abs(((fx["source_normals"].astype(np.float64) @ fx["R"]) * radial).sum(1)) - 1.0).max() < 1e-5
    signs = np.sign((fx["target_normals"] * (fx["target"] - ref.CENTRES[0])).sum(1))
    assert 0.4 < (signs > 0).mean() < 0.6                      # the normals point either way
    out = ref.fixture_align(fx)
    src = fx["source"].astype(np.float64)
    err = np.array([np.linalg.norm(src @ p[:9].reshape(3, 3).T + p[9:] - fx["source_true"], axis=1).max() for p in out["poses"]])
    wrong = err > ref.FAR
    w = int(np.argmax(out["counts"]))
    best_wrong = int(out["counts"][wrong].max())
    refined = ref.point_error(out["R"], out["t"], fx)
    print("fixture: %d correspondences, %d hypotheses of which %d near the truth, winner draw %d with %d inliers %.3f voxel off, best "
          "wrong pose %d, refined %d inliers %.3f voxel off" % (out["correspondences"], out["hypotheses"], int((~wrong).sum()), out["draw"],
                                                               int(out["counts"][w]), err[w], best_wrong, out["inliers"], refined))
    assert 1000 < out["hypotheses"] < 2000 and 5 <= int((~wrong).sum()) <= 50
    assert not wrong[w] and out["counts"][w] >= 1.1 * best_wrong
    assert refined <= ref.CORR_DIST                            # what the first gate of 4 has to bridge, with room
