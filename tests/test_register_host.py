"""The host side of pcgcv1_amd/register.py without a GPU: the rule in numpy (tests/_register_ref.py) recovers a known pose on
the partial-overlap pair the GPU tests use, and the solves, the pose conversion, the errors, the command line's argument
checks and the poses file of register.py agree with it."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _register_ref as ref                                              # noqa: E402
from pcgcv1_amd import ingest, register                                  # noqa: E402

_PAIR = {}


def _pair():
    """the overlap pair and the reference's sums at the start pose and the first gate, computed once"""
    if not _PAIR:
        d = ref.overlap_pair()
        q64 = d["target"].astype(np.float64)
        c = np.rint((q64.min(0) + q64.max(0)) / 2.0)
        _PAIR.update(d, c=c, S=ref.step(d["source"], d["target"], d["target_normals"], np.eye(3), np.zeros(3), c, 4.0)["S"])
    return _PAIR


def test_reference_loop_recovers_the_known_pose():
    """plane mode, schedule (4, 2, 1): every source point lands within 0.05 voxel of where it belongs (a condition on the
    generator: two independent samplings, a quarter of the object missing from each, 5 degrees and 1.4 voxels off)"""
    d = _pair()
    assert len(d["source"]) > 1500 and len(d["target"]) > 1500
    Rk, tk = ref.known_pose()
    moved = np.linalg.norm(d["source"].astype(np.float64) - d["source_true"], axis=1)
    assert 1.0 < moved.max() < 4.0 and abs(math.degrees(ref.angle(Rk)) - 5.0) < 1e-9
    out = ref.icp(d["source"], d["target"], d["target_normals"], "plane", (4.0, 2.0, 1.0))
    err = np.linalg.norm(d["source"].astype(np.float64) @ out["R"].T + out["t"] - d["source_true"], axis=1).max()
    rot = math.degrees(ref.angle(out["R"] @ Rk))
    print("reference loop: steps %s, max point error %.4f voxel, rotation error %.4f degrees" % (out["iterations"], err, rot))
    assert out["converged"] and err <= 0.05
    assert 0.5 < out["fitness"] < 0.9 and out["plane_rmse"] < out["rmse"]


def test_solves_and_compose_agree_with_the_reference():
    S, c = _pair()["S"], _pair()["c"]
    assert S[0] > 1000 and np.abs(S[17:45]).min() > 0
    for mine, theirs in ((register.solve_point, ref.solve_point), (register.solve_plane, ref.solve_plane)):
        (dR, dt), (dR_ref, dt_ref) = mine(S), theirs(S)
        assert np.abs(dR - dR_ref).max() <= 1e-12 and np.abs(dt - dt_ref).max() <= 1e-12
        assert np.abs(dR @ dR.T - np.eye(3)).max() < 1e-14 and np.linalg.det(dR) > 0
    R0, t0 = ref.rodrigues([0.1, -0.2, 0.05]), np.array([0.5, -1.0, 2.0])
    dR, dt = register.solve_plane(S)
    (R1, t1), (R2, t2) = register.compose(R0, t0, c, dR, dt), ref.compose(R0, t0, c, dR, dt)
    assert np.abs(R1 - R2).max() <= 1e-12 and np.abs(t1 - t2).max() <= 1e-12
    x = np.array([3.0, 20.0, 11.0])                           # compose = the step about c after the pose
    assert np.abs((R1 @ x + t1) - (dR @ ((R0 @ x + t0) - c) + dt + c)).max() < 1e-12
    assert abs(register.rotation_angle(dR) - ref.angle(dR)) <= 1e-15
    assert np.abs(register.rodrigues([0.3, 0.2, -0.1]) - ref.rodrigues([0.3, 0.2, -0.1])).max() <= 1e-15


def test_kabsch_returns_a_rotation_for_a_reflected_fit():
    """sums of a cloud and its mirror image: the best orthogonal map is a reflection, the solve returns a proper rotation"""
    rng = np.random.default_rng(3)
    a = rng.normal(size=(50, 3))
    b = a * np.array([1.0, 1.0, -1.0])
    S = np.zeros(45)
    S[0], S[2:5], S[5:8], S[8:17] = len(a), a.sum(0), b.sum(0), (a.T @ b).reshape(9)
    dR, _ = register.solve_point(S)
    assert abs(np.linalg.det(dR) - 1.0) < 1e-12


def test_pose_to_scan_units_round_trips_through_a_frame():
    frame = ingest.Frame((-1.25, 3.5, 0.125), 0.002, 10)
    R, t = ref.rodrigues([0.05, -0.02, 0.08]), np.array([1.5, -0.75, 0.25])
    Rs, ts = register.pose_to_scan_units(R, t, frame)
    p = np.random.default_rng(5).uniform(-1, 1, (20, 3)) + frame.origin
    g = (p - frame.origin) / frame.step
    want = frame.origin + frame.step * (g @ R.T + t)           # the motion on the grid, brought back
    assert np.abs((p @ Rs.T + ts) - want).max() < 1e-12
    Rg, tg = register.pose_from_scan_units(Rs, ts, frame)
    assert np.array_equal(Rg, R) and np.abs(tg - t).max() < 1e-10
    M = register.pose_matrix(Rs, ts)
    assert M.shape == (4, 4) and np.array_equal(M[:3, :3], Rs) and np.array_equal(M[:3, 3], ts) and M[3].tolist() == [0, 0, 0, 1]


def test_a_planar_cloud_is_refused_with_its_likely_cause():
    """every normal (0, 0, 1) and every point in z = 5: translation in the plane and rotation about z are free"""
    g = np.stack(np.meshgrid(np.arange(8.0), np.arange(8.0), indexing="ij"), -1).reshape(-1, 2)
    q = np.concatenate([g, np.full((64, 1), 5.0)], 1).astype(np.float32)
    n = np.tile(np.array([[0.0, 0.0, 1.0]], np.float32), (64, 1))
    S = ref.step(q + np.float32(0.25), q, n, np.eye(3), np.zeros(3), np.array([4.0, 4.0, 5.0]), 2.0)["S"]
    assert S[0] == 64
    with pytest.raises(ValueError, match="singular.*a plane, a sphere or too few pairs"):
        register.solve_plane(S)
    with pytest.raises(ValueError):
        ref.solve_plane(S)


def test_too_few_pairs_names_the_gate():
    S = np.zeros(45)
    for metric, n in (("point", 2), ("plane", 5)):
        S[0] = n
        with pytest.raises(ValueError, match=r"nothing lies within max_dist = 1\.5 "):
            register._check_pairs(S, metric, 1.5)
        S[0] = n + 1
        register._check_pairs(S, metric, 1.5)


def test_argument_errors_come_before_anything_is_loaded(tmp_path, capsys):
    """none of the named files exists: an error about the arguments, not about a file"""
    missing = [str(tmp_path / ("scan%d.ply" % k)) for k in range(2)]
    out = str(tmp_path / "merged.ply")
    cases = [
        (["--input"] + missing + ["--output", out], "give --bits or --voxel_size"),
        (["--input"] + missing + ["--output", out, "--bits", "10", "--voxel_size", "0.5"], "give --bits or --voxel_size"),
        (["--input"] + missing + ["--output", out, "--bits", "13"], "outside 1..12"),
        (["--input"] + missing[:1] + ["--output", out, "--bits", "10", "--metric", "point"], "two scans or more"),
        (["--input"] + missing + ["--output", out, "--bits", "10", "--metric", "point", "--max_dist", "4,0"], "--max_dist"),
        (["--input"] + missing + ["--output", out, "--bits", "10", "--metric", "point", "--iters", "0"], "--iters"),
        (["--input"] + missing + ["--output", out, "--bits", "10", "--clean", "bogus:1"], "clean"),
        (["--input"] + missing + ["--output", out, "--bits", "10"], "--metric=plane needs normals"),
        (["--input"] + missing + ["--output", out, "--bits", "10", "--metric", "point", "--init", str(tmp_path / "no.json")], "--init"),
    ]
    for argv, message in cases:
        with pytest.raises(SystemExit) as e:
            register.parse_args(argv)
        assert e.value.code == 2 and message in capsys.readouterr().err, argv
    args = register.parse_args(["--input"] + missing + ["--output", out, "--bits", "10", "--metric", "point", "--max_dist", "3,1.5"])
    assert args.max_dist == [3.0, 1.5] and args.min_fitness == 0.3 and args.iters == 50 and args.tol == 1e-3
    # the same rule through the functions, before a device is asked for
    cloud = np.zeros((4, 3), np.float32)
    with pytest.raises(ValueError, match="metric='plane' needs the target's normals"):
        register.icp(cloud, cloud)
    with pytest.raises(ValueError, match="metric='plane' needs the target's normals"):
        register.register_scans([(cloud, None, None), (cloud, None, None)], bits=5)
    with pytest.raises(ValueError, match="metric must be"):
        register.icp(cloud, cloud, metric="d2")


def test_poses_file_round_trips(tmp_path):
    R, t = ref.rodrigues([0.1, 0.2, -0.3]), np.array([1e-3, -2.5, 1.0 / 3.0])
    poses = [{"pose": np.eye(4), "iterations": [], "converged": True, "fitness": 1.0, "rmse": 0.0, "plane_rmse": None},
             {"pose": register.pose_matrix(R, t), "iterations": [8, 5, 3], "converged": True, "fitness": 0.72, "rmse": 0.379,
              "plane_rmse": 0.014}]
    name = str(tmp_path / "merged_vox10.poses.json")
    assert register.poses_path(str(tmp_path / "merged_vox10.ply")) == name
    register.write_poses(name, ["a.ply", "b.ply"], poses)
    back = register.read_poses(name)
    assert [e["file"] for e in back] == ["a.ply", "b.ply"]
    for e, p in zip(back, poses):
        assert e["pose"].tobytes() == np.asarray(p["pose"], np.float64).tobytes()
        assert all(e[k] == p[k] for k in ("iterations", "converged", "fitness", "rmse", "plane_rmse"))
    with open(name, "w") as f:
        f.write('[{"file": "a.ply", "pose": [[1, 0], [0, 1]]}]')
    with pytest.raises(ValueError, match="4x4 pose"):
        register.read_poses(name)
