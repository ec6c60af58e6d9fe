"""Registration on the device (csrc/offgrid.hip: pcgc_register_*; pcgcv1_amd/register.py) against the rule in numpy
(tests/_register_ref.py): one step sum by sum, then the loop, the merge of three scans and the command line."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _offgrid_ref as oref                                              # noqa: E402
import _register_ref as ref                                              # noqa: E402
from pcgcv1_amd import _lib, ingest, metrics, register                   # noqa: E402

OFFGRID = oref.cases()
# the off-grid pairs the step runs on, with a gate that at least one source point passes
GATES = {"twelve_ties": 4.0, "far": 100.0, "rod_edge_2": 60.0, "s5_8": 2.0}
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _lib.require_gpu()


def _pose_about(c, small=True):
    """a rotation about the centre c and a shift, with entries that are not float32 numbers"""
    R = ref.rodrigues(np.array([0.01, -0.02, 0.015]) if small else np.array([0.3, -0.2, 0.25]))
    return R, c - R @ c + np.array([0.3, -0.2, 0.1])


def _check_step(source, target, normals, R, t, max_dist, what):
    """a step on the device against the reference: n_used, best and ties equal, every sum within the summation bound"""
    m = register.Matcher(source, target, normals)
    c = m.centre
    if R is None:
        R, t = _pose_about(c)
    S, best, ties = m.step(R, t, c, max_dist, per_point=True)
    unit = None if normals is None else register._unit_normals(normals, len(target))
    want = ref.step(source, target, unit, R, t, c, max_dist)
    assert S[0] == want["S"][0], (what, S[0], want["S"][0])
    assert best.tobytes() == want["best"].tobytes(), (what, int((best != want["best"]).sum()))
    assert np.array_equal(ties, want["ties"]), what
    err, bound = np.abs(S - want["S"]), ref.bound(want)
    print(what, "n_used %d, largest error / bound %.3g" % (S[0], float((err / np.maximum(bound, 1e-300)).max())))
    assert np.all(err <= bound), (what, np.nonzero(err > bound)[0].tolist())
    return S, want, m


@pytest.mark.parametrize("posed", (False, True))
@pytest.mark.parametrize("name", sorted(GATES))
def test_step_on_the_offgrid_cases(name, posed):
    """ties (twelve_ties, s5_8), a source outside the target's box (far), cells of edge 2 with a negative origin
    (rod_edge_2); at identity, and under a pose whose result is rounded to float32"""
    a, b, _ = OFFGRID[name]
    normals = oref._normals(500 + len(b), len(b))
    identity = (np.eye(3), np.zeros(3))
    S, want, m = _check_step(a, b, normals, *(((None, None) if posed else identity) + (GATES[name], (name, posed))))
    assert S[0] >= 1 and m.cells.h == (2.0 if name == "rod_edge_2" else 1.0)
    if not posed:
        if name == "twelve_ties":
            assert want["ties"].tolist() == [12] and want["best"].tolist() == [4.5]
        if name == "s5_8":
            assert want["ties"].max() >= 2
    if name == "rod_edge_2":
        assert min(m.cells.origin) < 0


def _uniform_case():
    if "uniform" not in _CACHE:
        rng = np.random.default_rng(21)
        q = rng.uniform(0, 20, (1000, 3)).astype(np.float32)
        p = rng.uniform(-1, 21, (300000, 3)).astype(np.float32)
        p[0] = q[0] + np.float32(0.125)                       # the cloud of one point is inside the gate
        _CACHE["uniform"] = (p, q, oref._normals(22, 1000))
    return _CACHE["uniform"]


@pytest.mark.parametrize("n", (1, 63, 257, 300000))
def test_step_sizes(n):
    """less than a wave, more than a workgroup, and more points than 1024 workgroups x 256 threads: the stride loop runs"""
    p, q, normals = _uniform_case()
    S, want, _ = _check_step(p[:n], q, normals, None, None, 1.5, "n = %d" % n)
    assert 1 <= S[0] and (n == 1 or S[0] < n)
    assert n <= 1024 * 256 or S[0] > 1000


def test_gate_equal_to_a_distance():
    """best = 9 exactly: max_dist = 3 uses the point, the next number below 3 does not"""
    p = np.array([[5, 5, 5]], np.float32)
    q = np.array([[5, 5, 8], [20, 20, 20]], np.float32)
    normals = np.array([[0, 0, 1], [1, 0, 0]], np.float32)
    eye = (np.eye(3), np.zeros(3))
    S, want, m = _check_step(p, q, normals, *eye, 3.0, "gate = distance")
    assert S[0] == 1 and S[1] == 9.0 and want["ties"].tolist() == [1]
    S, want, _ = _check_step(p, q, normals, *eye, float(np.nextafter(3.0, 0.0)), "gate below distance")
    assert want["best"].tolist() == [9.0] and want["ties"].tolist() == [0]
    assert not S.any()


def test_a_gate_nothing_passes():
    """the sums are zero, and the loop says that nothing lies within max_dist"""
    p, q, normals = _uniform_case()
    far = p[:500] + np.float32(40.0)
    S, _, _ = _check_step(far, q, normals, np.eye(3), np.zeros(3), 1.0, "nothing passes")
    assert not S.any()
    for metric in ("plane", "point"):
        with pytest.raises(ValueError, match=r"nothing lies within max_dist = 1 "):
            register.icp(far, q, normals, metric=metric, max_dist=(1.0,))


def test_without_normals_the_plane_sums_are_zero():
    p, q, normals = _uniform_case()
    S, want, m = _check_step(p[:257], q, None, None, None, 1.5, "no normals")
    assert S[0] > 1 and S[8:17].all() and not S[17:].any() and not want["S"][17:].any()
    m = register.Matcher(p[:257], q, normals)                 # and a matcher that has normals leaves them out when asked to
    assert np.array_equal(m.step(*_pose_about(m.centre), m.centre, 1.5, with_normals=False), S)


def test_nan_source_is_an_error_and_leaves_the_matcher_usable():
    p, q, normals = _uniform_case()
    bad = p[:257].copy()
    bad[100, 1] = np.nan
    m = register.Matcher(bad, q, normals)
    with pytest.raises(RuntimeError, match="pcgc_register_step"):
        m.step(np.eye(3), np.zeros(3), m.centre, 1.5)
    with pytest.raises(RuntimeError, match="pcgc_register_step"):             # a pose that throws the cloud out of every cell's reach
        register.Matcher(p[:257], q, normals).step(np.eye(3), np.full(3, 1e30), m.centre, 1.5)
    good = register.Matcher(p[:257], q, normals)
    first = good.step(np.eye(3), np.zeros(3), good.centre, 1.5)
    with pytest.raises(RuntimeError):
        good.step(np.eye(3), np.full(3, np.float64(3e38)), good.centre, 1.5)
    assert np.array_equal(good.step(np.eye(3), np.zeros(3), good.centre, 1.5), first)      # the flag is the step's own


def test_bad_arguments_are_refused():
    p, q, normals = _uniform_case()
    m = register.Matcher(p[:63], q, normals)
    for R, t, c, gate in ((np.eye(3), np.zeros(3), m.centre, 0.0), (np.eye(3), np.zeros(3), m.centre, float("inf")),
                          (np.eye(3), np.zeros(3), m.centre, float("nan")), (np.eye(3) * np.nan, np.zeros(3), m.centre, 1.0),
                          (np.eye(3), np.array([0, np.inf, 0]), m.centre, 1.0), (np.eye(3), np.zeros(3), np.array([np.nan, 0, 0]), 1.0)):
        with pytest.raises(_lib.PcgcError, match="pcgc_register_step"):
            m.step(R, t, c, gate)
    lib = _lib.hip()
    assert lib.pcgc_register_workspace_bytes(0, 10) == 0 and lib.pcgc_register_workspace_bytes(8, 0) == 0
    assert lib.pcgc_register_workspace_bytes(8, 10) == lib.pcgc_offgrid_workspace_bytes(8, 10) + 45 * 1024 * 8
    assert lib.pcgc_register_prepare(_lib.dptr(m.cells.points), m.m, *m.cells.grid(), _lib.dptr(m.ws), m.ws.numel() - 1, _lib.stream()) != 0
    assert lib.pcgc_register_prepare(None, m.m, *m.cells.grid(), _lib.dptr(m.ws), m.ws.numel(), _lib.stream()) != 0


def test_two_runs_give_the_same_bits():
    p, q, normals = _uniform_case()
    m = register.Matcher(p, q, normals)
    R, t = _pose_about(m.centre)
    first = m.step(R, t, m.centre, 1.5)
    assert first.tobytes() == m.step(R, t, m.centre, 1.5).tobytes()
    assert first.tobytes() == register.Matcher(p, q, normals).step(R, t, m.centre, 1.5).tobytes()


def test_sorting_the_source_by_cell_keeps_every_answer():
    """what the loop does once per stage: the per-point outputs stay in the caller's order, the sums stay within the bound"""
    p, q, normals = _uniform_case()
    m = register.Matcher(p[:5000], q, normals)
    R, t = _pose_about(m.centre, small=False)
    want = ref.step(p[:5000], q, register._unit_normals(normals, len(q)), R, t, m.centre, 1.5)
    before = m.step(R, t, m.centre, 1.5, per_point=True)
    m.sort_source(R, t)
    m.sort_source(*_pose_about(m.centre))                     # twice: the orders compose
    assert not np.array_equal(m.source_d.cpu().numpy(), p[:5000])
    after = m.step(R, t, m.centre, 1.5, per_point=True)
    for S, best, ties in (before, after):
        assert best.tobytes() == want["best"].tobytes() and np.array_equal(ties, want["ties"])
        assert S[0] == want["S"][0] and np.all(np.abs(S - want["S"]) <= ref.bound(want))


def test_best_is_pc_error_floats_best_of_the_moved_cloud():
    p, q, normals = _uniform_case()
    m = register.Matcher(p[:5000], q, normals)
    R, t = _pose_about(m.centre, small=False)
    _, best, _ = m.step(R, t, m.centre, 1.5, per_point=True)
    _, detail = metrics.pc_error_float(ref.transform(p[:5000], R, t), q, None, 1023, per_point=True)
    assert best.tobytes() == detail["1"][0].tobytes()


# ---------------------------------------------------------------------------- the loop
def _apart(a, b, points):
    p = np.asarray(points, np.float64)
    return float(np.linalg.norm((p @ a["R"].T + a["t"]) - (p @ b["R"].T + b["t"]), axis=1).max())


# point mode gets 8 steps per stage, not the default 50: it creeps (100 steps and more to settle), every step of
# the reference is a dense 1 850 x 1 900 pair matrix, and 24 steps in step with the reference pin the loop as well as 150 would
@pytest.mark.parametrize("metric,iters", (("plane", 50), ("point", 8)))
def test_loop_follows_the_reference(metric, iters):
    """the partial-overlap pair, 5 degrees and 1.4 voxels off: the same steps per stage, the same points inside the last gate,
    and poses that move no source point apart by more than tol"""
    d = ref.overlap_pair()
    want = ref.icp(d["source"], d["target"], d["target_normals"], metric, (4.0, 2.0, 1.0), iters, 1e-3)
    got = register.icp(d["source"], d["target"], d["target_normals"], metric, (4.0, 2.0, 1.0), iters, 1e-3)
    apart = _apart(got, want, d["source"])
    err = np.linalg.norm(d["source"].astype(np.float64) @ got["R"].T + got["t"] - d["source_true"], axis=1).max()
    print("%s: steps %s, n_used %d, device and reference %.3g voxel apart, max point error %.4f voxel" % (
        metric, got["iterations"], got["n_used"], apart, err))
    assert got["iterations"] == want["iterations"] and got["converged"] == want["converged"]
    assert got["n_used"] == want["n_used"] and got["fitness"] == want["fitness"]
    assert apart <= 1e-3
    assert abs(got["rmse"] - want["rmse"]) < 1e-6 and (got["plane_rmse"] is None) == (metric == "point")
    if metric == "plane":
        assert got["converged"] and err <= 0.05 and abs(got["plane_rmse"] - want["plane_rmse"]) < 1e-6


UNIT = 0.01                  # scanner units per unit of the surface generator
VOXEL = 0.005                # the voxel edge the three scans are merged at: the object is 20 voxels in radius


def _three():
    """the three scans registered on the device, and their union built with the reference loop's poses; once"""
    if "three" not in _CACHE:
        scans, _ = ref.three_scans(unit=UNIT)
        out = register.register_scans(scans, voxel_size=VOXEL, metric="plane", estimate_normals=True)
        pts, ref_poses = [scans[0][0]], []
        for p, _, _ in scans[1:]:
            target = np.concatenate(pts)
            frame = ingest.fit_frame(target, voxel_size=VOXEL)
            normals = register._unit_normals(register.estimated_target_normals(target, frame), len(target))
            r = ref.icp(register.to_grid(p, frame), register.to_grid(target, frame), normals, "plane")
            r["R"], r["t"] = register.pose_to_scan_units(r["R"], r["t"], frame)
            ref_poses.append(r)
            pts.append(p @ r["R"].T + r["t"])
        union = np.concatenate(pts)
        want = ingest.voxelize_scan(union, np.concatenate([s[1] for s in scans]), None, voxel_size=VOXEL)
        _CACHE["three"] = (scans, out, ref_poses, union, want)
    return _CACHE["three"]


def test_three_scans_merge_as_the_reference_poses_merge_them():
    """scan 2 overlaps scan 1 and not scan 0; colours, estimated normals.  Voxels, counts and colours equal those of the union
    under the reference loop's poses, but for the voxels a point within 1e-3 voxel of a boundary touches: under 1 % of them"""
    scans, out, ref_poses, union, want = _three()
    lo = [s[0][:, 0].min() for s in scans]
    hi = [s[0][:, 0].max() for s in scans]
    assert hi[0] < lo[2] - VOXEL and lo[1] < hi[0] and lo[2] < hi[1]             # 0 and 2 are apart, 1 bridges them
    for k, (r, w) in enumerate(zip(out["poses"][1:], ref_poses), 1):
        apart = _apart(r, w, scans[k][0]) / VOXEL
        print("scan %d: steps %s, fitness %.3f, device and reference %.3g voxel apart" % (k, r["iterations"], r["fitness"], apart))
        assert r["converged"] and r["iterations"] == w["iterations"] and r["n_used"] == w["n_used"] and apart <= 1e-3
    points, colors, normals, counts, frame, n_dropped = out["merged"]
    w_points, w_colors, _, w_counts, w_frame, _ = want
    assert frame == w_frame and normals is None and n_dropped == 0 and counts.sum() == len(union) == w_counts.sum()
    # the voxels a boundary point of the reference union touches: its own and the one across the boundary
    u = (union - frame.origin) / frame.step + 0.5
    near = np.abs(u - np.rint(u)).min(1) < 1e-3
    res = 1 << frame.bits

    def keys(v):
        v = np.clip(v, 0, frame.R).astype(np.int64)
        return (v[:, 0] * res + v[:, 1]) * res + v[:, 2]
    own = np.unique(keys(np.floor(u[near])))
    touched = np.unique(np.concatenate([keys(np.floor(u[near] + (np.array(d) - 1.0) * 1e-3)) for d in np.ndindex(3, 3, 3)]))
    print("%d voxels, %d hold a point within 1e-3 of a boundary, %d dropped from the comparison" % (len(w_points), len(own), len(touched)))
    assert len(own) < 0.01 * len(w_points)
    k_got, k_want = keys(points), keys(w_points)
    keep_got, keep_want = ~np.isin(k_got, touched), ~np.isin(k_want, touched)
    assert keep_want.sum() > 0.97 * len(w_points)
    assert np.array_equal(points[keep_got], w_points[keep_want])
    assert np.array_equal(counts[keep_got], w_counts[keep_want]) and np.array_equal(colors[keep_got], w_colors[keep_want])


def test_command_line_round_trip(tmp_path, capsys):
    """plies in, the voxelised ply, its frame and the poses out: what register_scans returns for the same scans"""
    from pcgcv1_amd.dataprocess.inout_points import load_ply_scan, write_ply_colors
    scans, out = _three()[:2]
    names = [str(tmp_path / ("scan%d.ply" % k)) for k in range(3)]
    for name, (p, col, _) in zip(names, scans):
        write_ply_colors(name, p, col)
        back = load_ply_scan(name)
        assert np.array_equal(back[0], p) and np.array_equal(back[1], col)          # the text holds the float64 as they are
    merged = str(tmp_path / "merged.ply")
    register.main(["--input"] + names + ["--output", merged, "--voxel_size", repr(VOXEL), "--estimate_normals"])
    printed = capsys.readouterr().out
    assert printed.count("register: ") == 2 and "NOT converged" not in printed and "wrote " in printed
    points, colors, _ = load_ply_scan(merged)
    assert np.array_equal(points, out["merged"][0]) and np.array_equal(colors, out["merged"][1])
    assert ingest.read_frame(ingest.frame_path(merged)) == out["merged"][4]
    poses = register.read_poses(register.poses_path(merged))
    assert [e["file"] for e in poses] == ["scan0.ply", "scan1.ply", "scan2.ply"]
    for e, r in zip(poses, out["poses"]):
        assert e["pose"].tobytes() == r["pose"].tobytes() and e["iterations"] == r["iterations"] and e["converged"]
    # the poses it wrote are a start it accepts: at the last gate alone they are where the loop stays
    again = str(tmp_path / "again.ply")
    register.main(["--input"] + names + ["--output", again, "--voxel_size", repr(VOXEL), "--estimate_normals", "--max_dist", "1",
                   "--iters", "3", "--init", register.poses_path(merged)])
    for k, (e, r) in enumerate(zip(register.read_poses(register.poses_path(again)), out["poses"])):
        moved = _apart({"R": e["pose"][:3, :3], "t": e["pose"][:3, 3]}, r, scans[k][0]) / VOXEL
        assert moved <= 5e-3, (k, moved, e["iterations"])
    # a scan that cannot be matched is named, and nothing is written
    lost = str(tmp_path / "lost.ply")
    write_ply_colors(lost, scans[2][0] + 0.5, scans[2][1])
    with pytest.raises(SystemExit, match="lost.ply"):
        register.main(["--input", names[0], lost, "--output", str(tmp_path / "bad.ply"), "--voxel_size", repr(VOXEL), "--estimate_normals"])
    assert not os.path.exists(str(tmp_path / "bad.ply"))
