"""`--pointnums d2` on the device (csrc/pointnums.hip, pcgcv1_amd/pointnums.py): the point-to-plane curves and the sweep exactly
against the numpy definition (tests/_pointnums_d2_ref.py) on engineered 8^3 and 16^3 cubes, across chunks, and on real cubes of
the synthetic cloud under the a6 checkpoint; the voxel normals; the optimiser's guarantees; `metric="d1"` unchanged; the CLI."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _pointnums_d2_ref as ref2                                          # noqa: E402
import _pointnums_ref as ref                                              # noqa: E402
from test_pointnums_d2_host import engineered_cubes_d2, tiled_cubes_d2    # noqa: E402
from pcgcv1_amd import _lib, metrics, pointnums as pn, synthetic          # noqa: E402
from pcgcv1_amd.dataprocess import inout_bitstream as bs                  # noqa: E402
from pcgcv1_amd.dataprocess import inout_points as iop                    # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CKPT = os.path.join(ROOT, "checkpoints", "hyper", "a6.00b3.00")
NAMES = ("strings", "strings_head", "strings_hyper", "pointnums", "cubepos")


@pytest.fixture(scope="module")
def cloud():
    """the synthetic cloud with estimated normals, its cubes, the encoder-side logits under the a6 checkpoint, the voxel normals"""
    from pcgcv1_amd.models import model_voxception as model
    from pcgcv1_amd.process import preprocess_points
    from pcgcv1_amd.transform import compress_hyper
    _lib.require_gpu()
    pts = synthetic.make_cloud(1300)
    normals = metrics.estimate_normals(pts, 10, 20)
    cubes, pos, nums = preprocess_points(pts, 1.0, 64, 64)
    out = compress_hyper(cubes, model, CKPT, decompress=True)
    vn = pn.voxel_normals(pts, normals, pos, 1.0, 64)
    return {"pts": pts, "normals": normals, "cubes": cubes, "pos": pos, "nums": nums, "logits": out[8], "vn": vn}


def _vn16(nq):
    out = np.zeros((len(nq), 4), np.int16)
    out[:, :3] = nq
    return out


def _split(m, A, B, off):
    m, A, B = m.cpu().numpy(), A.cpu().numpy(), B.cpu().numpy()
    return [(m[a:b], A[a:b], B[a:b]) for a, b in zip(off[:-1], off[1:])]


def _check_curves(xs, ls, ns, nqs):
    """device curves of the batch (nqs: per cube, int [N_b, 3]) against the fast numpy form, exactly"""
    vn = _vn16(np.concatenate([np.asarray(q).reshape(-1, 3) for q in nqs]))
    m, A, B, off = pn.distortion_curves_d2(xs, ls, ns, vn)
    got = _split(m, A, B, off)
    want = [ref2.curves_d2_ref(x, l, n, q) for x, l, n, q in zip(xs, ls, ns, nqs)]
    for b, (g, w) in enumerate(zip(got, want)):
        for q in range(3):
            np.testing.assert_array_equal(g[q], w[q], err_msg="cube %d, curve %d" % (b, q))
    return (m, A, B, off), want


def _check_sweep(dev_curves, want, ns):
    m, A, B, off = dev_curves
    lad = pn.ladder_counts(ns, np.diff(off), pn.RHOS_D2)
    k, s = pn.sweep_curves(m, A, B, off, 64, lad)
    k_ref, s_ref = ref.sweep_ref(want, 64, lad)
    np.testing.assert_array_equal(k, k_ref)
    np.testing.assert_array_equal(s, s_ref)


def _batch(cases):
    xs = np.stack([c[1] for c in cases])[..., None]
    ls = np.stack([c[2] for c in cases])[..., None]
    ns = np.array([c[3] for c in cases], np.uint16)
    return xs, ls, ns, [ref2.quantise_normals(c[4]) for c in cases]


@pytest.mark.parametrize("part", ["8a", "8b", "16"])
def test_curves_and_sweep_engineered(part):
    cases = engineered_cubes_d2()
    assert len(cases) == 8
    cases = {"8a": cases[:4], "8b": cases[4:], "16": tiled_cubes_d2()}[part]          # 4, 4 and 3 cubes share a launch
    xs, ls, ns, nqs = _batch(cases)
    if part == "16":
        p = pn._Prepared(xs, ls, ns)
        assert (p.n_pts > 256).all() and (p.n_seg > 256).all()                       # both lists span several tiles
    dev, want = _check_curves(xs, ls, ns, nqs)
    _check_sweep(dev, want, ns)


def test_curves_across_chunks(monkeypatch):
    xs, ls, ns, nqs = _batch(tiled_cubes_d2(count=4))
    whole = pn.distortion_curves_d2(xs, ls, ns, _vn16(np.concatenate(nqs)))
    seg = pn._Prepared(xs, ls, ns).n_seg
    monkeypatch.setattr(pn, "_CHUNK_SEG", int(seg[0] + seg[1]))                       # two cubes fit, a third does not
    p = pn._Prepared(xs, ls, ns, _vn16(np.concatenate(nqs)))
    assert len(p.chunks) >= 2 and p.chunks[0] == (0, 2)
    dev, want = _check_curves(xs, ls, ns, nqs)
    for q in range(3):
        np.testing.assert_array_equal(dev[q].cpu().numpy(), whole[q].cpu().numpy())
    vn = _vn16(np.concatenate(nqs))
    counts_c, rep_c = pn.optimize_points_numbers(xs, ls, ns, metric="d2", normals=vn)
    monkeypatch.undo()
    counts, rep = pn.optimize_points_numbers(xs, ls, ns, metric="d2", normals=vn)
    np.testing.assert_array_equal(counts_c, counts)
    assert rep_c["sums"] == rep["sums"] and rep_c["choice"] == rep["choice"]


def _voxel_normal_slices(c):
    off = np.concatenate([[0], np.cumsum(c["nums"].astype(np.int64))])
    vn = c["vn"].cpu().numpy()
    return lambda b: vn[off[b]:off[b + 1], :3].astype(np.int64)


def test_curves_and_sweep_real_cubes(cloud):
    nums = cloud["nums"]
    order = np.argsort(nums.astype(np.int64), kind="stable")
    pick = sorted({int(order[0]), int(order[len(order) // 2]), int(order[-1])})      # smallest, median, largest cube
    xs = cloud["cubes"][pick].cpu().numpy()
    ls = cloud["logits"][pick].cpu().numpy()
    nq_of = _voxel_normal_slices(cloud)
    dev, want = _check_curves(xs, ls, nums[pick], [nq_of(b) for b in pick])
    _check_sweep(dev, want, nums[pick])


def _check_voxel_normals(pts, normals, scale):
    from pcgcv1_amd.process import preprocess_points
    cubes, pos, nums = preprocess_points(pts, scale, 64, 64)
    keys = pn.point_keys(pts, pos, scale, 64)
    x = cubes.reshape(len(nums), -1).cpu().numpy()
    kept = keys >= 0
    assert kept.any()
    assert (x[keys[kept] // 64 ** 3, keys[kept] % 64 ** 3] > 0).all()                 # every point lands on an occupied voxel
    uniq, want = ref2.voxel_normals_ref(keys, normals)
    np.testing.assert_array_equal(uniq, np.flatnonzero(x.reshape(-1) > 0))            # and every occupied voxel has a point
    got = pn.voxel_normals(pts, normals, pos, scale, 64).cpu().numpy()
    assert got.dtype == np.int16 and got.shape == (int(nums.astype(np.int64).sum()), 4)
    np.testing.assert_array_equal(got[:, :3], want)
    assert not got[:, 3].any()
    return keys, uniq


def test_voxel_normals_scale_1(cloud):
    nrm = cloud["normals"].copy()
    nrm[:7] = [[0, 0, 0], [np.nan, 0, 1], [np.inf, 1, 0], [0, 0, -3], [3, 4, 0], [1e-20, 0, 0], [-1, -1, -1]]
    keys, uniq = _check_voxel_normals(cloud["pts"], nrm, 1.0)
    assert len(uniq) == int((keys >= 0).sum())                                        # a voxelised cloud: one to one


def test_voxel_normals_scale_half(cloud):
    keys, uniq = _check_voxel_normals(cloud["pts"], cloud["normals"], 0.5)
    assert len(uniq) < int((keys >= 0).sum()) // 2                                    # several points share a voxel


def _f(s, sum_n):
    return pn.cloud_f(s[0], sum_n, s[1], s[2])


def test_optimiser_guarantees(cloud):
    cubes, logits, nums = cloud["cubes"], cloud["logits"], cloud["nums"]
    counts, rep = pn.optimize_points_numbers(cubes, logits, nums, metric="d2", normals=cloud["vn"])
    sum_n = rep["sum_n"]
    assert sum_n == int(nums.astype(np.int64).sum())
    assert [k for k in rep["sums"] if k[0] == "ladder"] == [("ladder", r) for r in pn.RHOS_D2]
    f = _f(rep["sums"][rep["choice"]], sum_n)
    for rho in pn.RHOS_D2:
        assert f <= _f(rep["sums"][("ladder", rho)], sum_n), rho
    assert rep["F_chosen"] <= rep["F_count"]
    assert rep["F_chosen"] == float(f / 1024 ** 2)
    # every assignment's sums are the device curves at its counts ...
    m, A, B, off = pn.distortion_curves_d2(cubes, logits, nums, cloud["vn"])
    m, A, B = m.cpu().numpy(), A.cpu().numpy(), B.cpu().numpy()
    rows = {("sweep", j): j for j in range(65)}
    rows.update({("ladder", r): 65 + i for i, r in enumerate(pn.RHOS_D2)})
    for key in (rep["choice"], ("ladder", 1.0), ("ladder", 0.3), ("sweep", 0), ("sweep", 64)):
        at = off[:-1] + rep["ks"][rows[key]] - 1
        assert rep["sums"][key] == (int(A[at].sum()), int(B[at].sum()), int(m[at].sum())), key
    np.testing.assert_array_equal(counts.astype(np.int64), rep["ks"][rows[rep["choice"]]])
    np.testing.assert_array_equal(rep["ks"][rows[("ladder", 1.0)]], nums.astype(np.int64))
    # ... and those entries are what the decoder's own masks give, measured from scratch, on three cubes
    order = np.argsort(nums.astype(np.int64), kind="stable")
    nq_of = _voxel_normal_slices(cloud)
    for b in sorted({int(order[0]), int(order[len(order) // 4]), int(order[len(order) // 2])}):
        x, l = cubes[b].cpu().numpy(), logits[b].cpu().numpy()
        ks = sorted({int(counts[b]), int(nums[b]), int(rep["ks"][rows[("ladder", 0.3)]][b])})
        direct = ref2.curves_d2_direct(x, l, ks, nq_of(b))
        for k, d in zip(ks, direct):
            at = off[b] + k - 1
            assert (int(m[at]), int(A[at]), int(B[at])) == d, (b, k)


def test_d1_unchanged(cloud):
    """metric="d1" is the default and gives what the D1 pieces give: curves, sweep over RHOS_D1, selection"""
    cubes, logits, nums = cloud["cubes"], cloud["logits"], cloud["nums"]
    counts, rep = pn.optimize_points_numbers(cubes, logits, nums)
    counts1, rep1 = pn.optimize_points_numbers(cubes, logits, nums, metric="d1")
    np.testing.assert_array_equal(counts, counts1)
    assert rep["sums"] == rep1["sums"] and rep["choice"] == rep1["choice"] and rep["F_chosen"] == rep1["F_chosen"]
    m, A, B, off = pn.distortion_curves(cubes, logits, nums)
    lad = pn.ladder_counts(nums, np.diff(off), pn.RHOS_D1)
    k, s = pn.sweep_curves(m, A, B, off, 64, lad)
    sums = [tuple(int(v) for v in r) for r in s]
    kind, i, f = pn.select_assignment(sums[:65], sums[65:], pn.RHOS_D1, int(nums.astype(np.int64).sum()))
    np.testing.assert_array_equal(counts.astype(np.int64), k[i if kind == "sweep" else 65 + i])
    assert rep["choice"] == (kind, i if kind == "sweep" else pn.RHOS_D1[i]) and rep["F_chosen"] == float(f)
    assert [rep["sums"][("sweep", j)] for j in range(65)] == sums[:65]
    assert [rep["sums"][("ladder", r)] for r in pn.RHOS_D1] == sums[65:]
    order = np.argsort(nums.astype(np.int64), kind="stable")                          # the curves against the D1 definition
    b = int(order[len(order) // 2])
    want = ref.curves_ref(cubes[b].cpu().numpy(), logits[b].cpu().numpy(), nums[b])
    for q, t in enumerate((m, A, B)):
        np.testing.assert_array_equal(t[off[b]:off[b + 1]].cpu().numpy(), want[q])


def _run_cli(args, cwd, ok=True):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-m", "pcgcv1_amd.test"] + args, cwd=cwd, env=env, capture_output=True, text=True,
                       timeout=600)
    if ok:
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def _per_cube(points, pos, cs=64):
    """points of a decoded cloud -> {cube index: number of points}"""
    where = {tuple(int(v) for v in p): i for i, p in enumerate(pos)}
    keys = np.asarray([where[tuple(int(v) for v in c)] for c in points // cs])
    return {int(i): int((keys == i).sum()) for i in np.unique(keys)}


def _small_cloud():
    return synthetic.make_cloud(7, res=256, n_shells=1, rmin=0.1, rmax=0.14)


def test_cli_hyper(tmp_path):
    from pcgcv1_amd.models import model_voxception as model
    from pcgcv1_amd.process import preprocess_points
    from pcgcv1_amd.transform import compress_hyper
    pts = _small_cloud()
    ply = str(tmp_path / "cloud.ply")
    iop.write_ply_normals(ply, pts, metrics.estimate_normals(pts, 10, 20))
    pts_f, normals = iop.load_ply_normals(ply)                                        # the normals as the file holds them
    np.testing.assert_array_equal(pts_f, pts)
    ck = ["--ckpt_dir=" + CKPT]
    _run_cli(["compress", ply, "cnt"] + ck, str(tmp_path))
    out = _run_cli(["compress", ply, "d2", "--pointnums", "d2"] + ck, str(tmp_path)).stdout
    assert "pointnums d2: chose" in out
    comp = str(tmp_path / "compressed")
    for k in NAMES:
        a = open(os.path.join(comp, "cnt." + k), "rb").read()
        b = open(os.path.join(comp, "d2." + k), "rb").read()
        if k == "pointnums":
            assert len(a) == len(b)
        else:
            assert a == b, k
    assert not os.path.exists(os.path.join(comp, "d2.colors"))
    _run_cli(["decompress", os.path.join(comp, "d2"), str(tmp_path / "d2_rec.ply"), "--rho", "1"] + ck, str(tmp_path))
    r = bs.read_binary_files_hyper("d2", comp)
    k_file = np.asarray(r[2]).astype(np.int64)
    spos = iop.ordered_positions(np.asarray(r[3]))

    cubes, pos, nums = preprocess_points(pts, 1.0, 64, 64)
    assert 3 <= len(nums) <= 40
    logits = compress_hyper(cubes, model, CKPT, decompress=True)[8]
    vn = pn.voxel_normals(pts, normals, pos, 1.0, 64)
    counts, rep = pn.optimize_points_numbers(cubes, logits, nums, metric="d2", normals=vn)
    np.testing.assert_array_equal(counts.astype(np.int64), k_file)                    # the CLI wrote what the optimiser picks
    m, A, B, off = pn.distortion_curves_d2(cubes, logits, nums, vn)
    m = m.cpu().numpy()
    dec = _per_cube(iop.load_ply_data(str(tmp_path / "d2_rec.ply")), spos)
    for b in range(len(nums)):                                                        # every cube: decoded count = m_b(k_b)
        assert dec.get(b, 0) == int(m[off[b] + k_file[b] - 1]), b
    assert rep["F_chosen"] <= rep["F_count"]


def test_cli_needs_normals(tmp_path):
    ply = str(tmp_path / "bare.ply")
    iop.write_ply_data(ply, _small_cloud())
    r = _run_cli(["compress", ply, "x", "--pointnums", "d2", "--ckpt_dir=" + CKPT], str(tmp_path), ok=False)
    assert r.returncode != 0
    assert "--estimate_normals" in r.stderr and "nx ny nz" in r.stderr
    assert not os.path.exists(str(tmp_path / "compressed" / "x.pointnums"))


def test_cli_factorized_estimated_normals(tmp_path):
    from pcgcv1_amd.models import model_voxception as model
    from pcgcv1_amd.process import preprocess_points
    from pcgcv1_amd.transform import compress_factorized, decompress_factorized
    pts = _small_cloud()
    ply = str(tmp_path / "bare.ply")
    iop.write_ply_data(ply, pts)
    ck = ["--mode", "factorized", "--ckpt_dir", "synthetic"]
    out = _run_cli(["compress", ply, "f"] + ck + ["--pointnums", "d2", "--estimate_normals"], str(tmp_path)).stdout
    assert "pointnums d2: chose" in out
    strings, k_file, pos_f, *_ = bs.read_binary_files_factorized("f", str(tmp_path / "compressed"))
    cubes, pos, nums = preprocess_points(pts, 1.0, 64, 64)
    s, mn, mx, sh = compress_factorized(cubes, model, "synthetic")
    logits = decompress_factorized(s, mn, mx, sh, model, "synthetic")
    vn = pn.voxel_normals(pts, metrics.estimate_normals(pts, 10, 20), pos, 1.0, 64)
    counts, rep = pn.optimize_points_numbers(cubes, logits, nums, metric="d2", normals=vn)
    np.testing.assert_array_equal(counts.astype(np.int64), np.asarray(k_file).astype(np.int64))
    assert rep["F_chosen"] <= rep["F_count"]
