"""Encoder-side point counts on the device (csrc/pointnums.hip, pcgcv1_amd/pointnums.py): the curves and the sweep exactly
against the numpy restatement (tests/_pointnums_ref.py), on engineered cubes and on real cubes of the synthetic cloud
under the a6 checkpoint, then `test.py compress --pointnums d1` + `decompress` end to end (hyper and factorized)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _pointnums_ref as ref                                             # noqa: E402
from test_pointnums_host import big_k_cube, engineered_cubes             # noqa: E402
from pcgcv1_amd import _lib, pointnums as pn, synthetic                  # noqa: E402
from pcgcv1_amd.dataprocess import inout_bitstream as bs                 # noqa: E402
from pcgcv1_amd.dataprocess import inout_points as iop                   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CKPT = os.path.join(ROOT, "checkpoints", "hyper", "a6.00b3.00")
NAMES = ("strings", "strings_head", "strings_hyper", "pointnums", "cubepos")


@pytest.fixture(scope="module")
def cloud():
    """the synthetic cloud, its cubes and the encoder-side logits under the a6 checkpoint"""
    from pcgcv1_amd.models import model_voxception as model
    from pcgcv1_amd.process import preprocess_points
    from pcgcv1_amd.transform import compress_hyper
    _lib.require_gpu()
    pts = synthetic.make_cloud(1300)
    cubes, pos, nums = preprocess_points(pts, 1.0, 64, 64)
    out = compress_hyper(cubes, model, CKPT, decompress=True)
    return pts, cubes, pos, nums, out[8]


def _split(m, A, B, off):
    m, A, B = m.cpu().numpy(), A.cpu().numpy(), B.cpu().numpy()
    return [(m[a:b], A[a:b], B[a:b]) for a, b in zip(off[:-1], off[1:])]


def _check_curves(xs, ls, ns):
    m, A, B, off = pn.distortion_curves(xs, ls, ns)
    got = _split(m, A, B, off)
    want = [ref.curves_ref(x, l, n) for x, l, n in zip(xs, ls, ns)]
    for b, (g, w) in enumerate(zip(got, want)):
        for q in range(3):
            np.testing.assert_array_equal(g[q], w[q], err_msg="cube %d, curve %d" % (b, q))
    return (m, A, B, off), want


def _check_sweep(dev_curves, want, ns):
    m, A, B, off = dev_curves
    lad = pn.ladder_counts(ns, np.diff(off), pn.RHOS_D1)
    k, s = pn.sweep_curves(m, A, B, off, 64, lad)
    k_ref, s_ref = ref.sweep_ref(want, 64, lad)
    np.testing.assert_array_equal(k, k_ref)
    np.testing.assert_array_equal(s, s_ref)


def test_curves_and_sweep_engineered():
    cases = engineered_cubes()
    xs = np.stack([c[1] for c in cases])[..., None]
    ls = np.stack([c[2] for c in cases])[..., None]
    ns = np.array([c[3] for c in cases], np.uint16)
    dev, want = _check_curves(xs, ls, ns)
    _check_sweep(dev, want, ns)


def test_curves_big_k():
    x, l, n = big_k_cube()
    dev, want = _check_curves(x[None, ..., None], l[None, ..., None], np.array([n], np.uint16))
    assert len(want[0][0]) == 65535
    _check_sweep(dev, want, np.array([n], np.uint16))


def test_curves_and_sweep_real_cubes(cloud):
    _, cubes, _, nums, logits = cloud
    order = np.argsort(nums.astype(np.int64), kind="stable")
    pick = sorted({int(order[0]), int(order[len(order) // 2]), int(order[-1])})      # smallest, median, largest cube
    xs = cubes[pick].cpu().numpy()
    ls = logits[pick].cpu().numpy()
    dev, want = _check_curves(xs, ls, nums[pick])
    _check_sweep(dev, want, nums[pick])


def _run_cli(args, cwd):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-m", "pcgcv1_amd.test"] + args, cwd=cwd, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def _per_cube(points, pos, cs=64):
    """points of a decoded cloud -> {cube index: local coordinates}"""
    where = {tuple(int(v) for v in p): i for i, p in enumerate(pos)}
    cube = points // cs
    out = {}
    keys = [where[tuple(int(v) for v in c)] for c in cube]
    keys = np.asarray(keys)
    for i in np.unique(keys):
        out[int(i)] = points[keys == i] - np.asarray(pos[i]) * cs
    return out


def test_cli_hyper_end_to_end(cloud, tmp_path):
    pts, cubes, pos, nums, logits = cloud
    ply = str(tmp_path / "cloud.ply")
    iop.write_ply_data(ply, pts)
    ck = ["--ckpt_dir=" + CKPT]
    _run_cli(["compress", ply, "cnt"] + ck, str(tmp_path))
    out = _run_cli(["compress", ply, "d1", "--pointnums", "d1"] + ck, str(tmp_path))
    assert "pointnums d1: chose" in out
    comp = str(tmp_path / "compressed")
    for k in NAMES:
        a = open(os.path.join(comp, "cnt." + k), "rb").read()
        b = open(os.path.join(comp, "d1." + k), "rb").read()
        if k == "pointnums":
            assert len(a) == len(b)
        else:
            assert a == b, k
    _run_cli(["decompress", os.path.join(comp, "d1"), str(tmp_path / "d1_rec.ply"), "--rho", "1"] + ck, str(tmp_path))
    r = bs.read_binary_files_hyper("d1", comp)
    k_file = np.asarray(r[2]).astype(np.int64)
    spos = iop.ordered_positions(np.asarray(r[3]))                          # the cubes' positions in stored order

    counts, rep = pn.optimize_points_numbers(cubes, logits, nums)
    np.testing.assert_array_equal(counts.astype(np.int64), k_file)            # the CLI wrote what the optimiser picks
    m, A, B, off = pn.distortion_curves(cubes, logits, nums)
    curves = _split(m, A, B, off)
    rec = iop.load_ply_data(str(tmp_path / "d1_rec.ply"))
    dec = _per_cube(rec, spos)
    for b in range(len(nums)):                                                # every cube: decoded count = m_b(k_b)
        assert len(dec.get(b, ())) == int(curves[b][0][k_file[b] - 1]), b
    order = np.argsort(nums.astype(np.int64), kind="stable")
    xs = cubes.cpu().numpy()
    for b in sorted({int(order[0]), int(order[1]), int(order[len(order) // 2]), int(order[-2]), int(order[-1])}):
        P = np.argwhere(xs[b, ..., 0] > 0).astype(np.int64)
        V = dec[b].astype(np.int64)
        D = ((P[:, None, :] - V[None, :, :]) ** 2).sum(-1)
        assert int(D.min(1).sum()) == int(curves[b][1][k_file[b] - 1]), b
        assert int(D.min(0).sum()) == int(curves[b][2][k_file[b] - 1]), b

    sum_n = rep["sum_n"]
    assert sum_n == int(nums.astype(np.int64).sum())
    f = pn.cloud_f(*(lambda s: (s[0], sum_n, s[1], s[2]))(rep["sums"][rep["choice"]]))
    for rho in pn.RHOS_D1:
        s = rep["sums"][("ladder", rho)]
        assert f <= pn.cloud_f(s[0], sum_n, s[1], s[2]), rho
    assert rep["F_chosen"] <= rep["F_count"]


def test_cli_factorized_small(tmp_path):
    from pcgcv1_amd.models import model_voxception as model
    from pcgcv1_amd.process import preprocess_points
    from pcgcv1_amd.transform import compress_factorized, decompress_factorized
    pts = synthetic.make_cloud(7, res=256, n_shells=1, rmin=0.1, rmax=0.14)
    ply = str(tmp_path / "small.ply")
    iop.write_ply_data(ply, pts)
    ck = ["--mode", "factorized", "--ckpt_dir", "synthetic"]
    _run_cli(["compress", ply, "f"] + ck + ["--pointnums", "d1"], str(tmp_path))
    _run_cli(["decompress", os.path.join(str(tmp_path / "compressed"), "f"), str(tmp_path / "f_rec.ply")] + ck, str(tmp_path))
    strings, k_file, pos, *_ = bs.read_binary_files_factorized("f", str(tmp_path / "compressed"))
    cubes, pos2, nums = preprocess_points(pts, 1.0, 64, 64)
    assert 1 <= len(nums) <= 40
    s, mn, mx, sh = compress_factorized(cubes, model, "synthetic")
    logits = decompress_factorized(s, mn, mx, sh, model, "synthetic")
    counts, rep = pn.optimize_points_numbers(cubes, logits, nums)
    np.testing.assert_array_equal(counts.astype(np.int64), np.asarray(k_file).astype(np.int64))
    m, A, B, off = pn.distortion_curves(cubes, logits, nums)
    curves = _split(m, A, B, off)
    dec = _per_cube(iop.load_ply_data(str(tmp_path / "f_rec.ply")), iop.ordered_positions(np.asarray(pos)))
    for b in range(len(nums)):
        assert len(dec.get(b, ())) == int(curves[b][0][int(k_file[b]) - 1]), b
    assert rep["F_chosen"] <= rep["F_count"]
