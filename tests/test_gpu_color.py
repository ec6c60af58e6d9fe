"""Colours on the device (csrc/color.hip): pcgc_recolor bit for bit against the numpy statement of the rule
(tests/_color_ref.py), metrics.color_metrics against the pc_error binary's printed values and against numpy, the off-grid
rule, test.py --colors_from and eval --color."""
import csv
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _color_ref as ref                                                 # noqa: E402
from _clouds import dense as _dense, faces as _faces                     # noqa: E402
from pcgcv1_amd import _lib, metrics, synthetic                          # noqa: E402
from pcgcv1_amd import recolor as rc                                     # noqa: E402
from pcgcv1_amd.dataprocess import inout_points as iop                   # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _lib.require_gpu()


def _cases():
    out = {}
    s, c = _dense(1, 12, 700)
    out["dense_ties"] = (s, c, _dense(2, 12, 500)[0], 12)
    s, c = _dense(3, 20, 1500)
    out["dense_ties_more_targets"] = (s, c, _dense(4, 20, 2500)[0], 20)
    # a sparse source and a dense target: most targets are chosen by no source point (forward branch)
    s, c = _dense(5, 24, 60)
    out["forward_branch"] = (s, c, _dense(6, 24, 2000)[0], 24)
    out["one_source"] = (np.array([[3, 4, 5]], np.int32), np.array([[7, 8, 9]], np.uint8), _dense(7, 16, 300)[0], 16)
    s, c = _dense(8, 16, 300)
    out["one_target"] = (s, c, np.array([[15, 0, 7]], np.int32), 16)
    out["one_each"] = (np.array([[0, 0, 0]], np.int32), np.array([[255, 0, 1]], np.uint8), np.array([[9, 9, 9]], np.int32), 10)
    s, c = _dense(9, 32, 2000)
    out["identity"] = (s, c, s[::-1].copy(), 32)
    s, c = _faces(10, 64, 1500)
    out["faces_res64"] = (s, c, _faces(11, 64, 1200)[0], 64)
    s, c = _faces(12, 1024, 1500)
    out["faces_res1024"] = (s, c, _faces(13, 1024, 1200)[0], 1024)
    return out


CASES = _cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_recolor_bit_exact_against_the_numpy_rule(name):
    s, c, t, res = CASES[name]
    want_c, want_n = ref.recolor(s, c, t)
    got_c, got_n = rc.recolor(s, c, t, res, return_counts=True)
    assert got_c.dtype == np.uint8 and got_c.shape == (len(t), 3)
    assert np.array_equal(got_n, want_n), (name, int((got_n != want_n).sum()))
    assert np.array_equal(got_c, want_c), (name, int((got_c != want_c).any(1).sum()))
    if name == "forward_branch":
        assert (want_n == 0).sum() > len(t) // 2
    if name.startswith("dense_ties"):
        assert (want_n > 1).sum() > len(t) // 10
    if name == "identity":
        assert np.array_equal(got_c, c[::-1]) and (got_n == 1).all()
    again = rc.recolor(s, c, t, res, return_counts=True)
    assert again[0].tobytes() == got_c.tobytes() and again[1].tobytes() == got_n.tobytes()


def test_recolor_default_resolution_and_input_checks():
    s, c, t, res = CASES["dense_ties"]
    assert np.array_equal(rc.recolor(s, c, t), ref.recolor(s, c, t)[0])
    with pytest.raises(ValueError, match="duplicate"):
        rc.recolor(np.concatenate([s, s[:1]]), np.concatenate([c, c[:1]]), t)
    with pytest.raises(ValueError, match="uint8"):
        rc.recolor(s, c.astype(np.int32), t)
    with pytest.raises(ValueError, match="within"):
        rc.recolor(s, c, t, resolution=4)


def test_recolor_larger_cloud_is_repeatable_and_spot_checked():
    """~10^5 points at res 256: two runs give the same bytes, and a sample of targets agrees with the brute-force rule
    restricted to the source points that can matter (|B(t)| and the colours of 300 targets against all sources)."""
    pts = synthetic.make_cloud(seed=3, res=256, n_shells=1, rmin=0.2, rmax=0.4).astype(np.int32)
    rng = np.random.default_rng(0)
    col = rng.integers(0, 256, (len(pts), 3)).astype(np.uint8)
    keep = rng.random(len(pts)) > 0.2
    t = np.unique(np.clip(pts[keep] + rng.integers(-1, 2, (int(keep.sum()), 3)) * (rng.random((int(keep.sum()), 3)) < 0.3), 0, 255), axis=0).astype(np.int32)
    got_c, got_n = rc.recolor(pts, col, t, 256, return_counts=True)
    again = rc.recolor(pts, col, t, 256, return_counts=True)
    assert again[0].tobytes() == got_c.tobytes() and again[1].tobytes() == got_n.tobytes()
    assert int(got_n.sum()) >= len(pts)                       # every source point chose at least one target
    # brute force around one target: the sources within 10 cells of it and the targets within 20 decide the targets within 5
    # (a source's nearest target is a few cells away: the target cloud is the source with points dropped and jittered by one)
    centre = t[len(t) // 2]
    inner = np.abs(t - centre).max(1) <= 5
    near_t = np.abs(t - centre).max(1) <= 20
    near_s = np.abs(pts - centre).max(1) <= 10
    assert inner.sum() > 20 and near_s.sum() < 6000 and near_t.sum() < 6000
    assert metrics.d1_metrics(pts, t, 255)["h.       1(p2point)"] <= 25          # no source is farther than 5 from the targets
    want_c, want_n = ref.recolor(pts[near_s], col[near_s], t[near_t])
    sel = inner[near_t]
    assert np.array_equal(got_n[near_t][sel], want_n[sel]) and np.array_equal(got_c[near_t][sel], want_c[sel])


def test_off_grid_targets_share_their_cells_colour():
    s, c = _dense(21, 40, 3000)
    grid = _dense(22, 25, 1500)[0]
    t = (grid.astype(np.float32) / np.float32(0.625)).astype(np.float32)        # a scale = 5/8 reconstruction scaled back
    t = np.concatenate([t, t[:50] + np.float32(0.2), [[-3.0, 2.0, 100.0]]]).astype(np.float32)
    res = 40
    want = ref.recolor_off_grid(s, c, t, res)
    got = rc.recolor(s, c, t, res)
    assert np.array_equal(got, want)
    cells = np.clip(np.rint(t.astype(np.float64)), 0, res - 1)
    _, inv, counts = np.unique(cells, axis=0, return_inverse=True, return_counts=True)
    assert counts.max() > 1                                   # some targets do share a cell
    for k in np.flatnonzero(counts > 1)[:20]:
        assert len(np.unique(got[inv.reshape(-1) == k], axis=0)) == 1


def test_color_metrics_against_pc_error_and_numpy(golden):
    """metrics.color_metrics against what `pc_error --color=1` printed (mse within 1e-5 relative, PSNR within 1e-3) and
    against the numpy statement to 1e-12 relative (float64 sums in another order)."""
    g = golden("pc_error_color.npz")
    keys = [str(k) for k in g["keys"]]
    for i in range(int(g["n_cases"])):
        a, ca, b, cb = g["a%d" % i], g["ca%d" % i], g["b%d" % i], g["cb%d" % i]
        m = metrics.color_metrics(a, ca, b, cb)
        r = ref.color_metrics(a, ca, b, cb)
        assert sorted(m) == sorted(keys)
        for key, val in zip(keys, g["vals%d" % i]):
            val = float(val)
            print(i, key, m[key], r[key], val)
            if "PSNR" in key:
                assert m[key] == val or abs(m[key] - val) < 1e-3, (i, key, m[key], val)
                assert m[key] == r[key] or abs(m[key] - r[key]) <= 1e-12 * abs(r[key]), (i, key, m[key], r[key])
            else:
                assert abs(m[key] - val) <= 1e-5 * abs(val), (i, key, m[key], val)
                assert abs(m[key] - r[key]) <= 1e-12 * abs(r[key]), (i, key, m[key], r[key])
        assert metrics.color_metrics(a, ca, b, cb) == m       # fixed-order sums: the same bits again
    a, ca, b, cb = g["a0"], g["ca0"], g["b0"], g["cb0"]
    both = metrics.pc_error(a, b, None, 11, colors_a=ca, colors_b=cb)
    plain = metrics.pc_error(a, b, None, 11)
    assert {k: both[k] for k in plain} == plain and all(both[k] == v for k, v in metrics.color_metrics(a, ca, b, cb).items())
    assert not any(k.startswith("c[") for k in plain)
    with pytest.raises(ValueError):
        metrics.pc_error(a, b, None, 11, colors_a=ca)


def _coloured_cloud():
    pts = synthetic.make_cloud(seed=5, res=128, n_shells=3, rmin=0.2, rmax=0.4).astype(np.int32)
    t = pts.astype(np.float64) / 128
    col = np.stack([128 + 100 * np.sin(7 * t[:, 0] + 3 * t[:, 1]), 128 + 100 * np.cos(5 * t[:, 1] - 2 * t[:, 2]), 255 * t[:, 2]], -1)
    col = np.clip(np.rint(col + np.random.default_rng(5).normal(0, 10, col.shape)), 0, 255).astype(np.uint8)
    return pts, col


def test_cli_colors_from(tmp_path, monkeypatch, capsys):
    from pcgcv1_amd import test as cli
    pts, col = _coloured_cloud()
    ply = tmp_path / "col_vox7.ply"
    iop.write_ply_colors(str(ply), pts, col)
    monkeypatch.chdir(tmp_path)
    cli.main(["compress", str(ply), "--ckpt_dir=synthetic:7:sparse", "--min_num=20"])
    cli.main(["decompress", "compressed/col_vox7", "plain_rec.ply", "--ckpt_dir=synthetic:7:sparse"])
    cli.main(["decompress", "compressed/col_vox7", "colour_rec.ply", "--ckpt_dir=synthetic:7:sparse", "--colors_from", str(ply)])
    plain = iop.load_ply_data(str(tmp_path / "plain_rec.ply"))
    rec_p, rec_c = iop.load_ply_colors(str(tmp_path / "colour_rec.ply"))
    assert rec_c is not None and np.array_equal(rec_p, plain)
    assert np.array_equal(rec_c, rc.recolor(pts, col, rec_p))
    assert len(rec_p) > 1000
    # without the flag: exactly the parent's writer on the same points
    iop.write_ply_data(str(tmp_path / "writer.ply"), plain.astype("int"))
    assert (tmp_path / "plain_rec.ply").read_bytes() == (tmp_path / "writer.ply").read_bytes()
    assert iop.load_ply_colors(str(tmp_path / "plain_rec.ply"))[1] is None
    # the module's own command line writes the same file as --colors_from
    rc.main(["--source", str(ply), "--target", "plain_rec.ply", "--output", "tool_rec.ply"])
    assert (tmp_path / "tool_rec.ply").read_bytes() == (tmp_path / "colour_rec.ply").read_bytes()
    plain_ply = tmp_path / "nocolour.ply"
    iop.write_ply_data(str(plain_ply), pts)
    with pytest.raises(SystemExit, match="nocolour.ply"):
        cli.main(["decompress", "compressed/col_vox7", "x_rec.ply", "--ckpt_dir=synthetic:7:sparse", "--colors_from", str(plain_ply)])


def test_eval_color(tmp_path):
    from pcgcv1_amd import eval as pe
    from pcgcv1_amd import eval_ablation_studies as pa
    from pcgcv1_amd.models import model_voxception as model
    pts, col = _coloured_cloud()
    ply = tmp_path / "col_vox7.ply"
    iop.write_ply_colors(str(ply), pts, col)
    body = "[DEFAULT]\ncube_size = 64\nmin_num = 20\n\n[R1]\nscale = 1.0\nckpt_dir = synthetic:7:sparse\nrho_d1 = 1.1\nrho_d2 = 1.0\n"
    ini = tmp_path / "cfg.ini"
    ini.write_text(body)
    rows_plain = pe.eval(str(ply), str(tmp_path / "plain"), str(ini), 128)
    rows = pe.eval(str(ply), str(tmp_path / "colour"), str(ini), 128, color=True)
    new = ["c[0],PSNRF", "c[1],PSNRF", "c[2],PSNRF", "optimal D1 c[0],PSNRF"]
    with open(tmp_path / "plain" / "col_vox7.csv") as f:
        head_plain = next(csv.reader(f))
    with open(tmp_path / "colour" / "col_vox7.csv") as f:
        head = next(csv.reader(f))
    # today's columns: the pc_error keys of a cloud without normals, then eval's own (eval.py)
    today = list(metrics.pc_error(pts, pts, None, 127)) + ["ori_points", "scale", "bpp", "bpp_strings", "bpp_strings_hyper",
                                                          "bpp_strings_head", "bpp_pointsnums", "bpp_cubepos", "rho_d1",
                                                          "optimal D1 PSNR", "rho_d2", "optimal D2 PSNR", "rate"]
    assert head_plain == today and head == today + new
    assert {k: rows[0][k] for k in today if k not in ("optimal D2 PSNR",)} == {k: rows_plain[0][k] for k in today if k not in ("optimal D2 PSNR",)}
    # the colour keys are those of the recoloured reconstructions
    cubes_d, cube_positions, points_numbers, n, _ = pe.rate_point(pts, model, "synthetic:7:sparse", 1.0, 64, 20)
    for rho, keys in ((1.0, new[:3]), (1.1, new[3:])):
        rec = pe.postprocess_points(cubes_d, points_numbers, cube_positions, 1.0, 64, rho, None)
        rec = np.unique(np.rint(rec).astype(np.int32), axis=0)
        want = metrics.color_metrics(pts, col, rec, rc.recolor(pts, col, rec))
        for k in keys:
            assert rows[0][k] == want[k.replace("optimal D1 ", "")] and np.isfinite(rows[0][k]), k
    plain_ply = tmp_path / "nocolour.ply"
    iop.write_ply_data(str(plain_ply), pts)
    with pytest.raises(ValueError, match="nocolour.ply"):
        pe.eval(str(plain_ply), str(tmp_path / "colour"), str(ini), 128, color=True)
    assert pa.main is not None and "color" in pa.eval.__code__.co_varnames
