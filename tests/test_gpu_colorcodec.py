"""The colour codec on the device (csrc/raht.hip, pcgcv1_amd/colorcodec.py) bit for bit against the numpy statement of the rule
(tests/_raht_ref.py): transform, inverse, decoded colours, the file's rate against the reference's empirical entropy, the
command line (compress --colors raht, decompress with <name>.colors) and eval's color_qstep."""
import csv
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _raht_ref as ref                                                  # noqa: E402
import _rans_ref as rans                                                 # noqa: E402
from pcgcv1_amd import _lib, metrics, synthetic                          # noqa: E402
from pcgcv1_amd import colorcodec as cc                                  # noqa: E402
from pcgcv1_amd import recolor as rc                                     # noqa: E402
from pcgcv1_amd.dataprocess import inout_points as iop                   # noqa: E402

STEPS = (1, 2, 4, 8, 16, 32)
# profiles/colorcodec_rd.txt, "test cloud": the largest measured bits / H of the six steps is 1.0951 (step 32), so
# m = 1.0951 - 1 + 0.05
RATE_MARGIN = 0.1451


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _lib.require_gpu()


def _dense(seed, res, n):
    rng = np.random.default_rng(seed)
    p = np.unique(rng.integers(0, res, (n, 3)), axis=0).astype(np.int32)
    p = p[rng.permutation(len(p))]
    return p, rng.integers(0, 256, (len(p), 3)).astype(np.uint8)


def _faces(seed, res, n):
    """as in test_gpu_color.py: a cloud that touches all six faces of the grid"""
    rng = np.random.default_rng(seed)
    axis = np.unique(np.r_[0:res:max(8, res // 8), res - 1])
    lattice = np.stack(np.meshgrid(axis, axis, axis, indexing="ij"), -1).reshape(-1, 3)
    corners = lattice[np.all((lattice == 0) | (lattice == res - 1), 1)]
    moved = lattice + rng.integers(-2, 3, lattice.shape)
    extra = lattice[rng.integers(0, len(lattice), n)] + rng.integers(-3, 4, (n, 3))
    p = np.unique(np.clip(np.concatenate([corners, moved, extra]), 0, res - 1), axis=0).astype(np.int32)
    p = p[rng.permutation(len(p))]
    return p, rng.integers(0, 256, (len(p), 3)).astype(np.uint8)


def _shell():
    p = synthetic.make_cloud(seed=3, res=256, n_shells=1, rmin=0.2, rmax=0.4).astype(np.int32)
    rng = np.random.default_rng(3)
    p = p[rng.permutation(len(p))]
    return p, rng.integers(0, 256, (len(p), 3)).astype(np.uint8)


def _twelve_bit():
    p, c = _dense(14, 4096, 4000)
    p[0] = [4095, 0, 4095]
    p = np.unique(p, axis=0)
    return p, c[:len(p)]


def _cases():
    col = lambda *rows: np.array(rows, np.uint8)                          # noqa: E731
    return {
        "dense_res12": _dense(1, 12, 700),
        "dense_res20": _dense(3, 20, 1500),
        "dense_res32": _dense(9, 32, 20000),
        "one_point": (np.array([[3, 4, 5]], np.int32), col([7, 200, 9])),
        "one_point_origin": (np.array([[0, 0, 0]], np.int32), col([255, 0, 128])),
        "two_siblings": (np.array([[6, 2, 5], [6, 2, 4]], np.int32), col([255, 0, 1], [3, 250, 77])),
        "two_meet_at_root": (np.array([[0, 0, 0], [7, 7, 7]], np.int32), col([10, 20, 30], [200, 100, 0])),
        "shell_res256": _shell(),
        "faces_res1024": _faces(12, 1024, 1500),
        "twelve_bit": _twelve_bit(),
    }


CASES = _cases()


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


@pytest.mark.parametrize("name", sorted(CASES))
def test_transform_bit_identical_to_the_numpy_rule(name):
    p, c = CASES[name]
    a = ref.rgb_to_ycocg(c)
    want_c, want_s, want_w = ref.forward(p, a)
    for fuse in (True, False):                                           # the one-workgroup tree top and the per-level launches
        got_c, got_s, got_w = cc.raht_forward(p, a, fuse_top=fuse)
        assert got_c.dtype == np.float64 and got_s.dtype == np.int32 and got_w.dtype == np.int64
        assert np.array_equal(got_s, want_s) and np.array_equal(got_w, want_w), name
        diff = _bits(got_c) != _bits(want_c)
        assert not diff.any(), (name, fuse, int(diff.sum()), np.abs(got_c - want_c).max())
        back = cc.raht_inverse(p, want_c, fuse_top=fuse)
        want_back = ref.inverse(p, want_c)
        diff = _bits(back) != _bits(want_back)
        assert not diff.any(), (name, fuse, int(diff.sum()), np.abs(back - want_back).max())
    if name == "twelve_bit":
        assert ref.depth_of(p) == 12 and want_s[0] == 36
    if name == "shell_res256":
        assert 50000 < len(p) <= 200000


@pytest.mark.parametrize("name", sorted(CASES))
def test_codec_round_trip_bit_identical_and_within_the_bound(name):
    p, c = CASES[name]
    a = ref.rgb_to_ycocg(c).astype(np.float64)
    for step in STEPS:
        want, q, sub, _ = ref.codec(p, c, step)
        data = cc.encode_colors(p, c, step)
        got = cc.decode_colors(p, data)
        assert got.dtype == np.uint8 and got.shape == (len(p), 3)
        assert np.array_equal(got, want), (name, step, int((got != want).any(1).sum()))
        if step == 4:
            assert cc.encode_colors(p, c, step) == data                  # the same bytes again
            shuffle = np.random.default_rng(0).permutation(len(p))
            assert cc.encode_colors(p[shuffle], c[shuffle], step) == data           # the file does not depend on the row order
            assert np.array_equal(cc.decode_colors(p[shuffle], data), want[shuffle])
        # derived: orthonormal transform, |coef - q step| <= step / 2, rint adds at most 1 / 2 and the clip to the channel's range
        # cannot add (tests/test_colorcodec_host.py); measured on the device's reconstruction before the final rgb clip
        rec = cc.raht_inverse(p, ref.dequantize(q, step))
        ycc = np.rint(rec)
        ycc = np.stack([np.clip(ycc[:, 0], 0, 255), np.clip(ycc[:, 1], -255, 255), np.clip(ycc[:, 2], -255, 255)], -1)
        rms = np.sqrt(((ycc - a) ** 2).mean(0))
        print(name, step, "rms YCoCg", rms, "bytes", len(data))
        assert (rms <= step / 2 + 0.5 + 1e-9).all(), (name, step, rms)
        assert np.array_equal(np.clip(ref.ycocg_to_rgb(ycc.astype(np.int32)), 0, 255), got)


ESCAPE_CLOUDS = dict(CASES, dense_res48=_dense(21, 48, 30000))


@functools.lru_cache(maxsize=None)
def _escape_reference(name, step):
    """the numpy rule's decoded colours and what it hands to the container, as test_gpu_rans._reference builds it, with both
    files: version 1 from colorcodec.pack (tables from the symbols' histogram sums, on the host), version 2 from the reference"""
    p, c = ESCAPE_CLOUDS[name]
    want, q, sub, _ = ref.codec(p, c, step)
    d = ref.depth_of(p)
    counts = np.bincount(sub, minlength=3 * d + 1)
    qg = q[ref.subband_order(sub)]
    n_coded = cc.coded_levels(counts)
    k = int(counts[:n_coded].sum())
    lev = np.repeat(np.arange(n_coded), counts[:n_coded])
    biggest = np.zeros(n_coded, np.int64)
    np.maximum.at(biggest, lev, np.abs(qg[:k]).max(1))
    amax = np.minimum(biggest, cc.AMAX_CAP).astype(np.int32)
    a = amax[lev][:, None]
    inside = np.abs(qg[:k]) <= a
    sym = np.where(inside, qg[:k] + a, 2 * a + 1).astype(np.int16)
    pos = np.flatnonzero(~inside.reshape(-1))
    args = (d, len(p), step, counts, amax, sym, qg[k:], pos, qg[:k].reshape(-1)[pos])
    return want, counts, amax, np.bincount(lev[pos // 3], minlength=n_coded), cc.pack(*args), rans.pack_v2(*args)


@pytest.mark.parametrize("name,step", [("dense_res20", 0.0625), ("dense_res20", 1), ("dense_res32", 0.0625), ("dense_res48", 0.0625)])
def test_escapes_through_the_one_encoder_tail(name, step):
    """Both coders take their tables from pcgc_raht_abs_sums and their escapes from the device-side search; the files must be
    the host's, byte for byte, where escapes are many.  dense_res20 at step 1 / 16: 555 escapes over all 8 coded levels, every
    level at AMAX_CAP; at step 1: none.  An escape inside a rANS level: the level sizes follow from the geometry alone, and
    dense_res32's largest level has 4125 leaves (12 375 symbols < RANS_MIN_SYMBOLS) whatever the step, so that condition is
    asserted on dense_res48 (26 266 points: level 2 is a rANS level between range-coded ones) and dense_res32 keeps the rest."""
    p, c = ESCAPE_CLOUDS[name]
    want, counts, amax, escapes, want_v1, want_v2 = _escape_reference(name, step)
    if name == "dense_res20":
        assert len(p) == 1378 and len(amax) == 8
        if step == 1:
            assert escapes.sum() == 0
        else:
            assert escapes.sum() == 555 and (escapes > 0).all() and (amax == cc.AMAX_CAP).all()
    else:
        assert escapes.sum() > 0
    kinds = cc.level_coders(counts)
    if name == "dense_res48":
        assert any(3 * counts[l] >= cc.RANS_MIN_SYMBOLS and kinds[l] == cc.CODER_RANS and escapes[l] > 0 for l in range(len(amax)))
        assert kinds[:4] == [cc.CODER_RANGE, cc.CODER_RANGE, cc.CODER_RANS, cc.CODER_RANGE]
    v1 = cc.encode_colors(p, c, step)
    assert v1 == want_v1, (name, step, len(v1), len(want_v1))
    v2 = cc.encode_colors(p, c, step, coder="rans")
    assert v2 == want_v2, (name, step, len(v2), len(want_v2))
    shuffle = np.random.default_rng(1).permutation(len(p))
    for data in (v1, v2):
        assert np.array_equal(cc.decode_colors(p, data), want)
        assert np.array_equal(cc.decode_colors(p[shuffle], data), want[shuffle])


def test_input_checks():
    p, c = CASES["dense_res12"]
    with pytest.raises(ValueError, match="duplicate"):
        cc.encode_colors(np.concatenate([p, p[:1]]), np.concatenate([c, c[:1]]), 4)
    with pytest.raises(ValueError, match="uint8"):
        cc.encode_colors(p, c.astype(np.int32), 4)
    with pytest.raises(ValueError, match="within"):
        cc.encode_colors(p - 1, c, 4)
    with pytest.raises(ValueError, match="within"):
        cc.encode_colors(p + 4090, c, 4)
    with pytest.raises(ValueError, match="integer"):
        cc.encode_colors(p.astype(np.float32), c, 4)
    with pytest.raises(ValueError, match="positive"):
        cc.encode_colors(p, c, 0)
    data = cc.encode_colors(p, c, 4)
    other, _ = CASES["dense_res20"]
    with pytest.raises(ValueError, match="other geometry"):
        cc.decode_colors(other, data)
    with pytest.raises(ValueError, match="truncated"):
        cc.decode_colors(p, data[:len(data) // 2])


def _coloured_cloud():
    """test_gpu_color.py's: a smooth colour field plus noise of sigma 10 on three shells at res 128"""
    pts = synthetic.make_cloud(seed=5, res=128, n_shells=3, rmin=0.2, rmax=0.4).astype(np.int32)
    t = pts.astype(np.float64) / 128
    col = np.stack([128 + 100 * np.sin(7 * t[:, 0] + 3 * t[:, 1]), 128 + 100 * np.cos(5 * t[:, 1] - 2 * t[:, 2]), 255 * t[:, 2]], -1)
    col = np.clip(np.rint(col + np.random.default_rng(5).normal(0, 10, col.shape)), 0, 255).astype(np.uint8)
    return pts, col


def test_rate_against_the_references_empirical_entropy():
    """bits <= (1 + m) H + 8 header bytes, H = sum over subbands of n H0(q) of the NUMPY reference's quantised coefficients, at
    every step at which H is below the raw 24 bits per point.  m = RATE_MARGIN comes from profiles/colorcodec_rd.txt."""
    p, c = _coloured_cloud()
    qualified = 0
    for step in STEPS:
        _, q, sub, _ = ref.codec(p, c, step)
        h = ref.empirical_bits(q, sub)
        data = cc.encode_colors(p, c, step)
        bits, head = 8 * len(data), cc.header_bytes(data)
        print("step", step, "bits", bits, "H", h, "bits / H", bits / h, "header bytes", head, "bpp", bits / len(p))
        if h < 24 * len(p):
            qualified += 1
            assert bits <= (1 + RATE_MARGIN) * h + 8 * head, (step, bits, h, bits / h)
    assert qualified >= 4


def test_cli_colors_raht(tmp_path, monkeypatch):
    from pcgcv1_amd import test as cli
    pts, col = _coloured_cloud()
    ply = tmp_path / "col_vox7.ply"
    iop.write_ply_colors(str(ply), pts, col)
    monkeypatch.chdir(tmp_path)
    five = ("strings", "strings_head", "strings_hyper", "pointnums", "cubepos")
    cli.main(["compress", str(ply), "--ckpt_dir=synthetic:7:sparse", "--min_num=20"])
    plain = {k: (tmp_path / "compressed" / ("col_vox7." + k)).read_bytes() for k in five}
    assert not (tmp_path / "compressed" / "col_vox7.colors").exists()
    cli.main(["decompress", "compressed/col_vox7", "plain_rec.ply", "--ckpt_dir=synthetic:7:sparse"])
    cli.main(["compress", str(ply), "--ckpt_dir=synthetic:7:sparse", "--min_num=20", "--colors", "raht", "--color_qstep", "8"])
    assert {k: (tmp_path / "compressed" / ("col_vox7." + k)).read_bytes() for k in five} == plain
    data = (tmp_path / "compressed" / "col_vox7.colors").read_bytes()
    cli.main(["decompress", "compressed/col_vox7", "colour_rec.ply", "--ckpt_dir=synthetic:7:sparse"])
    plain_p = iop.load_ply_data(str(tmp_path / "plain_rec.ply"))
    rec_p, rec_c = iop.load_ply_colors(str(tmp_path / "colour_rec.ply"))
    assert rec_c is not None and np.array_equal(rec_p, plain_p) and len(rec_p) > 1000
    assert np.array_equal(rec_c, cc.decode_colors(rec_p.astype(np.int32), data))
    assert np.array_equal(rec_c, ref.codec(rec_p, rc.recolor(pts, col, rec_p), 8)[0])
    # the refusals: the colours were coded for the rho = 1, scale = 1 geometry on one GPU
    for extra, word in ((["--rho=1.2"], "rho"), (["--scale=0.5"], "scale"), (["--colors_from", str(ply)], "colors_from"), (["--gpu=2"], "gpu")):
        with pytest.raises(SystemExit, match=word) as e:
            cli.main(["decompress", "compressed/col_vox7", "x_rec.ply", "--ckpt_dir=synthetic:7:sparse"] + extra)
        assert "rho = 1" in str(e.value)
    with pytest.raises(SystemExit, match="scale"):
        cli.main(["compress", str(ply), "--ckpt_dir=synthetic:7:sparse", "--colors", "raht", "--scale=0.5"])
    with pytest.raises(SystemExit, match="one GPU"):
        cli.main(["compress", str(ply), "--ckpt_dir=synthetic:7:sparse", "--colors", "raht", "--gpu=2"])
    nocolour = tmp_path / "nocolour.ply"
    iop.write_ply_data(str(nocolour), pts)
    with pytest.raises(SystemExit, match="nocolour.ply"):
        cli.main(["compress", str(nocolour), "--ckpt_dir=synthetic:7:sparse", "--min_num=20", "--colors", "raht"])
    # composes with --pointnums d1 (the counts are chosen first) and with the factorized mode
    cli.main(["compress", str(ply), "d1", "--ckpt_dir=synthetic:7:sparse", "--min_num=20", "--pointnums", "d1", "--colors", "raht"])
    cli.main(["decompress", "compressed/d1", "d1_rec.ply", "--ckpt_dir=synthetic:7:sparse"])
    d1_p, d1_c = iop.load_ply_colors(str(tmp_path / "d1_rec.ply"))
    assert np.array_equal(d1_c, ref.codec(d1_p, rc.recolor(pts, col, d1_p), 4)[0])
    cli.main(["compress", str(ply), "fz", "--ckpt_dir=synthetic:7:sparse", "--min_num=20", "--mode=factorized", "--colors", "raht"])
    cli.main(["decompress", "compressed/fz", "fz_rec.ply", "--ckpt_dir=synthetic:7:sparse", "--mode=factorized"])
    fz_p, fz_c = iop.load_ply_colors(str(tmp_path / "fz_rec.ply"))
    assert np.array_equal(fz_c, ref.codec(fz_p, rc.recolor(pts, col, fz_p), 4)[0])
    # a .colors taken from another cloud
    (tmp_path / "compressed" / "col_vox7.colors").write_bytes((tmp_path / "compressed" / "d1.colors").read_bytes())
    if len(d1_p) != len(rec_p) or not np.array_equal(d1_p, rec_p):
        with pytest.raises(ValueError, match="other geometry"):
            cli.main(["decompress", "compressed/col_vox7", "y_rec.ply", "--ckpt_dir=synthetic:7:sparse"])
    (tmp_path / "compressed" / "col_vox7.colors").write_bytes(cc.encode_colors(*CASES["dense_res20"], 4))
    with pytest.raises(ValueError, match="other geometry"):
        cli.main(["decompress", "compressed/col_vox7", "y_rec.ply", "--ckpt_dir=synthetic:7:sparse"])


def test_eval_color_qstep(tmp_path):
    from pcgcv1_amd import eval as pe
    pts, col = _coloured_cloud()
    ply = tmp_path / "col_vox7.ply"
    iop.write_ply_colors(str(ply), pts, col)
    body = "[DEFAULT]\ncube_size = 64\nmin_num = 20\n\n[R1]\nscale = 1.0\nckpt_dir = synthetic:7:sparse\nrho_d1 = 1.1\nrho_d2 = 1.0\n"
    ini = tmp_path / "cfg.ini"
    ini.write_text(body)
    rows_old = pe.eval(str(ply), str(tmp_path / "old"), str(ini), 128, color=True)
    rows = pe.eval(str(ply), str(tmp_path / "new"), str(ini), 128, color=True, color_qstep=8)
    new = ["bpp_colors", "coded c[0],PSNRF", "coded c[1],PSNRF", "coded c[2],PSNRF"]
    with open(tmp_path / "old" / "col_vox7.csv") as f:
        head_old = next(csv.reader(f))
    with open(tmp_path / "new" / "col_vox7.csv") as f:
        head = next(csv.reader(f))
    assert head == head_old + new
    same = [k for k in head_old if k != "optimal D2 PSNR"]
    assert {k: rows[0][k] for k in same} == {k: rows_old[0][k] for k in same}
    assert rows[0]["bpp_colors"] > 0 and all(np.isfinite(rows[0][k]) for k in new)
    # coded colours are the recoloured ones plus quantisation noise: never better than the uncoded figure by more than rounding
    assert rows[0]["coded c[0],PSNRF"] <= rows[0]["c[0],PSNRF"] + 0.5
    from pcgcv1_amd.models import model_voxception as model
    cubes_d, cube_positions, points_numbers, n, _ = pe.rate_point(pts, model, "synthetic:7:sparse", 1.0, 64, 20)
    rec = pe.postprocess_points(cubes_d, points_numbers, cube_positions, 1.0, 64, 1.0, None)
    rec = np.unique(np.rint(rec).astype(np.int32), axis=0)
    data = cc.encode_colors(rec, rc.recolor(pts, col, rec), 8)
    want = metrics.color_metrics(pts, col, rec, cc.decode_colors(rec, data))
    assert rows[0]["bpp_colors"] == round(8 * len(data) / len(pts), 4)
    for k in new[1:]:
        assert rows[0][k] == want[k.replace("coded ", "")]
