"""The host side of the ingest step (pcgcv1_amd/ingest.py, inout_points.load_ply_scan, the --voxelize flags of test.py): the
frame file, frame fitting against the rule in numpy (tests/_ingest_ref.py), the float ply reader and the refusals.  No GPU."""
import os
import struct
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _ingest_ref as ref                                                # noqa: E402
from pcgcv1_amd import ingest                                            # noqa: E402
from pcgcv1_amd import test as cli                                       # noqa: E402
from pcgcv1_amd.dataprocess import inout_points as iop                   # noqa: E402


def _same_frame(frame, want):
    origin, step, bits = want
    assert frame.origin.tobytes() == np.asarray(origin, np.float64).tobytes() and frame.step == step and frame.bits == bits


# ---------------------------------------------------------------------------- <name>.frame
def test_frame_file_layout_and_round_trip(tmp_path):
    frame = ingest.Frame((-1.25, 0.1, 3e5), 0.002, 10)
    name = str(tmp_path / "a.frame")
    ingest.write_frame(name, frame)
    data = open(name, "rb").read()
    assert len(data) == 40 and data[:4] == b"PCFR" and data[4] == 1 and data[5] == 10 and data[6:8] == b"\0\0"
    assert struct.unpack("<3d", data[8:32]) == (-1.25, 0.1, 3e5) and struct.unpack("<d", data[32:]) == (0.002,)
    back = ingest.read_frame(name)
    assert back == frame and back.R == 1023
    assert ingest.frame_path("x/scan_vox10.ply") == "x/scan_vox10.frame"


@pytest.mark.parametrize("damage, cause", [
    (lambda d: b"PCFX" + d[4:], "magic"),
    (lambda d: d[:4] + b"\x02" + d[5:], "version"),
    (lambda d: d[:-1], "40 bytes"),
    (lambda d: d + b"\0", "40 bytes"),
    (lambda d: d[:5] + b"\x00" + d[6:], "bits"),
    (lambda d: d[:5] + b"\x0d" + d[6:], "bits"),
    (lambda d: d[:32] + struct.pack("<d", 0.0), "step"),
    (lambda d: d[:8] + struct.pack("<d", float("nan")) + d[16:], "finite"),
])
def test_frame_reader_names_what_is_wrong(tmp_path, damage, cause):
    name = str(tmp_path / "a.frame")
    with open(name, "wb") as f:
        f.write(damage(ingest.frame_bytes(ingest.Frame((0.0, 1.0, 2.0), 0.5, 7))))
    with pytest.raises(ValueError, match=cause):
        ingest.read_frame(name)


# ---------------------------------------------------------------------------- fit_frame
def test_fit_frame_bits_on_hand_made_inputs():
    p = np.array([[-3.0, 10.0, 0.5], [1.0, 10.5, 0.25], [0.0, 12.0, -0.0]])
    f = ingest.fit_frame(p, bits=3)
    assert f.origin.tolist() == [-3.0, 10.0, 0.0] and f.step == 4.0 / 7 and f.bits == 3
    assert np.signbit(p[:, 2].min()) and not np.signbit(f.origin[2])   # the -0.0 minimum came out as +0.0
    _same_frame(f, ref.fit_frame(p, bits=3))
    # one point, and several equal ones: the extent is 0 and the step 1
    for q in (p[:1], np.repeat(p[1:2], 4, 0)):
        f = ingest.fit_frame(q, bits=12)
        assert f.step == 1.0 and f.origin.tolist() == q[0].tolist()
        _same_frame(f, ref.fit_frame(q, bits=12))
    # non-finite rows do not count, wherever they stand
    bad = np.concatenate([[[np.nan, 0, 0]], p, [[0, np.inf, 0], [0, 0, -np.inf]]])
    _same_frame(ingest.fit_frame(bad, bits=3), ref.fit_frame(p, bits=3))
    for b in (0, 13):
        with pytest.raises(ValueError, match="bits"):
            ingest.fit_frame(p, bits=b)
    with pytest.raises(ValueError, match="finite"):
        ingest.fit_frame(bad[[0, -1]], bits=3)
    with pytest.raises(ValueError, match="one of them"):
        ingest.fit_frame(p)
    with pytest.raises(ValueError, match="one of them"):
        ingest.fit_frame(p, bits=3, voxel_size=1.0)


def test_fit_frame_voxel_size_on_hand_made_inputs():
    p = np.array([[-0.7, 0.0, 5.0], [0.3, 0.26, 5.24]])
    f = ingest.fit_frame(p, voxel_size=0.25)
    assert f.origin.tolist() == [-0.75, 0.0, 5.0] and f.step == 0.25       # floor(min / s) * s, also below zero
    assert f.bits == 3                                                     # (0.3 + 0.75) / 0.25 + 0.5 -> 4: three bits
    _same_frame(f, ref.fit_frame(p, voxel_size=0.25))
    # exactly 12 bits: the largest coordinate is 4095 (accepted); 4096 needs 13 (refused, naming extent and voxel size)
    ok = np.array([[0.0, 0.0, 0.0], [4095.0, 1.0, 2.0]])
    f = ingest.fit_frame(ok, voxel_size=1.0)
    assert f.bits == 12 and f.R == 4095
    _same_frame(f, ref.fit_frame(ok, voxel_size=1.0))
    assert ingest.fit_frame(ok * 0.5, voxel_size=0.5).bits == 12
    too_big = np.array([[0.0, 0.0, 0.0], [4096.0, 1.0, 2.0]])
    with pytest.raises(ValueError, match=r"4096\.0 at voxel size 1\.0 needs more than 12 bits"):
        ingest.fit_frame(too_big, voxel_size=1.0)
    with pytest.raises(ValueError):
        ref.fit_frame(too_big, voxel_size=1.0)
    with pytest.raises(ValueError, match="12 bits"):
        ingest.fit_frame(np.array([[0.0, 0.0, 0.0], [1e300, 0.0, 0.0]]), voxel_size=1e-300)
    for s in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="voxel_size"):
            ingest.fit_frame(p, voxel_size=s)
    # a single point still gets a grid
    assert ingest.fit_frame(p[:1], voxel_size=0.25).bits == 1


@pytest.mark.parametrize("kind", ["bits", "voxel_size"])
def test_apply_frame_of_quantised_points_lies_within_half_a_step(kind):
    rng = np.random.default_rng(5)
    p = rng.normal(size=(2000, 3)) * (3.0, 0.01, 40.0) + (-7.0, 2.0, 1e3)
    frame = ingest.fit_frame(p, bits=9) if kind == "bits" else ingest.fit_frame(p, voxel_size=0.37)
    q, keys = ref.quantize(p, frame.origin, frame.step, frame.bits)
    assert q.min() >= 0 and q.max() <= frame.R and (keys >= 0).all()
    back = ingest.apply_frame(q, frame)
    assert back.dtype == np.float64
    np.testing.assert_array_equal(back, ref.apply_frame(q, frame.origin, frame.step))
    # half a step, plus the rounding of the three operations on coordinates of this size
    assert np.abs(back - p).max() <= frame.step / 2 + 8 * np.spacing(np.abs(p).max())
    if kind == "bits":
        assert q.max() == frame.R                                          # the far corner lands on R, not R + 1


# ---------------------------------------------------------------------------- load_ply_scan
def _scan(n=37, seed=3):
    rng = np.random.default_rng(seed)
    pts = np.round(rng.normal(size=(n, 3)) * 2.5, 4)                       # fractional and negative
    pts = pts.astype(np.float32).astype(np.float64)                        # what a `float` property holds
    colors = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    normals = rng.normal(size=(n, 3)).astype(np.float32)
    return pts, colors, normals


def _write_binary(name, order, pts, colors, normals, double_xyz=False):
    t = "double" if double_xyz else "float"
    fields = [("x", order + ("f8" if double_xyz else "f4")), ("y", order + ("f8" if double_xyz else "f4")),
              ("z", order + ("f8" if double_xyz else "f4"))]
    head = "ply\nformat binary_%s_endian 1.0\nelement vertex %d\nproperty %s x\nproperty %s y\nproperty %s z\n" % (
        "little" if order == "<" else "big", len(pts), t, t, t)
    if normals is not None:
        fields += [(k, order + "f4") for k in ("nx", "ny", "nz")]
        head += "property float nx\nproperty float ny\nproperty float nz\n"
    if colors is not None:
        fields += [(k, "u1") for k in ("red", "green", "blue")]
        head += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    v = np.zeros(len(pts), np.dtype(fields))
    for k, name_ in enumerate("xyz"):
        v[name_] = pts[:, k]
    if normals is not None:
        for k, name_ in enumerate(("nx", "ny", "nz")):
            v[name_] = normals[:, k]
    if colors is not None:
        for k, name_ in enumerate(("red", "green", "blue")):
            v[name_] = colors[:, k]
    with open(name, "wb") as f:
        f.write((head + "end_header\n").encode() + v.tobytes())


def _write_ascii(name, pts, colors, normals):
    head = "ply\nformat ascii 1.0\ncomment a scan\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n" % len(pts)
    cols = [pts]
    if normals is not None:
        head += "property float nx\nproperty float ny\nproperty float nz\n"
        cols.append(normals.astype(np.float64))
    if colors is not None:
        head += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    with open(name, "w") as f:
        f.write(head + "end_header\n")
        for i in range(len(pts)):
            row = [repr(float(x)) for c in cols for x in c[i]] + ([str(int(x)) for x in colors[i]] if colors is not None else [])
            f.write(" ".join(row) + "\n")


@pytest.mark.parametrize("form", ["ascii", "<", ">"])
@pytest.mark.parametrize("with_colors, with_normals", [(True, True), (True, False), (False, True), (False, False)])
def test_load_ply_scan_reads_floats_colours_and_normals(tmp_path, form, with_colors, with_normals):
    pts, colors, normals = _scan()
    colors, normals = colors if with_colors else None, normals if with_normals else None
    name = str(tmp_path / "scan.ply")
    if form == "ascii":
        _write_ascii(name, pts, colors, normals)
    else:
        _write_binary(name, form, pts, colors, normals)
    got_p, got_c, got_n = iop.load_ply_scan(name)
    assert (pts < 0).any() and (pts != np.rint(pts)).any()
    assert got_p.dtype == np.float64 and got_p.flags["C_CONTIGUOUS"]
    np.testing.assert_array_equal(got_p, pts)
    for got, want, dtype in ((got_c, colors, np.uint8), (got_n, normals, np.float32)):
        if want is None:
            assert got is None
        else:
            assert got.dtype == dtype
            np.testing.assert_array_equal(got, want)
    # the loaders that were there keep truncating
    np.testing.assert_array_equal(iop.load_ply_data(name), pts.astype(np.int32))


def test_load_ply_scan_keeps_double_coordinates(tmp_path):
    pts = np.array([[1e6 + 0.001, -0.1, 1 / 3], [2.0, 3.0, 4.0]])
    name = str(tmp_path / "d.ply")
    _write_binary(name, "<", pts, None, None, double_xyz=True)
    np.testing.assert_array_equal(iop.load_ply_scan(name)[0], pts)
    assert (pts.astype(np.float32) != pts).any()


def test_load_ply_scan_agrees_with_load_ply_colors_as_float(tmp_path):
    pts, colors, normals = _scan(50, 8)
    name = str(tmp_path / "scan.ply")
    _write_ascii(name, pts, colors, normals)
    want_p, want_c = iop.load_ply_colors(name, as_float=True)
    got_p, got_c, _ = iop.load_ply_scan(name)
    np.testing.assert_array_equal(got_p, want_p)
    np.testing.assert_array_equal(got_c, want_c)


def test_load_ply_scan_refuses_a_file_without_header(tmp_path):
    name = str(tmp_path / "bare.ply")
    with open(name, "w") as f:
        f.write("0.5 1.5 2.5\n")
    with pytest.raises(ValueError, match="header"):
        iop.load_ply_scan(name)


# ---------------------------------------------------------------------------- command lines
@pytest.mark.parametrize("argv, words", [
    (["compress", "scan.ply", "--voxelize", "7", "--voxel_size", "0.1"], "give one of them"),
    (["compress", "scan.ply", "--voxelize", "7", "--scale", "0.5"], "--scale must be 1"),
    (["compress", "scan.ply", "--voxel_size", "0.1", "--scale", "0.5"], "--scale must be 1"),
    (["decompress", "compressed/scan", "--voxelize", "7"], "belong to compress"),
    (["decompress", "compressed/scan", "--voxel_size", "0.1"], "belong to compress"),
    (["compress", "scan.ply", "--voxelize", "7", "--gpu", "2"], r"multi-GPU runs .*one GPU"),
    (["compress", "scan.ply", "--voxel_size", "0.1", "--gpu", "8"], r"multi-GPU runs .*one GPU"),
    (["compress", "scan.ply", "--voxelize", "13"], r"1\.\.12"),
    (["compress", "scan.ply", "--voxel_size", "-1"], "positive"),
])
def test_codec_cli_refusals_by_name_before_any_gpu_work(argv, words, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert isinstance(e.value.code, str) and __import__("re").search(words, e.value.code), e.value.code


def test_codec_cli_prints_its_arguments_as_before_without_the_new_flags(capsys):
    with pytest.raises(SystemExit):
        cli.main(["compress", "scan.ply", "--gpu", "0"])
    line = capsys.readouterr().out.splitlines()[0]
    assert line.startswith("Namespace(command='compress'") and "voxel" not in line
    with pytest.raises(SystemExit):
        cli.main(["compress", "scan.ply", "--gpu", "0", "--voxelize", "9"])
    assert "voxelize=9" in capsys.readouterr().out.splitlines()[0]


@pytest.mark.parametrize("argv", [
    ["--input", "a.ply", "--output", "b.ply"],
    ["--input", "a.ply", "--output", "b.ply", "--bits", "10", "--voxel_size", "0.1"],
    ["--input", "a.ply", "--output", "b.ply", "--bits", "13"],
    ["--input", "a.ply", "--output", "b.ply", "--voxel_size", "0"],
    ["--input", "a.ply", "--bits", "10"],
])
def test_ingest_cli_refuses_bad_arguments(argv):
    with pytest.raises(SystemExit) as e:
        ingest.parse_args(argv)
    assert e.value.code == 2


def test_frame_travels_with_the_compressed_files_and_a_stale_one_is_taken_away(tmp_path, capsys):
    from pcgcv1_amd.dataprocess import inout_bitstream as bs
    fb = ingest.frame_bytes(ingest.Frame((0.5, -1.0, 2.0), 0.125, 7))
    cloud = ("x", b"abc", np.array([70], np.uint16), np.array([[0, 1, 2]]), -2, 3, np.array([1, 2, 2, 2, 8], np.int16))
    sizes = bs.write_binary_files_factorized(*cloud, rootdir=str(tmp_path), frame=fb)
    assert (tmp_path / "x.frame").read_bytes() == fb and ingest.read_frame(str(tmp_path / "x.frame")).bits == 7
    assert "Total file size (Bytes): %d\n" % (sum(sizes) + 40) in capsys.readouterr().out
    assert bs.write_binary_files_factorized(*cloud, rootdir=str(tmp_path)) == sizes
    said = capsys.readouterr().out
    assert not (tmp_path / "x.frame").exists() and "x.frame" in said and "Total file size (Bytes): %d\n" % sum(sizes) in said
    bs.write_binary_files_factorized(*cloud, rootdir=str(tmp_path))
    assert "frame" not in capsys.readouterr().out                         # nothing new is printed where there never was a frame
