"""Colours on the host: coloured ply I/O (dataprocess/inout_points.py, libpcgc_host.so), the numpy statement of pc_error's
colour distortion against the values the pc_error binary printed (tests/golden/pc_error_color.npz), the new library symbols."""
import os
import re
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _color_ref as ref                                                 # noqa: E402
from pcgcv1_amd import _lib                                              # noqa: E402
from pcgcv1_amd.dataprocess import inout_points as iop                   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_HIP = ["pcgc_recolor_workspace_bytes", "pcgc_recolor", "pcgc_color_mse_workspace_bytes", "pcgc_color_mse"]
NEW_HOST = ["pcgc_parse_ply_columns", "pcgc_format_points_colors_int"]


def _cloud(seed, n=300, res=64):
    rng = np.random.default_rng(seed)
    pts = np.unique(rng.integers(0, res, (n, 3)), axis=0).astype(np.int32)
    pts = pts[rng.permutation(len(pts))]
    return pts, rng.integers(0, 256, (len(pts), 3)).astype(np.uint8), rng.standard_normal((len(pts), 3)).astype(np.float32)


# property name -> (ply type, struct code, value of row i)
def _columns(pts, col, nrm, color_names=("red", "green", "blue"), color_type="uchar"):
    code = {"uchar": "B", "float": "f"}[color_type]
    c = {"x": ("float", "f", pts[:, 0]), "y": ("float", "f", pts[:, 1]), "z": ("float", "f", pts[:, 2]),
         "nx": ("float", "f", nrm[:, 0]), "ny": ("float", "f", nrm[:, 1]), "nz": ("float", "f", nrm[:, 2]),
         "alpha": ("uchar", "B", np.full(len(pts), 255))}
    for k, name in enumerate(color_names):
        c[name] = (color_type, code, col[:, k])
    return c


def _write(path, order, columns, n, fmt="ascii", faces=False):
    head = "ply\nformat %s 1.0\ncomment made by a test\nelement vertex %d\n" % (fmt, n)
    head += "".join("property %s %s\n" % (columns[k][0], k) for k in order)
    if faces:
        head += "element face 1\nproperty list uchar int vertex_indices\n"
    head += "end_header\n"
    with open(path, "wb") as f:
        f.write(head.encode())
        for i in range(n):
            if fmt == "ascii":
                f.write((" ".join(("%d" % columns[k][2][i]) if columns[k][1] == "B" or k in "xyz" else ("%.6f" % columns[k][2][i])
                                  for k in order) + "\n").encode())
            else:
                e = "<" if fmt == "binary_little_endian" else ">"
                f.write(b"".join(struct.pack(e + columns[k][1], columns[k][2][i]) for k in order))
        if faces:
            f.write(b"3 0 1 2\n" if fmt == "ascii" else struct.pack(("<" if fmt == "binary_little_endian" else ">") + "Biii", 3, 0, 1, 2))


ORDERS = [
    ["x", "y", "z", "red", "green", "blue"],
    ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue", "alpha"],
    ["red", "x", "blue", "y", "alpha", "green", "z"],
    ["x", "y", "z", "blue", "green", "red", "nx", "ny", "nz"],
]


@pytest.mark.parametrize("fmt", ["ascii", "binary_little_endian", "binary_big_endian"])
@pytest.mark.parametrize("order", range(len(ORDERS)))
def test_load_ply_colors_finds_the_columns(tmp_path, fmt, order):
    pts, col, nrm = _cloud(10 + order)
    path = str(tmp_path / "c.ply")
    _write(path, ORDERS[order], _columns(pts, col, nrm), len(pts), fmt, faces=order == 1)
    got_p, got_c = iop.load_ply_colors(path)
    assert got_p.dtype == np.int32 and got_c.dtype == np.uint8
    assert np.array_equal(got_p, pts) and np.array_equal(got_c, col)


@pytest.mark.parametrize("names", [("r", "g", "b"), ("diffuse_red", "diffuse_green", "diffuse_blue")])
@pytest.mark.parametrize("fmt", ["ascii", "binary_little_endian"])
def test_load_ply_colors_other_names_and_float_colours(tmp_path, names, fmt):
    pts, col, nrm = _cloud(20)
    path = str(tmp_path / "c.ply")
    _write(path, ["x", "y", "z"] + list(names), _columns(pts, col, nrm, names, "float"), len(pts), fmt)
    got_p, got_c = iop.load_ply_colors(path)
    assert np.array_equal(got_p, pts) and np.array_equal(got_c, col) and got_c.dtype == np.uint8


@pytest.mark.parametrize("fmt", ["ascii", "binary_little_endian", "binary_big_endian"])
def test_load_ply_colors_without_colours_gives_none(tmp_path, fmt):
    pts, col, nrm = _cloud(30)
    path = str(tmp_path / "plain.ply")
    _write(path, ["x", "y", "z", "nx", "ny", "nz"], _columns(pts, col, nrm), len(pts), fmt)
    got_p, got_c = iop.load_ply_colors(path)
    assert np.array_equal(got_p, pts) and got_c is None
    iop.write_ply_data(path, pts)                              # the codec's own writer
    got_p, got_c = iop.load_ply_colors(path)
    assert np.array_equal(got_p, pts) and got_c is None


def test_existing_readers_are_unchanged_on_a_coloured_file(tmp_path):
    pts, col, nrm = _cloud(40)
    for fmt in ("ascii", "binary_little_endian"):
        path = str(tmp_path / ("c_%s.ply" % fmt))
        _write(path, ORDERS[1], _columns(pts, col, nrm), len(pts), fmt)
        assert np.array_equal(iop.load_ply_data(path), pts)
        p2, n2 = iop.load_ply_normals(path)
        assert np.array_equal(p2, pts) and np.allclose(n2, nrm, atol=1e-6)
    out = iop._load_binary_ply(str(tmp_path / "c_binary_little_endian.ply"))
    assert len(out) == 2                                       # (points, normals), as before


def test_write_ply_colors_round_trip_and_text(tmp_path):
    pts, col, _ = _cloud(50, n=40000, res=1024)                # large enough for the formatter's threads
    pts[0] = (0, 0, 0)
    col[0] = (0, 9, 10)
    col[1] = (99, 100, 255)
    path = str(tmp_path / "w.ply")
    iop.write_ply_colors(path, pts, col)
    got_p, got_c = iop.load_ply_colors(path)
    assert np.array_equal(got_p, pts) and np.array_equal(got_c, col)
    text = open(path).read()
    head = ("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
            "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n" % len(pts))
    assert text == head + "".join("%d %d %d %d %d %d\n" % (*p, *c) for p, c in zip(pts.tolist(), col.tolist()))
    # positions by write_ply_data's rule: dropping the colour columns gives its text
    iop.write_ply_data(str(tmp_path / "plain.ply"), pts)
    plain = open(str(tmp_path / "plain.ply")).read().split("end_header\n")[1]
    assert [" ".join(ln.split(" ")[:3]) for ln in text.split("end_header\n")[1].splitlines()] == plain.splitlines()
    assert np.array_equal(iop.load_ply_data(path), pts)
    with pytest.raises(ValueError):
        iop.write_ply_colors(path, pts, col[:-1])


def test_write_ply_colors_float_positions(tmp_path):
    pts, col, _ = _cloud(60, n=200)
    fpts = (pts.astype(np.float32) / np.float32(0.625)).astype(np.float32)
    path = str(tmp_path / "f.ply")
    iop.write_ply_colors(path, fpts, col)
    iop.write_ply_data(str(tmp_path / "plain.ply"), fpts)
    body = open(path).read().split("end_header\n")[1].splitlines()
    plain = open(str(tmp_path / "plain.ply")).read().split("end_header\n")[1].splitlines()
    assert [" ".join(ln.split(" ")[:3]) for ln in body] == plain
    got_p, got_c = iop.load_ply_colors(path, as_float=True)
    assert np.array_equal(got_c, col) and np.array_equal(got_p.astype(np.float32), fpts)
    assert np.array_equal(iop.load_ply_colors(path)[0], fpts.astype(np.int32))


def test_parse_ply_columns_reports_bad_rows(tmp_path):
    path = str(tmp_path / "bad.ply")
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\n"
                "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n1 2 3 4 5 6\n1 2 3 4 5\n7 8 9 1 2 3\n")
    with pytest.raises(_lib.PcgcError, match="line 2"):
        iop.load_ply_colors(path)
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\n"
                "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n1 2 3 300 5 6\n")
    with pytest.raises(ValueError, match="0..255"):
        iop.load_ply_colors(path)


def test_numpy_colour_rule_matches_the_pc_error_binary(golden):
    """tests/_color_ref.color_metrics against what `pc_error --color=1` printed (six significant digits for the mse, four
    decimals for the PSNR): mse within 1e-5 relative, PSNR within 1e-3."""
    g = golden("pc_error_color.npz")
    keys = [str(k) for k in g["keys"]]
    assert sorted(keys) == sorted(ref.COLOR_KEYS)
    assert int(g["n_cases"]) >= 5
    for i in range(int(g["n_cases"])):
        m = ref.color_metrics(g["a%d" % i], g["ca%d" % i], g["b%d" % i], g["cb%d" % i])
        for key, val in zip(keys, g["vals%d" % i]):
            val = float(val)
            print(i, key, m[key], val)
            if "PSNR" in key:
                assert m[key] == val or abs(m[key] - val) < 1e-3, (i, key, m[key], val)      # == : both inf on identical colours
            else:
                assert abs(m[key] - val) <= 1e-5 * abs(val), (i, key, m[key], val)


def test_numpy_recolour_rule_on_hand_made_cases():
    # t0 is chosen by s0 and s1 (a tie of s1 between t0 and t1): mean (10 + 13) / 2 = 11.5 -> 12; t2 is chosen by nobody and
    # takes the rounded mean of its two nearest source points s1, s2
    s = np.array([[0, 0, 0], [2, 0, 0], [6, 0, 0]])
    c = np.array([[10, 0, 255], [13, 1, 255], [20, 2, 0]], np.uint8)
    t = np.array([[1, 0, 0], [3, 0, 0], [4, 1, 0], [7, 0, 0]])
    col, cnt = ref.recolor(s, c, t)
    assert cnt.tolist() == [2, 1, 0, 1]
    assert col.tolist() == [[12, 1, 255], [13, 1, 255], [17, 2, 128], [20, 2, 0]]


def test_libraries_export_the_colour_symbols():
    header = open(os.path.join(ROOT, "include", "pcgc.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(pcgc_[a-z0-9_]+)\s*\(", header))
    for name in NEW_HIP + NEW_HOST:
        assert name in declared, name
    hip, host = _lib.hip(), _lib.host()                        # raises if a declared symbol is missing
    for name in NEW_HIP:
        assert name in _lib.HIP_API and hasattr(hip, name)
    for name in NEW_HOST:
        assert name in _lib.HOST_API and hasattr(host, name)
    assert hip.pcgc_recolor_workspace_bytes(64, 10, 10) > 2 * (64 ** 3 // 8)
    assert hip.pcgc_recolor_workspace_bytes(5000, 10, 10) == 0


def test_cli_flags_exist_and_default_off():
    from pcgcv1_amd import test as cli
    assert cli.parse_args(["decompress", "x"]).colors_from == ""
    assert cli.parse_args(["decompress", "x", "--colors_from", "o.ply"]).colors_from == "o.ply"
    with pytest.raises(SystemExit, match="one GPU"):
        cli.main(["decompress", "x", "--gpu=2", "--colors_from", "o.ply"])
    with pytest.raises(SystemExit, match="decompress"):
        cli.main(["compress", "x.ply", "--colors_from", "o.ply"])
