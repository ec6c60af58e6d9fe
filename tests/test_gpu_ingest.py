"""The ingest kernels (csrc/ingest.hip: pcgc_ingest_bounds, _quantize, _merge, each called alone through pcgcv1_amd/ingest.py)
against the rule in numpy (tests/_ingest_ref.py): points, counts, colours, row count and dropped count bit for bit, normals
within one float32 ulp (the sums are exact integers on both sides; only the last float64 -> float32 rounding of the same
quotient may differ) and zero normals exactly.  Then a raw scan end to end through the ingest CLI and the codec's CLI."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _ingest_ref as ref                                                # noqa: E402
from _clouds import faces                                                # noqa: E402
from pcgcv1_amd import _lib, ingest, metrics                             # noqa: E402
from pcgcv1_amd.dataprocess import inout_points as iop                   # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _lib.require_gpu()


def _attributes(rng, n):
    colors = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    normals = rng.normal(size=(n, 3))
    normals = (normals / np.linalg.norm(normals, axis=1, keepdims=True)).astype(np.float32)
    return colors, normals


def _assert_normals(got, want):
    assert got.dtype == np.float32 and got.shape == want.shape
    zero = (want == 0).all(1)
    np.testing.assert_array_equal(got[zero], want[zero])
    diff = np.abs(got.astype(np.float64) - want.astype(np.float64))
    assert (diff <= np.spacing(np.abs(want))).all(), float((diff / np.spacing(np.abs(want))).max())


def _check(points, colors, normals, frame):
    """every stage alone against the rule; -> what the merge returned"""
    want_lo, want_hi, want_dropped = ref.bounds(points)
    lo, hi, dropped = ingest.bounds(points)
    np.testing.assert_array_equal(lo, want_lo)
    np.testing.assert_array_equal(hi, want_hi)
    assert dropped == want_dropped
    want_q, want_keys = ref.quantize(points, frame.origin, frame.step, frame.bits)
    q, keys = ingest.quantize(points, frame)
    np.testing.assert_array_equal(q.cpu().numpy(), want_q)
    np.testing.assert_array_equal(keys.cpu().numpy(), want_keys)
    want = ref.merge(want_keys, frame.bits, colors, normals)
    got = ingest.merge(keys, frame.bits, colors, normals)
    np.testing.assert_array_equal(got[0], want[0])
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32
    np.testing.assert_array_equal(got[1], want[1])
    assert int(got[1].sum()) == len(points) - dropped
    np.testing.assert_array_equal(got[0], np.unique(want_q[want_keys >= 0], axis=0))       # np.unique's order
    if colors is None:
        assert got[2] is None
    else:
        assert got[2].dtype == np.uint8
        np.testing.assert_array_equal(got[2], want[2])
    if normals is None:
        assert got[3] is None
    else:
        _assert_normals(got[3], want[3])
    return got


@pytest.mark.parametrize("bits", [1, 7])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_wave_and_block_edges(n, bits):
    rng = np.random.default_rng(100 * bits + n)
    points = rng.normal(size=(n, 3)) * (0.5, 2.0, 0.01) + (3.0, -40.0, 0.0)
    colors, normals = _attributes(rng, n)
    frame = ingest.fit_frame(points, bits=bits)
    pts = _check(points, colors, normals, frame)[0]
    assert pts.max() == (frame.R if n > 1 else 0) and pts.min() == 0          # the far corner lands on R, not on R + 1
    # the whole call, and a frame fitted on the device
    out = ingest.voxelize_scan(points, colors, normals, bits=bits)
    want = ref.voxelize_scan(points, colors, normals, bits=bits)
    assert out[4] == frame == ingest.fit_frame(torch.from_numpy(points).cuda(), bits=bits) and out[5] == want[5] == 0
    np.testing.assert_array_equal(out[0], want[0])
    np.testing.assert_array_equal(out[1], want[1])
    np.testing.assert_array_equal(out[3], want[3])
    _assert_normals(out[2], want[2])


def test_heavy_contention_in_one_corner():
    rng = np.random.default_rng(7)
    points = rng.uniform(-0.5, 1.49, (4000, 3))
    colors, normals = _attributes(rng, 4000)
    normals = np.abs(normals)                                  # one octant: no voxel's sum cancels
    pts, counts, _, _ = _check(points, colors, normals, ingest.Frame((0.0, 0.0, 0.0), 1.0, 5))
    assert len(pts) == 8 and pts.max() == 1 and counts.min() > 300 and counts.sum() == 4000


def test_half_boundaries_round_up_and_the_far_corner_lands_on_R():
    # step a power of two, origin a multiple of it: every operation is exact
    frame = ingest.Frame((-2.0, 0.0, 4.0), 0.25, 4)
    k = np.arange(-1, 16)
    g = np.stack(np.meshgrid(k, k[::5], k[::7], indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    on_half = frame.origin + (g + 0.5) * 0.25
    q = _check(on_half, None, None, frame)[0]
    want_q, _ = ref.quantize(on_half, frame.origin, frame.step, frame.bits)
    np.testing.assert_array_equal(want_q, np.clip(g + 1, 0, 15).astype(np.int32))       # .5 goes up; -0.5 -> 0; 15.5 -> clamped to R
    assert q.max() == 15
    below_half = frame.origin + (g + 0.5) * 0.25 - 2.0 ** -40
    np.testing.assert_array_equal(ref.quantize(below_half, frame.origin, frame.step, frame.bits)[0], np.clip(g, 0, 15).astype(np.int32))
    _check(below_half, None, None, frame)
    # a fitted frame: the maximum of the longest axis is R exactly
    corner = np.array([[0.1, 0.2, 0.3], [12.9, 7.7, 3.3], [5.0, 6.0, 1.0]])
    fitted = ingest.fit_frame(corner, bits=7)
    assert _check(corner, None, None, fitted)[0].max(0).tolist() == [127, 74, 30]


def test_a_frame_applied_to_points_outside_it_clamps():
    frame = ingest.Frame((10.0, -5.0, 0.0), 0.5, 3)
    points = np.array([[9.0, -5.0, 0.0], [10.0, -100.0, 0.3], [1e6, -4.0, 1e300], [-1.7e308, 1.7e308, 2.0], [12.0, -3.0, 3.4],
                       [13.76, -1.24, 3.76], [1e-310, -1e-310, 5e-324]])
    colors, normals = _attributes(np.random.default_rng(2), len(points))
    q, keys = ingest.quantize(points, frame)
    assert q.cpu().numpy().tolist() == [[0, 0, 0], [0, 0, 1], [7, 2, 7], [0, 7, 4], [4, 4, 7], [7, 7, 7], [0, 7, 0]]
    pts = _check(points, colors, normals, frame)[0]
    assert pts.min() == 0 and pts.max() == 7


def test_non_finite_rows_are_dropped_and_counted():
    rng = np.random.default_rng(9)
    points = rng.uniform(0, 10, (300, 3))
    points[0, 1] = np.nan                                       # the first row, the last, a block edge and an all-bad row
    points[-1, 2] = np.inf
    points[255, 0] = -np.inf
    points[256] = (np.nan, np.inf, -np.inf)
    points[17, 0] = np.inf
    colors, normals = _attributes(rng, 300)
    frame = ingest.fit_frame(points, bits=6)
    _check(points, colors, normals, frame)
    out = ingest.voxelize_scan(points, colors, normals, bits=6)
    assert out[5] == 5 and out[3].sum() == 295 and out[4] == frame
    with pytest.raises(ValueError, match="finite"):
        ingest.voxelize_scan(points[[0, 256, 299]], bits=6)


def test_colour_means_round_half_up():
    frame = ingest.Frame((0.0, 0.0, 0.0), 1.0, 2)
    points = np.array([[0, 0, 0], [0, 0, 0], [3, 3, 3], [3, 3, 3], [3, 3, 3], [1, 2, 3]], np.float64)
    colors = np.array([[0, 1, 255], [1, 0, 254], [254, 255, 255], [255, 254, 255], [255, 255, 254], [7, 0, 255]], np.uint8)
    got = _check(points, colors, None, frame)
    assert got[2].tolist() == [[1, 1, 255], [7, 0, 255], [255, 255, 255]] and got[1].tolist() == [2, 1, 3]


def test_normals_cancel_to_zero_and_non_finite_components_count_as_zero():
    frame = ingest.Frame((0.0, 0.0, 0.0), 1.0, 3)
    points = np.array([[1, 1, 1], [1, 1, 1], [2, 2, 2], [2, 2, 2], [5, 0, 7], [5, 0, 7], [6, 6, 6]], np.float64)
    normals = np.array([[0.6, -0.8, 0.0], [-0.6, 0.8, 0.0],                         # opposite: the zero normal
                        [np.nan, 0.0, 1.0], [0.0, np.inf, 1.0],                       # bad components are 0: (0, 0, 1)
                        [3.0, 0.0, 0.0], [0.0, -1.0, 0.0],                            # clamped to 1: (1, -1, 0) / sqrt 2
                        [np.nan, -np.inf, np.nan]], np.float32)                       # nothing left: zero
    got = _check(points, None, normals, frame)[3]
    assert got[0].tolist() == [0, 0, 0] and got[1].tolist() == [0, 0, 1] and got[3].tolist() == [0, 0, 0]
    assert got[2, 2] == 0 and got[2, 0] == -got[2, 1] == np.float32(np.sqrt(0.5))


def test_keys_outside_the_grid_contribute_nothing():
    bits, n = 2, 70
    rng = np.random.default_rng(4)
    keys = rng.integers(0, 64, n).astype(np.int64)
    keys[[0, 13, 64, 69]] = (-1, 64, 2 ** 40, -2 ** 62)
    colors, normals = _attributes(rng, n)
    want = ref.merge(keys, bits, colors, normals)
    got = ingest.merge(torch.from_numpy(keys).cuda(), bits, colors, normals)
    for g, w in zip(got[:3], want[:3]):
        np.testing.assert_array_equal(g, w)
    _assert_normals(got[3], want[3])
    assert got[1].sum() == n - 4
    # nothing in the grid at all: no rows
    none = ingest.merge(torch.full((5,), -1, dtype=torch.int64).cuda(), bits, colors[:5], None)
    assert none[0].shape == (0, 3) and none[1].shape == (0,) and none[2].shape == (0, 3)


def test_argument_checks():
    lib = _lib.hip()
    assert lib.pcgc_ingest_workspace_bytes(0, 10) == 0 and lib.pcgc_ingest_workspace_bytes(13, 10) == 0
    assert lib.pcgc_ingest_workspace_bytes(7, 0) == 0 and lib.pcgc_ingest_workspace_bytes(7, 2 ** 31) == 0
    assert lib.pcgc_ingest_workspace_bytes(7, 10) > 2 * (128 ** 3) // 8
    dev = _lib.require_gpu()
    keys = torch.zeros(8, dtype=torch.int64, device=dev)
    small = torch.zeros(64, dtype=torch.uint8, device=dev)
    ws = torch.zeros(int(lib.pcgc_ingest_workspace_bytes(1, 8)), dtype=torch.uint8, device=dev)
    s = _lib.stream()

    def merge(n, bits, colors, cap, ws_bytes):
        return lib.pcgc_ingest_merge(_lib.dptr(keys), n, bits, _lib.dptr(small) if colors else None, None, _lib.dptr(small), _lib.dptr(small),
                                     _lib.dptr(small) if colors else None, None, cap, _lib.dptr(keys), _lib.dptr(ws), ws_bytes, s)
    assert merge(8, 1, False, 7, ws.numel()) == -1 and b"capacity" in lib.pcgc_last_error()
    assert merge(8, 1, False, 8, ws.numel() - 1) == -1 and b"workspace" in lib.pcgc_last_error()
    assert merge(8, 0, False, 8, ws.numel()) == -1 and merge(8, 13, False, 8, ws.numel()) == -1
    assert merge(16843010, 1, True, 8, ws.numel()) == -1 and b"colour sums" in lib.pcgc_last_error()       # refused before any launch
    origin = np.zeros(3)
    for bad_origin, step in ((np.array([np.nan, 0, 0]), 1.0), (origin, 0.0), (origin, -1.0), (origin, float("inf")), (origin, float("nan"))):
        assert lib.pcgc_ingest_quantize(_lib.dptr(ws), 1, _lib.nptr(bad_origin), step, 1, _lib.dptr(small), _lib.dptr(keys), s) == -1
    with pytest.raises(ValueError, match="uint8"):
        ingest.voxelize_scan(np.zeros((2, 3)), colors=np.zeros((2, 3), np.float32), bits=3)
    with pytest.raises(ValueError, match="shape"):
        ingest.voxelize_scan(np.zeros((2, 3)), normals=np.zeros((3, 3), np.float32), bits=3)


# ---------------------------------------------------------------------------- end to end
FIVE = ("strings", "strings_head", "strings_hyper", "pointnums", "cubepos")
ORIGIN, STEP = np.array([-3.5, 10.0, 0.75]), 0.25
CKPT = "--ckpt_dir=synthetic:0"


@pytest.fixture(scope="module")
def scan(tmp_path_factory):
    """A surface-like cloud on the 128 grid as a scanner would have seen it: p = origin + step * (g + jitter), |jitter| < 0.4 in
    64ths, two to four points per voxel with random colours, as a binary little-endian ply.  The first point of a voxel has no
    jitter and the jitter points inwards on the outer faces, so --bits 7 fits exactly (origin, step) and every coordinate, the
    decoded ones included, is a float32."""
    g, _ = faces(11, 128, 6000)
    rng = np.random.default_rng(11)
    rep = rng.integers(2, 5, len(g))
    idx = np.repeat(np.arange(len(g)), rep)
    first = np.r_[True, idx[1:] != idx[:-1]]
    jitter = rng.integers(-25, 26, (len(idx), 3)) / 64.0
    jitter[first] = 0
    cells = g[idx]
    jitter = np.where(cells == 0, np.abs(jitter), np.where(cells == 127, -np.abs(jitter), jitter))
    points = ORIGIN + STEP * (cells + jitter)
    order = rng.permutation(len(points))
    points, cells = points[order], cells[order]
    colors = rng.integers(0, 256, (len(points), 3)).astype(np.uint8)
    assert np.abs(jitter).max() < 0.4 and np.array_equal(points.astype(np.float32).astype(np.float64), points)
    d = tmp_path_factory.mktemp("scan")
    v = np.zeros(len(points), np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")]))
    for k, name in enumerate(("x", "y", "z")):
        v[name] = points[:, k]
    for k, name in enumerate(("red", "green", "blue")):
        v[name] = colors[:, k]
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
            "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n" % len(points))
    with open(str(d / "scan.ply"), "wb") as f:
        f.write(head.encode() + v.tobytes())
    return d, points, colors, np.unique(g, axis=0)


def test_scan_through_the_ingest_cli_and_the_codec(scan, monkeypatch, capsys):
    from pcgcv1_amd import test as cli
    d, points, colors, grid = scan
    monkeypatch.chdir(d)
    # 1. ingest, then compress the voxelised ply; compress --voxelize: the same five files, and a frame only there
    ingest.main(["--input", "scan.ply", "--output", "scan_vox7.ply", "--bits", "7"])
    said = capsys.readouterr().out
    assert "%d input points, 0 dropped" % len(points) in said and "%d occupied voxels, at most 4 points" % len(grid) in said
    frame = ingest.read_frame("scan_vox7.frame")
    assert frame == ingest.Frame(ORIGIN, STEP, 7)
    vox_p, vox_c = iop.load_ply_colors("scan_vox7.ply")
    np.testing.assert_array_equal(vox_p, grid)
    want = ref.voxelize_scan(points, colors, bits=7)
    np.testing.assert_array_equal(vox_c, want[1])
    cli.main(["compress", "scan_vox7.ply", "a", CKPT])
    plain = {k: open("compressed/a." + k, "rb").read() for k in FIVE}
    assert not os.path.exists("compressed/a.frame")
    cli.main(["compress", "scan.ply", "b", CKPT, "--voxelize", "7"])
    said = capsys.readouterr().out
    assert {k: open("compressed/b." + k, "rb").read() for k in FIVE} == plain
    assert open("compressed/b.frame", "rb").read() == open("scan_vox7.frame", "rb").read()
    assert "Total file size (Bytes): %d" % (sum(len(v) for v in plain.values()) + 40) in said
    assert len(np.frombuffer(plain["pointnums"], np.uint16)) == 8                      # every 64^3 cube is above --min_num
    # 2. decompress both: the scan-frame output is apply_frame of the integer output, in the same order
    cli.main(["decompress", "compressed/a", "a_rec.ply", CKPT])
    cli.main(["decompress", "compressed/b", "b_rec.ply", CKPT])
    a_rec = iop.load_ply_data("a_rec.ply")
    b_rec, b_col, _ = iop.load_ply_scan("b_rec.ply")
    assert b_col is None and len(a_rec) > 1000
    np.testing.assert_array_equal(b_rec, ingest.apply_frame(a_rec, frame))
    # 3. measured in the scan's own units
    res = metrics.pc_error_float(points.astype(np.float32), b_rec.astype(np.float32))
    print("D1 in scan units:", res["mseF      (p2point)"])
    assert np.isfinite(res["mseF      (p2point)"]) and res["mseF      (p2point)"] >= 0
    assert (b_rec >= points.min(0) - STEP).all() and (b_rec <= points.max(0) + STEP).all()
    # a voxel size gives the same grid here; --render keeps working on the float file
    cli.main(["compress", "scan.ply", "c", CKPT, "--voxel_size", "0.25"])
    assert {k: open("compressed/c." + k, "rb").read() for k in FIVE} == plain
    assert ingest.read_frame("compressed/c.frame") == frame
    cli.main(["decompress", "compressed/b", "b2_rec.ply", CKPT, "--render", "b.png"])
    assert open("b2_rec.ply", "rb").read() == open("b_rec.ply", "rb").read() and os.path.getsize("b.png") > 1000


def test_scan_with_coded_colours(scan, monkeypatch):
    from pcgcv1_amd import test as cli
    d, points, colors, grid = scan
    monkeypatch.chdir(d)
    ingest.main(["--input", "scan.ply", "--output", "col_vox7.ply", "--bits", "7"])
    extra = [CKPT, "--colors", "raht", "--color_coder", "rans"]
    cli.main(["compress", "col_vox7.ply", "ca"] + extra)
    cli.main(["compress", "scan.ply", "cb"] + extra + ["--voxelize", "7"])
    for k in FIVE + ("colors",):
        assert open("compressed/cb." + k, "rb").read() == open("compressed/ca." + k, "rb").read(), k
    assert os.path.exists("compressed/cb.frame") and not os.path.exists("compressed/ca.frame")
    cli.main(["decompress", "compressed/ca", "ca_rec.ply", CKPT])
    cli.main(["decompress", "compressed/cb", "cb_rec.ply", CKPT])
    a_p, a_c = iop.load_ply_colors("ca_rec.ply")
    b_p, b_c, _ = iop.load_ply_scan("cb_rec.ply")
    assert b_c is not None and len(b_p) > 1000
    np.testing.assert_array_equal(b_c, a_c)
    np.testing.assert_array_equal(b_p, ingest.apply_frame(a_p, ingest.Frame(ORIGIN, STEP, 7)))
    # the refusals that need the file
    for more, word in ((["--scale=0.5"], "scale"), (["--gpu=2"], "gpu")):
        os.rename("compressed/cb.colors", "compressed/cb.colors_")
        try:
            with pytest.raises(SystemExit, match=word) as e:
                cli.main(["decompress", "compressed/cb", "x_rec.ply", CKPT] + more)
            assert "cb.frame" in str(e.value)
        finally:
            os.rename("compressed/cb.colors_", "compressed/cb.colors")


def test_scan_with_normals_feeds_pointnums_d2(scan, monkeypatch, capsys):
    """the merged normals reach --pointnums d2 as the voxelised ply would hand them on (six decimals)"""
    from pcgcv1_amd import test as cli
    d, points, colors, grid = scan
    monkeypatch.chdir(d)
    rng = np.random.default_rng(3)
    normals = points - points.mean(0) + rng.normal(0, 0.5, points.shape)
    normals = (normals / np.linalg.norm(normals, axis=1, keepdims=True)).astype(np.float32)
    fields = [(k, "<f4") for k in ("x", "y", "z", "nx", "ny", "nz")] + [(k, "u1") for k in ("red", "green", "blue")]
    v = np.zeros(len(points), np.dtype(fields))
    for k in range(3):
        v["xyz"[k]], v[("nx", "ny", "nz")[k]], v[("red", "green", "blue")[k]] = points[:, k], normals[:, k], colors[:, k]
    head = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % len(points) + "".join(
        "property %s %s\n" % ("float" if t == "<f4" else "uchar", k) for k, t in fields) + "end_header\n"
    with open("nscan.ply", "wb") as f:
        f.write(head.encode() + v.tobytes())
    ingest.main(["--input", "nscan.ply", "--output", "n_vox7.ply", "--bits", "7", "--attributes", "normals"])
    vox_p, vox_n = iop.load_ply_normals("n_vox7.ply")
    want = ref.voxelize_scan(points, None, normals, bits=7)
    np.testing.assert_array_equal(vox_p, grid)
    assert np.abs(vox_n - want[2]).max() <= 5.1e-7                                  # six decimals in the text
    ingest.main(["--input", "nscan.ply", "--output", "c_vox7.ply", "--bits", "7"])  # colours by default when it has both
    np.testing.assert_array_equal(iop.load_ply_colors("c_vox7.ply")[1], ref.voxelize_scan(points, colors, bits=7)[1])
    capsys.readouterr()
    cli.main(["compress", "n_vox7.ply", "na", CKPT, "--pointnums", "d2"])
    line_a = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("pointnums d2")]
    cli.main(["compress", "nscan.ply", "nb", CKPT, "--pointnums", "d2", "--voxelize", "7"])
    line_b = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("pointnums d2")]
    assert line_a == line_b and len(line_a) == 1
    for k in FIVE:
        assert open("compressed/nb." + k, "rb").read() == open("compressed/na." + k, "rb").read(), k
    assert os.path.exists("compressed/nb.frame") and not os.path.exists("compressed/na.frame")
