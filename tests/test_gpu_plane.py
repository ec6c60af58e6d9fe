"""The plane kernels (csrc/plane.hip: pcgc_plane_count and pcgc_plane_select, called through the C ABI) against the rule in numpy
(tests/_plane_ref.py): counts, masks and sums bit for bit.  Then clean.keep_mask on a table with a sphere on it, and that scene
as a raw scan through the three command lines."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _plane_ref as ref                                                 # noqa: E402
import _ingest_ref as ingest_ref                                         # noqa: E402
from pcgcv1_amd import _lib, clean, ingest                               # noqa: E402
from pcgcv1_amd.dataprocess import inout_points as iop                   # noqa: E402

# csrc/plane.hip: "kPlanePointTile = 2048 points per workgroup ... against kPlaneChunk = 64 planes per workgroup"
POINT_TILE, PLANE_CHUNK = 2048, 64


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _lib.require_gpu()


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype))).cuda()


def _count(points, bits, planes):
    """pcgc_plane_count on canary-filled counts -> host int32 [K]"""
    p, q = _dev(points, np.int32).reshape(-1, 3), _dev(planes, np.int64).reshape(-1, 5)
    counts = torch.full((len(q),), -7, dtype=torch.int32, device=p.device)
    rc = _lib.hip().pcgc_plane_count(_lib.dptr(p), len(p), bits, _lib.dptr(q), len(q), _lib.dptr(counts), _lib.stream())
    assert rc == 0, _lib.hip().pcgc_last_error()
    return counts.cpu().numpy()


def _select(points, bits, plane, sums=True):
    """pcgc_plane_select on canary-filled outputs -> host (mask uint8 [n], sums int64 [10] | None)"""
    p, q = _dev(points, np.int32).reshape(-1, 3), _dev(plane, np.int64).reshape(5)
    mask = torch.full((len(p),), 0x5A, dtype=torch.uint8, device=p.device)
    ten = torch.full((10,), -7, dtype=torch.int64, device=p.device) if sums else None
    rc = _lib.hip().pcgc_plane_select(_lib.dptr(p), len(p), bits, _lib.dptr(q), _lib.dptr(mask), _lib.dptr(ten), _lib.stream())
    assert rc == 0, _lib.hip().pcgc_last_error()
    return mask.cpu().numpy(), None if ten is None else ten.cpu().numpy()


def _cloud(n, bits, seed):
    """n distinct voxels near a tilted slab, so that a draw's count is neither 0 nor n, in a random order"""
    rng = np.random.default_rng(seed)
    res = 1 << bits
    xy = rng.permutation(res * res)[:n]
    x, y = xy // res, xy % res
    z = np.clip(res // 3 + (x + 2 * y) // 8 + rng.integers(-2, 3, n), 0, res - 1)
    return np.stack([x, y, z], 1).astype(np.int32)


# ---------------------------------------------------------------------------- pcgc_plane_count
@pytest.mark.parametrize("n", [1, 3, 63, 64, 65, POINT_TILE + 1, 2 * POINT_TILE + 300])
def test_counts_are_the_rules(n):
    bits = 7
    p = _cloud(n, bits, n)
    draws = ref.draw_planes(p, 3, PLANE_CHUNK + 1, n)
    # a plane that holds every point, one that holds none, and one whose coefficients need the 64-bit products
    wide = np.array([[3 << 40, -(5 << 41), 7 << 44, (7 << 44) * (1 << bits) // 3, 1 << 50]], np.int64)
    planes = np.r_[[[0, 0, 1, 0, 1000]], draws[:PLANE_CHUNK - 2], [[0, 0, 0, 0, -1]], wide, draws[PLANE_CHUNK - 2:]]
    assert len(planes) == PLANE_CHUNK + 4
    want = ref.counts(p, bits, planes)
    assert want[0] == n and want[PLANE_CHUNK - 1] == 0
    if n > 64:
        assert 0 < want[PLANE_CHUNK] < n and (want[1:PLANE_CHUNK - 1] > 2).any()
    order = np.random.default_rng(n + 1).permutation(n)
    for K in (1, 2, PLANE_CHUNK + 1, len(planes)):
        got = _count(p, bits, planes[:K])
        assert got.dtype == np.int32
        np.testing.assert_array_equal(got, want[:K])
        assert _count(p, bits, planes[:K]).tobytes() == got.tobytes()
        np.testing.assert_array_equal(_count(p[order], bits, planes[:K]), want[:K])
    np.testing.assert_array_equal(_count(p, bits, planes[PLANE_CHUNK:]), want[PLANE_CHUNK:])
    np.testing.assert_array_equal(clean.plane_counts(p, bits, planes).cpu().numpy(), want)


def _diagonal_cloud():
    """bits = 12: the eight corners, points along the grid's diagonals and a few hundred anywhere"""
    rng = np.random.default_rng(4095)
    corners = np.stack(np.meshgrid(*[[0, 4095]] * 3, indexing="ij"), -1).reshape(-1, 3)
    t = rng.integers(0, 4096, 200)
    p = np.r_[corners, np.stack([t, t, t], 1), np.stack([t, 4095 - t, t], 1), rng.integers(0, 4096, (300, 3))]
    return np.unique(p, axis=0)[rng.permutation(len(np.unique(p, axis=0)))].astype(np.int32)


def test_the_extremes_at_12_bits():
    p = _diagonal_cloud()
    corner = lambda c: int(np.flatnonzero((p == c).all(1))[0])
    assert p.min() == 0 and p.max() == 4095
    planes = ref.draw_planes(p, 64, 200, 12)
    # triples that span the grid: two opposite corners and a third, so that |(a, b, c)| and |s| are as large as they get
    spans = []
    for third in ([4095, 0, 0], [0, 4095, 0], [0, 4095, 4095], [4095, 4095, 0]):
        tri = p[[corner([0, 0, 0]), corner([4095, 4095, 4095]), corner(third)]].astype(np.int64)
        a, b, c = [int(v) for v in np.cross(tri[1] - tri[0], tri[2] - tri[0])]
        spans.append([a, b, c, 0, ref.threshold(64, a * a + b * b + c * c)])
    tri = np.array([[0, 0, 4095], [4095, 1, 4095], [1, 4095, 0]], np.int64)
    a, b, c = [int(v) for v in np.cross(tri[1] - tri[0], tri[2] - tri[0])]
    far = [a, b, c, a * 0 + b * 0 + c * 4095, ref.threshold(64, a * a + b * b + c * c)]
    assert max(abs(a), abs(b), abs(c)) > 2 ** 23 and far[4] > 2 ** 28
    s = p.astype(np.int64) @ np.array(far[:3]) - far[3]
    assert np.abs(s).max() > 2 ** 31
    # the same plane moved so that one point lies exactly on |s| == T, then on T + 1, on either side
    q = p[len(p) // 2].astype(np.int64)
    sq = int(q @ np.array(far[:3])) - far[3]
    edge = [far[:3] + [far[3] + sq - sign * (far[4] + k), far[4]] for sign in (1, -1) for k in (0, 1)]
    planes = np.r_[planes, spans, [far], edge].astype(np.int64)
    want = ref.counts(p, 12, planes)
    np.testing.assert_array_equal(_count(p, 12, planes), want)
    assert (want[200:204] >= 2).all() and want.max() < len(p)
    for k, plane in enumerate(edge):
        mask, ten = _select(p, 12, plane)
        inside = ref.inliers(p, 12, plane)
        assert bool(mask[len(p) // 2]) == inside[len(p) // 2] == (k % 2 == 0)
        np.testing.assert_array_equal(mask, inside.astype(np.uint8))
        np.testing.assert_array_equal(ten, ref.sums(p, inside))
    # the smallest normal there is: z = 100 from three neighbours, D = 32: the layers 68 .. 132 and not 67 or 133
    col = np.array([[7, 9, z] for z in (66, 67, 68, 100, 132, 133, 134)], np.int32)
    flat = ref.draw_planes(np.array([[0, 0, 100], [1, 0, 100], [0, 1, 100]]), 64, 64, 0)
    live = flat[flat[:, 4] >= 0]
    assert len(live) and (np.abs(live[:, 2]) == 1).all() and (live[:, 4] == 32).all()
    assert _count(col, 12, live[:1]).tolist() == [3]
    assert _select(col, 12, live[0])[0].tolist() == [0, 0, 1, 1, 1, 0, 0]


def test_no_threshold_and_points_outside_the_grid():
    bits = 6
    inside = _cloud(500, bits, 5)
    p = np.r_[inside[:100], [[64, 3, 3]], inside[100:], [[3, -1, 3]], [[3, 3, 1 << 20]], [[-(1 << 31), 0, 0]]].astype(np.int32)
    out = np.array([100, len(p) - 3, len(p) - 2, len(p) - 1])
    planes = np.array([[0, 0, 0, 0, -1], [0, 0, 0, 0, 0], [1, 2, 3, 0, -1], [0, 0, 1, 0, 1 << 40], [0, 0, 0, 0, -(1 << 62)]], np.int64)
    assert _count(p, bits, planes).tolist() == [0, 500, 0, 500, 0] == ref.counts(p, bits, planes).tolist()
    for plane in planes:
        mask, ten = _select(p, bits, plane)
        want = ref.inliers(p, bits, plane)
        assert not want[out].any() and want.sum() in (0, 500)
        np.testing.assert_array_equal(mask, want.astype(np.uint8))
        np.testing.assert_array_equal(ten, ref.sums(p, want))
    # bits = 12: the cell next to the last one is outside
    p = np.array([[4095, 4095, 4095], [4096, 0, 0], [0, 4096, 0], [0, 0, -1]], np.int32)
    assert _count(p, 12, planes[3:4]).tolist() == [1] and _select(p, 12, planes[3])[0].tolist() == [1, 0, 0, 0]


# ---------------------------------------------------------------------------- pcgc_plane_select
@pytest.mark.parametrize("n", [1, 65, 5000, 2048 * 256 + 77])
def test_select_mask_and_sums(n):
    """a draw's plane and a refit plane with the coefficients a cloud of 2^31 voxels would give it; the last n is past what one
    pass of the grid covers"""
    bits = 12 if n > 5000 else 7
    p = _cloud(n, bits, n + 2)
    if n > 5000:
        p[:, 2] += 2000                                                  # large coordinates: the squares' sums pass 2^32
    draws = ref.draw_planes(p, 3, 64, n)
    score = ref.counts(p[:5000], bits, draws)
    plane = draws[int(np.argmax(score))] if score.max() else np.array([0, 0, 1, int(p[0, 2]), 0], np.int64)
    inside = ref.inliers(p, bits, plane)
    assert inside.any()
    ten = ref.sums(p, inside)
    scale = (2 ** 31 - 1) // int(ten[0])
    wide = ref.refit(ten * scale, 3)[0]
    assert 2 ** 44 < np.abs(wide[:3]).max() < 2 ** 47 and wide[4] < 2 ** 54
    for q in (plane, wide):
        want = ref.inliers(p, bits, q)
        assert 0 < want.sum() and (n < 100 or want.sum() < n)
        mask, got = _select(p, bits, q)
        assert mask.dtype == np.uint8 and got.dtype == np.int64
        np.testing.assert_array_equal(mask, want.astype(np.uint8))
        np.testing.assert_array_equal(got, ref.sums(p, want))
        assert got[0] == _count(p, bits, q[None])[0]
        again, none = _select(p, bits, q, sums=False)                    # sums may be left out
        assert none is None and again.tobytes() == mask.tobytes()
    mask, got = clean.plane_select(p, bits, wide)
    np.testing.assert_array_equal(mask.cpu().numpy(), ref.inliers(p, bits, wide).astype(np.uint8))
    np.testing.assert_array_equal(got.cpu().numpy(), ref.sums(p, ref.inliers(p, bits, wide)))
    assert clean.plane_select(p, bits, wide, want_sums=False)[1] is None
    np.testing.assert_array_equal(clean.refit_plane(ten, 3), ref.refit(ten, 3)[0])


def test_bad_arguments_touch_nothing():
    lib = _lib.hip()
    dev = _lib.require_gpu()
    n, bits, K = 8, 3, 2
    p = _dev(_cloud(n, bits, 0), np.int32)
    planes = _dev([[0, 0, 1, 2, 100], [0, 0, 0, 0, -1]], np.int64)
    counts = torch.full((K,), -7, dtype=torch.int32, device=dev)
    mask = torch.full((n,), 0x5A, dtype=torch.uint8, device=dev)
    ten = torch.full((10,), -7, dtype=torch.int64, device=dev)
    s = _lib.stream()

    def count(points=p, n=n, bits=bits, planes=planes, K=K, counts=counts):
        return lib.pcgc_plane_count(_lib.dptr(points), n, bits, _lib.dptr(planes), K, _lib.dptr(counts), s)

    def select(points=p, n=n, bits=bits, plane=planes, mask=mask, ten=ten):
        return lib.pcgc_plane_select(_lib.dptr(points), n, bits, _lib.dptr(plane), _lib.dptr(mask), _lib.dptr(ten), s)
    for kw in (dict(points=None), dict(planes=None), dict(counts=None), dict(n=0), dict(n=-1), dict(n=2 ** 31), dict(K=0), dict(K=65537),
               dict(K=-1), dict(bits=0), dict(bits=13)):
        assert count(**kw) == -1, kw
        assert lib.pcgc_last_error().startswith(b"pcgc_plane_count")
    for kw in (dict(points=None), dict(plane=None), dict(mask=None), dict(n=0), dict(n=2 ** 31), dict(bits=0), dict(bits=13)):
        assert select(**kw) == -1, kw
        assert lib.pcgc_last_error().startswith(b"pcgc_plane_select")
    torch.cuda.synchronize()
    assert (counts == -7).all() and (mask == 0x5A).all() and (ten == -7).all()
    assert count() == 0 and select() == 0
    torch.cuda.synchronize()
    assert counts.tolist() == [n, 0] and mask.tolist() == [1] * n and ten[0].item() == n
    assert select(ten=None) == 0
    with pytest.raises(_lib.PcgcError, match="pcgc_plane_count"):
        clean.plane_counts(p, 13, planes)


# ---------------------------------------------------------------------------- the filter
SPECS = ("plane:1.5:0.05:256:0", "plane:0.5", "plane:4:0.9")


@pytest.fixture(scope="module")
def scene():
    """tests/_plane_ref.py's table with a sphere on it, its rows shuffled, and the rule's answer per spec, computed once"""
    vox, is_table = ref.scene()
    assert (len(vox), int(is_table.sum())) == (ref.SCENE_VOXELS, ref.SCENE_TABLE)
    order = np.random.default_rng(3).permutation(len(vox))
    vox, is_table = vox[order], is_table[order]
    return vox, is_table, {spec: ref.segment(vox, 7, *ref.parse_spec(spec)[1:]) for spec in SPECS}


@pytest.mark.parametrize("spec", SPECS)
def test_keep_mask_is_the_rules_mask(scene, spec):
    vox, is_table, answers = scene
    plane, inside, info = answers[spec]
    want = ~inside if info["dropped"] else np.ones(len(vox), bool)
    got = clean.keep_mask(vox, 7, spec)
    assert got.dtype == np.bool_ and got.shape == (len(vox),)
    np.testing.assert_array_equal(got, want)
    report = []
    np.testing.assert_array_equal(clean.keep_mask(torch.from_numpy(vox).cuda(), 7, clean.parse_spec(spec), report), want)
    assert report == [clean.plane_line(clean.parse_spec(spec), plane, info)]
    found, mask, told = clean.segment_plane(vox, 7, spec)
    np.testing.assert_array_equal(found, plane)
    np.testing.assert_array_equal(mask.cpu().numpy(), inside.astype(np.uint8))
    assert told == info
    if spec == "plane:4:0.9":
        assert want.all() and "no plane holds 0.9 of the voxels" in report[0] and not info["dropped"] and info["count"] > 20000
    else:
        assert info["dropped"] and report[0].startswith("plane: %s dropped normal (-0.1" % spec)
        assert (~want)[~is_table].mean() <= 0.02 and (~want)[is_table].mean() >= (0.98 if spec == SPECS[0] else 0.3)


def test_no_plane_at_all():
    p = np.array([[3, 4, 5], [9, 9, 9]], np.int32)
    report = []
    assert clean.keep_mask(p, 4, "plane:1.5", report).tolist() == [True, True]
    assert report == ["plane: plane:1.5 no plane holds 0.05 of the voxels: none of 1024 draws spans a plane"]
    plane, mask, info = clean.segment_plane(p[:1], 4, "plane:1:0.5:7")
    assert plane is None and mask.tolist() == [0] and info == dict(n=1, draws=7, best_count=0, count=0, dropped=False)


def test_the_filters_in_order(scene):
    vox, is_table, _ = scene
    specs = ["plane:1.5:0.05:256", "largest"]
    want = ref.keep_mask_all(vox, 7, specs)
    assert want[~is_table].mean() >= 0.98 and want[is_table].mean() <= 0.005
    report = []
    np.testing.assert_array_equal(clean.keep_mask_all(vox, 7, specs, report), want)
    assert len(report) == 2 and report[0].startswith("plane: plane:1.5:0.05:256 dropped ") and report[1].startswith("components: largest saw ")
    kept, _, _, _, mask = clean.clean_cloud(vox, None, None, None, 7, specs)
    np.testing.assert_array_equal(mask, want)
    np.testing.assert_array_equal(kept, vox[want])
    flat = np.stack(np.meshgrid(np.arange(16), np.arange(16), [5], indexing="ij"), -1).reshape(-1, 3).astype(np.int32)
    with pytest.raises(ValueError, match="plane:0.5 removes every voxel"):
        clean.keep_mask_all(flat, 4, ["plane:0.5"])


# ---------------------------------------------------------------------------- end to end
FIVE = ("strings", "strings_head", "strings_hyper", "pointnums", "cubepos")
CKPT = "--ckpt_dir=synthetic:0"
PLANE, CHAIN = "plane:1.5:0.05:256", ["plane:1.5:0.05:256", "largest"]


def _write_scan(filename, points, colors):
    v = np.zeros(len(points), np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")]))
    for k, name in enumerate(("x", "y", "z")):
        v[name] = points[:, k]
    for k, name in enumerate(("red", "green", "blue")):
        v[name] = colors[:, k]
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
            "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n" % len(points))
    with open(filename, "wb") as f:
        f.write(head.encode() + v.tobytes())


@pytest.fixture(scope="module")
def scan(tmp_path_factory):
    """the scene's samples in scanner units (a cell = 5 mm, moved off the origin) as a binary ply with colours, every fourth of
    them; with the rule's answer for the plane filter and `largest` behind it at 7 bits"""
    samples, from_table = ref.scene_samples()
    samples, from_table = samples[::4], from_table[::4]
    points = (samples * 0.005 + (1.0, -2.0, 0.25)).astype(np.float32).astype(np.float64)
    colors = np.random.default_rng(5).integers(0, 256, (len(points), 3)).astype(np.uint8)
    d = tmp_path_factory.mktemp("table")
    _write_scan(str(d / "scan.ply"), points, colors)
    return d, points, colors, from_table, ref.voxelize_scan_clean(points, colors, bits=7, clean=CHAIN)


def _cubes(p):
    return len(np.unique(np.asarray(p) >> 6, axis=0))


def test_scan_through_the_ingest_cli(scan, monkeypatch, capsys):
    d, points, colors, from_table, want = scan
    monkeypatch.chdir(d)
    seen = ingest_ref.voxelize_scan(points, bits=7)[0]                   # pass 1's voxels: what the filter saw
    plane, inside, info = ref.segment(seen, 7, 3, 0.05, 256, 0)
    assert info["dropped"] and want[6] >= inside.sum() > 0.5 * len(seen)
    # by input row the table goes, and of the sphere the cap of about 2 of its 46 cells that lies within the table's slab
    assert want[10][~from_table].mean() > 0.95 and want[10][from_table].mean() < 0.001
    ingest.main(["--input", "scan.ply", "--output", "clean.ply", "--bits", "7", "--clean", CHAIN[0], "--clean", CHAIN[1]])
    said = capsys.readouterr().out.splitlines()
    refit = ingest.Frame(*want[4])
    assert said[0] == ingest.summary_line(len(points), 0, want[3], refit)
    assert said[1] == "clean: %s %s removed %d of %d voxels (%d input points); 64^3 cubes %d -> %d" % (
        CHAIN[0], CHAIN[1], want[6], len(seen), want[7], _cubes(seen), _cubes(want[0]))
    assert said[2] == clean.plane_line(clean.parse_spec(PLANE), plane, info) and said[2].startswith("plane: %s dropped normal (" % PLANE)
    assert said[3].startswith("components: largest saw ")
    assert said[4] == "wrote clean.ply and clean.frame" and len(said) == 5
    # the frame is fitted again to what is left: the sphere, less than half as wide as the table
    assert open("clean.frame", "rb").read() == ingest.frame_bytes(refit)
    assert refit.step < ingest.Frame(*want[9]).step / 2
    got_p, got_c = iop.load_ply_colors("clean.ply")
    np.testing.assert_array_equal(got_p, want[0])
    np.testing.assert_array_equal(got_c, want[1])


def test_scan_through_the_codec_cli(scan, monkeypatch, capsys):
    from pcgcv1_amd import test as cli
    d, points, colors, from_table, want = scan
    monkeypatch.chdir(d)
    extra = [CKPT, "--colors", "raht"]
    ingest.main(["--input", "scan.ply", "--output", "clean_vox7.ply", "--bits", "7", "--clean", CHAIN[0], "--clean", CHAIN[1]])
    plane_said = capsys.readouterr().out.splitlines()[2]
    cli.main(["compress", "clean_vox7.ply", "ca"] + extra)
    assert "plane: " not in capsys.readouterr().out
    cli.main(["compress", "scan.ply", "cb", "--voxelize", "7", "--clean", CHAIN[0], "--clean", CHAIN[1]] + extra)
    lines = capsys.readouterr().out.splitlines()
    assert "clean=[Spec('%s'), Spec('%s')]" % tuple(CHAIN) in lines[0]
    at = [k for k, line in enumerate(lines) if line.startswith("clean: ")]
    assert len(at) == 1 and lines[at[0] + 1] == plane_said and plane_said.startswith("plane: %s dropped normal (" % PLANE)
    assert lines[at[0] + 2].startswith("components: largest saw ")
    assert open("compressed/cb.frame", "rb").read() == ingest.frame_bytes(ingest.Frame(*want[4]))
    for k in FIVE + ("colors",):
        assert open("compressed/cb." + k, "rb").read() == open("compressed/ca." + k, "rb").read(), k


def test_a_voxelised_ply_through_the_clean_cli(scan, monkeypatch, capsys):
    d, points, colors, from_table, want = scan
    monkeypatch.chdir(d)
    ingest.main(["--input", "scan.ply", "--output", "dirty_vox.ply", "--bits", "7"])
    vox_p, vox_c = iop.load_ply_colors("dirty_vox.ply")
    specs = CHAIN
    plane, inside, info = ref.segment(vox_p, 7, 3, 0.05, 256, 0)
    mask = ref.keep_mask_all(vox_p, 7, specs)
    assert info["dropped"] and 0 < mask.sum() <= (~inside).sum()
    capsys.readouterr()
    clean.main(["--input", "dirty_vox.ply", "--output", "tidy_vox.ply", "--clean", specs[0], "--clean", specs[1]])
    said = capsys.readouterr().out.splitlines()
    assert said[0] == clean.summary_line(specs, len(vox_p), int((~mask).sum()), _cubes(vox_p), _cubes(vox_p[mask]))
    assert said[1] == clean.plane_line(clean.parse_spec(PLANE), plane, info)
    assert said[2].startswith("components: largest saw ") and said[3] == "wrote tidy_vox.ply" and len(said) == 4
    got_p, got_c = iop.load_ply_colors("tidy_vox.ply")
    np.testing.assert_array_equal(got_p, vox_p[mask])
    np.testing.assert_array_equal(got_c, vox_c[mask])
    # compress --clean on the voxelised ply prints the same lines
    from pcgcv1_amd import test as cli
    cli.main(["compress", "dirty_vox.ply", "tb", "--clean", specs[0], "--clean", specs[1], CKPT, "--colors", "raht"])
    assert "\n".join(said[:3]) + "\nRead and clean" in capsys.readouterr().out
