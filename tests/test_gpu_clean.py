"""The cleaning kernel (csrc/clean.hip: pcgc_clean_neighbors, called alone through clean.neighbor_statistics) against the rule in
numpy (tests/_clean_ref.py): S and cnt bit for bit, the two filters' masks exactly.  Then a raw scan with stray points end to
end through the ingest command line and the codec's.

The scan of the end-to-end tests is a sheet (a height field, as a scanner sees a wall or a relief), 1 % stray points in a box
three times its extent and one point about ten extents away on a diagonal.  With --bits the refit spends the whole grid on
what is kept, so the cleaned cloud never touches fewer than two 64^3 cubes along its longest axis at 7 bits, and a compact
surface would fill all eight.  The cubes get fewer here because the sheet fills four (2 x 2 x 1), while on the unclean grid
the far point holds one cube and the strays around the surface, which that point pushes to the middle of the y and z axes,
four more.  With --voxel_size the grid keeps its resolution and the strays' cubes simply go."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _clean_ref as ref                                                 # noqa: E402
import _ingest_ref as ingest_ref                                         # noqa: E402
from pcgcv1_amd import _lib, clean, ingest                               # noqa: E402
from pcgcv1_amd.dataprocess import inout_points as iop                   # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _lib.require_gpu()


def _check(points, bits, k, radius, want=None):
    """S and cnt of one call against the rule, bit for bit -> the rule's (S, cnt)"""
    want = ref.neighbor_statistics(points, k, radius) if want is None else want
    S, cnt = clean.neighbor_statistics(points, bits, k, radius)
    assert cnt.dtype == torch.int32 and cnt.shape == (len(points),)
    np.testing.assert_array_equal(cnt.cpu().numpy(), want[1])
    if k == 0:
        assert S is None
    else:
        assert S.dtype == torch.int64 and S.shape == (len(points),)
        np.testing.assert_array_equal(S.cpu().numpy(), want[0])
    return want


def _grid(bits, half, seed=0):
    res = 1 << bits
    p = np.stack(np.meshgrid(*[np.arange(res)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.int32)
    rng = np.random.default_rng(seed + bits)
    if half:
        p = p[rng.permutation(len(p))[:len(p) // 2]]
    return p[rng.permutation(len(p))]


@pytest.mark.parametrize("half", [False, True], ids=["full", "half"])
@pytest.mark.parametrize("bits", [1, 2, 3])
def test_rows_shorter_than_a_word_and_a_ball_larger_than_the_grid(bits, half):
    p = _grid(bits, half)
    for k, radius in ((1, 1), (8, 2), (5, 3), (64, 32), (0, 32)):
        want = _check(p, bits, k, radius)
        if radius == 32:                                                # the ball holds the whole grid
            assert (want[1] == len(p) - 1).all()


@pytest.fixture(scope="module")
def surface():
    """bits = 6: about 3000 voxels of a sphere that the grid's faces cut (flat caps on x = 0, y = 63 and z = 0), a filled 5^3
    block (more than 64 neighbours within 8 cells), plus 30 scattered ones; the rule's answers per (k, R), computed once"""
    rng = np.random.default_rng(21)
    d = rng.normal(size=(6000, 3))
    p = np.rint((30, 36, 28) + 33.0 * d / np.linalg.norm(d, axis=1, keepdims=True))
    p = np.clip(p, 0, 63)
    p = np.unique(p, axis=0)
    p = p[rng.permutation(len(p))[:3000]]
    block = np.stack(np.meshgrid(*[np.arange(30, 35)] * 3, indexing="ij"), -1).reshape(-1, 3)
    p = np.unique(np.r_[p, block, rng.integers(0, 64, (30, 3)), [[0, 0, 0], [63, 63, 63], [0, 63, 31], [32, 0, 63]]], axis=0).astype(np.int32)
    p = p[rng.permutation(len(p))]
    assert 3000 < len(p) < 3200 and p.min() == 0 and p.max() == 63
    return p, {}


@pytest.mark.parametrize("radius", [1, 2, 8, 32])
@pytest.mark.parametrize("k", [1, 8, 64])
def test_surface_with_scattered_points(surface, k, radius):
    p, cache = surface
    cache[k, radius] = _check(p, 6, k, radius)
    cnt = cache[k, radius][1]
    if radius == 8:
        assert cnt.max() > 64 > cnt.min()                               # both the k nearest of many and k > cnt occur


def test_s_only_cnt_only_and_both_agree_and_a_call_repeats_itself(surface):
    p, cache = surface
    want = cache.get((8, 8)) or ref.neighbor_statistics(p, 8, 8)
    both = clean.neighbor_statistics(p, 6, 8, 8)
    s_only = clean.neighbor_statistics(p, 6, 8, 8, want_counts=False)
    c_only = clean.neighbor_statistics(p, 6, 0, 8)
    again = clean.neighbor_statistics(p, 6, 8, 8)
    assert s_only[1] is None and c_only[0] is None
    for S in (both[0], s_only[0], again[0]):
        assert S.cpu().numpy().tobytes() == want[0].tobytes()
    for cnt in (both[1], c_only[1], again[1]):
        assert cnt.cpu().numpy().tobytes() == want[1].tobytes()


def test_one_voxel_and_two_at_opposite_corners():
    for bits in (1, 6):
        S, cnt = clean.neighbor_statistics(np.array([[0, 1, (1 << bits) - 1]], np.int32), bits, 8, 8)
        assert S.tolist() == [8 * (9 << 16)] and cnt.tolist() == [0]
    for bits, radius in ((1, 1), (1, 2), (2, 5), (2, 6), (5, 32), (9, 32)):
        R = (1 << bits) - 1
        want = _check(np.array([[R, R, R], [0, 0, 0]], np.int32), bits, 3, radius)
        assert want[1].tolist() == [int(3 * R * R <= radius * radius)] * 2


def test_64_bit_cell_indices():
    """bits = 11: res^3 = 2^33 cells; clusters at both ends of the key range, the far one up to the last cell"""
    rng = np.random.default_rng(33)
    far = 2047 - np.unique(rng.integers(0, 41, (300, 3)), axis=0)
    near = np.unique(rng.integers(0, 41, (300, 3)), axis=0)
    p = np.r_[far, near, [[2047, 2047, 2047], [0, 0, 0], [2047, 0, 2047]]]
    p = np.unique(p, axis=0).astype(np.int32)
    p = p[rng.permutation(len(p))]
    assert (p[:, 0].astype(np.int64) * 2048 * 2048).max() > 2 ** 32
    for k, radius in ((8, 8), (64, 32), (1, 1)):
        want = _check(p, 11, k, radius)
    assert want[1].max() > 0


def test_a_point_outside_the_grid_is_nobodys_neighbour():
    inside = _grid(3, True)
    p = np.r_[inside[:100], [[8, 0, 0]], inside[100:], [[-1, 3, 3]], [[2, 2, 1 << 20]]].astype(np.int32)
    S, cnt = clean.neighbor_statistics(p, 3, 6, 2)
    S, cnt = S.cpu().numpy(), cnt.cpu().numpy()
    out = np.array([100, len(p) - 2, len(p) - 1])
    assert S[out].tolist() == [6 * (3 << 16)] * 3 and cnt[out].tolist() == [0, 0, 0]
    want = ref.neighbor_statistics(inside, 6, 2)
    np.testing.assert_array_equal(np.delete(S, out), want[0])
    np.testing.assert_array_equal(np.delete(cnt, out), want[1])


def test_bad_arguments_touch_nothing():
    lib = _lib.hip()
    assert lib.pcgc_clean_workspace_bytes(0, 10) == 0 and lib.pcgc_clean_workspace_bytes(13, 10) == 0
    assert lib.pcgc_clean_workspace_bytes(7, 0) == 0 and lib.pcgc_clean_workspace_bytes(7, 2 ** 31) == 0
    assert lib.pcgc_clean_workspace_bytes(7, 10) >= 128 ** 3 // 8
    dev = _lib.require_gpu()
    n, bits = 8, 2
    p = torch.from_numpy(_grid(bits, False)[:n].copy()).to(dev)
    S = torch.full((n,), -7, dtype=torch.int64, device=dev)
    cnt = torch.full((n,), -7, dtype=torch.int32, device=dev)
    ws = torch.full((int(lib.pcgc_clean_workspace_bytes(bits, n)),), 0x5A, dtype=torch.uint8, device=dev)
    s = _lib.stream()

    def call(points=p, n=n, bits=bits, k=4, radius=2, S=S, cnt=cnt, ws=ws, ws_bytes=None):
        return lib.pcgc_clean_neighbors(_lib.dptr(points), n, bits, k, radius, _lib.dptr(S), _lib.dptr(cnt), _lib.dptr(ws),
                                        ws.numel() if ws_bytes is None and ws is not None else (ws_bytes or 0), s)
    bad = [dict(points=None), dict(n=0), dict(n=2 ** 31), dict(bits=0), dict(bits=13), dict(k=-1), dict(k=65), dict(radius=0),
           dict(radius=33), dict(S=None, cnt=None), dict(k=0), dict(ws=None), dict(ws_bytes=ws.numel() - 1)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert lib.pcgc_last_error().startswith(b"pcgc_clean_neighbors")
    torch.cuda.synchronize()
    assert (S == -7).all() and (cnt == -7).all() and (ws == 0x5A).all()
    assert call() == 0 and call(k=0, S=None) == 0 and call(cnt=None) == 0
    torch.cuda.synchronize()
    want = ref.neighbor_statistics(p.cpu().numpy(), 4, 2)
    np.testing.assert_array_equal(S.cpu().numpy(), want[0])
    np.testing.assert_array_equal(cnt.cpu().numpy(), want[1])
    with pytest.raises(_lib.PcgcError, match="radius"):
        clean.neighbor_statistics(p, bits, 4, 33)
    with pytest.raises(ValueError):
        clean.neighbor_statistics(p, bits, 0, 2, want_counts=False)


SPECS = ["radius:2:5", "radius:1:1", "stat:8:2.0", "stat:20:1.0:4", "stat:1:0:32", "stat:64:0.5"]


@pytest.mark.parametrize("spec", SPECS)
def test_keep_mask_is_the_rules_mask(surface, spec):
    p = surface[0]
    want = ref.keep_mask(p, spec)
    got = clean.keep_mask(p, 6, spec)
    assert got.dtype == np.bool_ and got.shape == (len(p),) and 0 < want.sum() < len(p)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(clean.keep_mask(torch.from_numpy(p).cuda(), 6, clean.parse_spec(spec)), want)


def test_clean_cloud_applies_the_specs_in_order(surface):
    p = surface[0]
    rng = np.random.default_rng(2)
    colors = rng.integers(0, 256, (len(p), 3)).astype(np.uint8)
    normals = rng.normal(size=(len(p), 3)).astype(np.float32)
    counts = rng.integers(1, 9, len(p)).astype(np.int32)
    specs = ["radius:2:4", "stat:8:2.0"]
    want = ref.keep_mask_all(p, specs)
    first = ref.keep_mask(p, specs[0])
    assert want.sum() < first.sum() < len(p) and not np.array_equal(want, first & ref.keep_mask(p, specs[1]))     # the order matters
    kept, c, nrm, cn, mask = clean.clean_cloud(p, colors, normals, counts, 6, specs)
    np.testing.assert_array_equal(mask, want)
    for got, full in ((kept, p), (c, colors), (nrm, normals), (cn, counts)):
        np.testing.assert_array_equal(got, full[want])                  # the kept rows, in their order
    assert clean.clean_cloud(p, None, None, None, 6, specs[:1])[1:4] == (None, None, None)
    with pytest.raises(ValueError, match="every voxel"):
        clean.clean_cloud(p, None, None, None, 6, ["radius:1:26"])


# ---------------------------------------------------------------------------- end to end
FIVE = ("strings", "strings_head", "strings_hyper", "pointnums", "cubepos")
CKPT = "--ckpt_dir=synthetic:0"
SPEC = "stat:8:2.0"
MODES = {"bits": (["--bits", "7"], dict(bits=7)), "voxel_size": (["--voxel_size", "0.03125"], dict(voxel_size=0.03125))}


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
    """the scan of the module's docstring as a binary ply of float32 coordinates, and the rule's answers for both modes"""
    rng = np.random.default_rng(5)
    xy = rng.uniform(-0.5, 0.5, (20000, 2))
    surf = np.c_[xy, 0.15 * np.sin(4 * xy[:, 0]) * np.cos(3 * xy[:, 1])]
    ext = surf.max(0) - surf.min(0)
    strays = rng.uniform(-1.5, 1.5, (200, 3)) * ext
    far = np.array([[-8.0, -4.75, -4.75]]) * ext.max()
    points = (np.r_[surf, strays, far] + (2.0, -1.0, 0.5)).astype(np.float32).astype(np.float64)
    order = np.r_[rng.permutation(len(points) - 1), len(points) - 1]      # the far point stays the last row
    points = points[order]
    colors = rng.integers(0, 256, (len(points), 3)).astype(np.uint8)
    d = tmp_path_factory.mktemp("dirty")
    _write_scan(str(d / "scan.ply"), points, colors)
    want = {m: ref.voxelize_scan_clean(points, colors, clean=[SPEC], **kw) for m, (_, kw) in MODES.items()}
    return d, points, colors, want, ext.max()


def _cubes(p):
    return len(np.unique(np.asarray(p) >> 6, axis=0))


@pytest.mark.parametrize("mode", ["bits", "voxel_size"])
def test_scan_through_the_ingest_cli(scan, mode, monkeypatch, capsys):
    d, points, colors, want, extent = scan
    argv, kw = MODES[mode]
    want = want[mode]
    monkeypatch.chdir(d)
    # without --clean: what the command wrote before it knew the flag
    ingest.main(["--input", "scan.ply", "--output", mode + "_plain.ply"] + argv)
    plain = ingest_ref.voxelize_scan(points, colors, **kw)
    frame = ingest.Frame(*plain[4])
    assert capsys.readouterr().out == "%s\nwrote %s_plain.ply and %s_plain.frame\n" % (ingest.summary_line(len(points), 0, plain[3], frame), mode, mode)
    iop.write_ply_colors("expect.ply", plain[0], plain[1])
    assert open(mode + "_plain.ply", "rb").read() == open("expect.ply", "rb").read()
    assert open(mode + "_plain.frame", "rb").read() == ingest.frame_bytes(frame)
    out = ingest.voxelize_scan(points, colors, **kw)
    assert len(out) == 6 and out[4] == frame and out[5] == 0
    for k in (0, 1, 3):
        np.testing.assert_array_equal(out[k], plain[k])
    # with it: the rule's points, colours, counts and frame, bit for bit
    ingest.main(["--input", "scan.ply", "--output", mode + ".ply", "--clean", SPEC] + argv)
    said = capsys.readouterr().out.splitlines()
    refit = ingest.Frame(*want[4])
    assert open(mode + ".frame", "rb").read() == ingest.frame_bytes(refit)
    got_p, got_c = iop.load_ply_colors(mode + ".ply")
    np.testing.assert_array_equal(got_p, want[0])
    np.testing.assert_array_equal(got_c, want[1])
    out = ingest.voxelize_scan(points, colors, clean=SPEC, **kw)
    assert len(out) == 8 and out[2] is None and out[4] == refit and out[5:] == want[5:8] and out[6] > 0 and out[7] >= out[6]
    for k in (0, 1, 3):
        assert out[k].dtype == want[k].dtype
        np.testing.assert_array_equal(out[k], want[k])
    vox1, row_keep = want[8], want[10]
    assert said[0] == ingest.summary_line(len(points), 0, want[3], refit)
    assert said[1] == "clean: %s removed %d of %d voxels (%d input points); 64^3 cubes %d -> %d" % (
        SPEC, want[6], len(vox1) + want[6], want[7], _cubes(plain[0]), _cubes(want[0]))
    # the refitted frame is that of the kept rows; the far point is gone
    kept = points[row_keep]
    assert refit.origin.tolist() == (kept.min(0) if mode == "bits" else np.floor(kept.min(0) / 0.03125) * 0.03125).tolist()
    assert refit.step == ((kept.max(0) - kept.min(0)).max() / 127 if mode == "bits" else 0.03125)
    assert not row_keep[-1] and row_keep.sum() == len(points) - want[7]
    back = ingest.apply_frame(got_p, refit)
    assert np.abs(back - (2.0, -1.0, 0.5)).max() < 2 * extent < np.abs(points[-1] - (2.0, -1.0, 0.5)).max()
    print("64^3 cubes without --clean: %d, with: %d" % (_cubes(plain[0]), _cubes(got_p)))
    assert _cubes(got_p) < _cubes(plain[0])
    if mode == "bits":
        assert got_p.min(0).tolist() == [0, 0, 0] and got_p.max() == 127
        assert refit.step < frame.step / 3                               # the resolution the far point took is back
    else:
        # the kept voxels of pass 1, shifted by whole cells into fewer bits
        first = ingest.Frame(*want[9])
        shift = (first.origin - refit.origin) / 0.03125
        assert (shift == np.rint(shift)).all() and refit.bits < first.bits == frame.bits
        np.testing.assert_array_equal(got_p, vox1 + shift.astype(np.int32))


def test_scan_through_the_codec_cli(scan, monkeypatch, capsys):
    from pcgcv1_amd import test as cli
    d, points, colors, want, extent = scan
    want = want["bits"]
    refit = ingest.Frame(*want[4])
    monkeypatch.chdir(d)
    extra = [CKPT, "--colors", "raht"]
    # without --clean: the files of the voxelised ply, as before; nothing about cleaning is printed
    ingest.main(["--input", "scan.ply", "--output", "plain_vox7.ply", "--bits", "7"])
    capsys.readouterr()
    cli.main(["compress", "plain_vox7.ply", "pa"] + extra)
    cli.main(["compress", "scan.ply", "pb", "--voxelize", "7"] + extra)
    assert "clean" not in capsys.readouterr().out
    for k in FIVE + ("colors",):
        assert open("compressed/pb." + k, "rb").read() == open("compressed/pa." + k, "rb").read(), k
    assert open("compressed/pb.frame", "rb").read() == open("plain_vox7.frame", "rb").read()
    # with it: the refit path; the frame that is written is the refitted one
    cli.main(["compress", "scan.ply", "cb", "--voxelize", "7", "--clean", SPEC] + extra)
    said = capsys.readouterr().out
    assert "clean=[Spec('%s')]" % SPEC in said.splitlines()[0]
    assert "clean: %s removed %d of %d voxels (%d input points)" % (SPEC, want[6], len(want[8]) + want[6], want[7]) in said
    assert open("compressed/cb.frame", "rb").read() == ingest.frame_bytes(refit)
    ingest.main(["--input", "scan.ply", "--output", "clean_vox7.ply", "--bits", "7", "--clean", SPEC])
    cli.main(["compress", "clean_vox7.ply", "ca"] + extra)
    for k in FIVE + ("colors",):
        assert open("compressed/cb." + k, "rb").read() == open("compressed/ca." + k, "rb").read(), k
    cli.main(["decompress", "compressed/cb", "cb_rec.ply", CKPT])
    rec_p, rec_c, _ = iop.load_ply_scan("cb_rec.ply")
    assert rec_c is not None and len(rec_p) > 1000                       # the round trip completes
    # in scan units: on the refitted frame's lattice, inside its grid (the synthetic weights decode voxels anywhere in a cube
    # that is coded, so the kept rows' own bounds say nothing), which the unclean frame's far corner is not
    assert (rec_p >= refit.origin).all() and (rec_p <= refit.origin + refit.R * refit.step).all()
    assert np.abs(rec_p - (2.0, -1.0, 0.5)).max() < 3 * extent
    np.testing.assert_allclose(rec_p, ingest.apply_frame(np.rint((rec_p - refit.origin) / refit.step), refit), rtol=0, atol=1e-5)


def test_a_voxelised_ply_through_the_clean_cli_and_the_codec(scan, monkeypatch, capsys):
    from pcgcv1_amd import test as cli
    d, points, colors, _, _ = scan
    monkeypatch.chdir(d)
    ingest.main(["--input", "scan.ply", "--output", "dirty_vox.ply", "--voxel_size", "0.03125"])
    vox_p, vox_c = iop.load_ply_colors("dirty_vox.ply")
    specs = [SPEC, "radius:2:4"]
    mask = ref.keep_mask_all(vox_p, specs)
    capsys.readouterr()
    clean.main(["--input", "dirty_vox.ply", "--output", "tidy_vox.ply", "--clean", specs[0], "--clean", specs[1]])
    line = clean.summary_line(specs, len(vox_p), int((~mask).sum()), _cubes(vox_p), _cubes(vox_p[mask]))
    assert capsys.readouterr().out == line + "\nwrote tidy_vox.ply\n"
    got_p, got_c = iop.load_ply_colors("tidy_vox.ply")
    np.testing.assert_array_equal(got_p, vox_p[mask])
    np.testing.assert_array_equal(got_c, vox_c[mask])
    assert _cubes(got_p) < _cubes(vox_p) and 0 < (~mask).sum() < 400
    # compress --clean on the voxelised ply: the files of the cleaned ply, and no frame
    extra = [CKPT, "--colors", "raht"]
    cli.main(["compress", "tidy_vox.ply", "ta"] + extra)
    cli.main(["compress", "dirty_vox.ply", "tb", "--clean", specs[0], "--clean", specs[1]] + extra)
    assert line in capsys.readouterr().out
    for k in FIVE + ("colors",):
        assert open("compressed/tb." + k, "rb").read() == open("compressed/ta." + k, "rb").read(), k
    assert not os.path.exists("compressed/tb.frame")
