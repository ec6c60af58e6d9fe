"""The component kernels (csrc/components.hip: pcgc_clean_components, called alone through clean.components) against the rule in
numpy (tests/_components_ref.py): label, size and n_components bit for bit, the two filters' masks exactly.  Then a raw scan
with dense clumps far from its surface end to end through the ingest command line and the codec's.

The snake is one path through the whole grid, so its only component is as long as it is large: label propagation by sweeps
would need as many sweeps as it has cells.  Cut in the middle it is two components whose smallest keys are known from the
construction."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _components_ref as ref                                            # noqa: E402
import _clean_ref as clean_ref                                           # noqa: E402
import _ingest_ref as ingest_ref                                         # noqa: E402
from pcgcv1_amd import _lib, clean, ingest                               # noqa: E402
from pcgcv1_amd.dataprocess import inout_points as iop                   # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _lib.require_gpu()


def _check(points, bits, gap, want=None):
    """label, size and n_components of one call against the rule, bit for bit -> the rule's (label, size, n_components)"""
    want = ref.components(points, bits, gap) if want is None else want
    label, size, n = clean.components(points, bits, gap)
    assert label.dtype == torch.int64 and label.shape == (len(points),)
    assert size.dtype == torch.int32 and size.shape == (len(points),)
    assert n.dtype == torch.int64 and n.shape == (1,)
    np.testing.assert_array_equal(label.cpu().numpy(), want[0])
    np.testing.assert_array_equal(size.cpu().numpy(), want[1])
    assert n.tolist() == [want[2]]
    return want


def _grid(bits, half, seed=0):
    res = 1 << bits
    p = np.stack(np.meshgrid(*[np.arange(res)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.int32)
    rng = np.random.default_rng(seed + bits)
    if half:
        p = p[rng.permutation(len(p))[:len(p) // 2]]
    return p[rng.permutation(len(p))]


def test_one_voxel_and_two_at_opposite_corners():
    for bits in (1, 6):
        R = (1 << bits) - 1
        for gap in (1, 8):
            want = _check(np.array([[0, 1, R]], np.int32), bits, gap)
            assert want[0].tolist() == [((0 << bits) + 1 << bits) + R] and want[1].tolist() == [1] and want[2] == 1
            want = _check(np.array([[R, R, R], [0, 0, 0]], np.int32), bits, gap)
            assert want[2] == (1 if R <= gap else 2)


def test_the_link_is_the_chebyshev_cube():
    at = np.array([20, 30, 40])
    for d, gap, n in (((1, 1, 1), 1, 1), ((1, -1, 1), 1, 1), ((2, 0, 0), 1, 2), ((2, 0, 0), 2, 1), ((0, 0, 2), 1, 2), ((0, -2, 2), 2, 1),
                      ((9, 0, 0), 8, 2), ((8, -8, 8), 8, 1), ((0, 0, 9), 8, 2), ((0, 9, 0), 8, 2)):
        for p in (np.array([at, at + d], np.int32), np.array([at + d, at], np.int32)):
            assert _check(p, 6, gap)[2] == n, (d, gap)


def test_nothing_wraps_into_the_next_row_plane_or_grid():
    for pair in (((0, 0, 7), (0, 1, 0)), ((0, 7, 3), (1, 0, 3)), ((7, 7, 7), (0, 0, 0)), ((3, 7, 7), (4, 0, 0))):
        want = _check(np.array(pair, np.int32), 3, 1)
        assert want[2] == 2 and want[1].tolist() == [1, 1]
    assert _check(np.array([[0, 0, 7], [0, 1, 0]], np.int32), 3, 7)[2] == 1


@pytest.mark.parametrize("half", [False, True], ids=["full", "half"])
@pytest.mark.parametrize("bits", [1, 2, 3])
def test_rows_shorter_than_a_word(bits, half):
    p = _grid(bits, half)
    for gap in (1, 2, 8):
        want = _check(p, bits, gap)
        if not half:                                                    # a full grid is one component with label 0
            assert want[2] == 1 and (want[0] == 0).all() and (want[1] == len(p)).all()


@pytest.mark.parametrize("n", [63, 65, 257])
def test_row_counts(n):
    p = _grid(4, False, seed=n)[:n]
    for gap in (1, 2):
        assert _check(p, 4, gap)[2] > 1


@pytest.fixture(scope="module")
def surface():
    """tests/test_gpu_clean.py's surface (3159 voxels, bits = 6), and the rule's answers per gap, computed once"""
    p = ref.surface()
    assert len(p) == 3159
    return p, {gap: ref.components(p, 6, gap) for gap in (1, 2, 3, 8)}


@pytest.mark.parametrize("gap, n_components", [(1, 768), (2, 28), (3, 22), (8, 6)])
def test_surface(surface, gap, n_components):
    p, want = surface
    assert want[gap][2] == n_components
    _check(p, 6, gap, want[gap])
    # the rows in another order: the same values per voxel; the same rows again: the same bytes
    order = np.random.default_rng(gap).permutation(len(p))
    _check(p[order], 6, gap, (want[gap][0][order], want[gap][1][order], n_components))
    for _ in range(2):
        label, size, n = clean.components(p, 6, gap)
        assert label.cpu().numpy().tobytes() == want[gap][0].tobytes() and size.cpu().numpy().tobytes() == want[gap][1].tobytes()
        assert n.item() == n_components


CUT_LABEL = {3: 6, 4: 10, 5: 18}


@pytest.mark.parametrize("bits, n", [(3, 143), (4, 1087), (5, 8447)])
def test_snake(bits, n):
    walk = ref.snake(bits)
    assert len(walk) == n
    order = np.random.default_rng(bits).permutation(n)
    whole = (np.zeros(n, np.int64), np.full(n, n, np.int32), 1)
    _check(walk, bits, 1, whole)
    _check(walk[order], bits, 1, whole)
    # cut: two components, the first from the cell with key 0, the second with the label the construction gives it
    at = n // 2 + 3
    cut = np.delete(walk, at, axis=0)
    want = (np.r_[np.zeros(at, np.int64), np.full(n - at - 1, CUT_LABEL[bits], np.int64)],
            np.r_[np.full(at, at, np.int32), np.full(n - at - 1, n - at - 1, np.int32)], 2)
    assert (at, n - at - 1) == {3: (74, 68), 4: (546, 540), 5: (4226, 4220)}[bits]
    if bits < 5:
        again = ref.components(cut, bits, 1)
        for a, b in zip(again, want):
            np.testing.assert_array_equal(a, b)
    _check(cut, bits, 1, want)
    order = np.random.default_rng(bits + 10).permutation(n - 1)
    _check(cut[order], bits, 1, (want[0][order], want[1][order], 2))
    _check(cut, bits, 2, (np.zeros(n - 1, np.int64), np.full(n - 1, n - 1, np.int32), 1))


def test_64_bit_cell_indices():
    """bits = 11: res^3 = 2^33 cells; test_gpu_clean.py's clusters at both ends of the key range, the far one up to the last cell"""
    rng = np.random.default_rng(33)
    far = 2047 - np.unique(rng.integers(0, 41, (300, 3)), axis=0)
    near = np.unique(rng.integers(0, 41, (300, 3)), axis=0)
    p = np.r_[far, near, [[2047, 2047, 2047], [0, 0, 0], [2047, 0, 2047]]]
    p = np.unique(p, axis=0).astype(np.int32)
    p = p[rng.permutation(len(p))]
    assert (p[:, 0].astype(np.int64) * 2048 * 2048).max() > 2 ** 32
    for gap in (1, 8):
        want = _check(p, 11, gap)
    assert want[0].max() > 2 ** 32 and 2 < want[2] < len(p)


def test_a_point_outside_the_grid_belongs_to_no_component():
    inside = _grid(3, True)
    p = np.r_[inside[:100], [[8, 0, 0]], inside[100:], [[-1, 3, 3]], [[2, 2, 1 << 20]]].astype(np.int32)
    out = np.array([100, len(p) - 2, len(p) - 1])
    for gap in (1, 2):
        label, size, n = clean.components(p, 3, gap)
        label, size = label.cpu().numpy(), size.cpu().numpy()
        assert label[out].tolist() == [-1] * 3 and size[out].tolist() == [0] * 3
        want = ref.components(inside, 3, gap)
        np.testing.assert_array_equal(np.delete(label, out), want[0])
        np.testing.assert_array_equal(np.delete(size, out), want[1])
        assert n.item() == want[2]


def test_rows_that_repeat_index_nothing_out_of_bounds():
    inside = _grid(3, True)
    p = np.r_[inside, inside[:50], inside[:7]].astype(np.int32)
    label, size, n = clean.components(p, 3, 1)
    want = ref.components(inside, 3, 1)
    pick = np.r_[np.arange(len(inside)), np.arange(50), np.arange(7)]
    np.testing.assert_array_equal(label.cpu().numpy(), want[0][pick])
    np.testing.assert_array_equal(size.cpu().numpy(), want[1][pick])              # a cell counts once
    assert n.item() == want[2]


def test_bad_arguments_touch_nothing():
    lib = _lib.hip()
    sized = lib.pcgc_clean_components_workspace_bytes
    assert sized(0, 10) == 0 and sized(13, 10) == 0 and sized(7, 0) == 0 and sized(7, 2 ** 31) == 0
    assert sized(7, 10) >= 2 * 128 ** 3 // 8 + 16 * 10 and sized(7, 1000) >= 2 * 128 ** 3 // 8 + 16 * 1000
    dev = _lib.require_gpu()
    n, bits = 8, 2
    p = torch.from_numpy(_grid(bits, False)[:n].copy()).to(dev)
    label = torch.full((n,), -7, dtype=torch.int64, device=dev)
    size = torch.full((n,), -7, dtype=torch.int32, device=dev)
    count = torch.full((1,), -7, dtype=torch.int64, device=dev)
    ws = torch.full((int(sized(bits, n)),), 0x5A, dtype=torch.uint8, device=dev)
    s = _lib.stream()

    def call(points=p, n=n, bits=bits, gap=1, label=label, size=size, count=count, ws=ws, ws_bytes=None):
        return lib.pcgc_clean_components(_lib.dptr(points), n, bits, gap, _lib.dptr(label), _lib.dptr(size), _lib.dptr(count), _lib.dptr(ws),
                                         ws.numel() if ws_bytes is None and ws is not None else (ws_bytes or 0), s)
    bad = [dict(points=None), dict(n=0), dict(n=2 ** 31), dict(bits=0), dict(bits=13), dict(gap=0), dict(gap=9), dict(gap=-1),
           dict(label=None), dict(ws=None), dict(ws_bytes=ws.numel() - 1)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert lib.pcgc_last_error().startswith(b"pcgc_clean_components")
    torch.cuda.synchronize()
    assert (label == -7).all() and (size == -7).all() and (count == -7).all() and (ws == 0x5A).all()
    want = ref.components(p.cpu().numpy(), bits, 1)
    assert call(size=None, count=None) == 0                              # size and n_components may be left out
    torch.cuda.synchronize()
    np.testing.assert_array_equal(label.cpu().numpy(), want[0])
    assert (size == -7).all() and (count == -7).all()
    assert call() == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(label.cpu().numpy(), want[0])
    np.testing.assert_array_equal(size.cpu().numpy(), want[1])
    assert count.tolist() == [want[2]]
    with pytest.raises(_lib.PcgcError, match="gap"):
        clean.components(p, bits, 9)
    with pytest.raises(ValueError):
        clean.components(p, 13)


# ---------------------------------------------------------------------------- masks
@pytest.mark.parametrize("spec", ["component:28", "component:6:2", "largest", "largest:2"])
def test_keep_mask_is_the_rules_mask(surface, spec):
    p = surface[0]
    want = ref.keep_mask(p, 6, spec)
    got = clean.keep_mask(p, 6, spec)
    assert got.dtype == np.bool_ and got.shape == (len(p),) and 0 < want.sum() < len(p)
    np.testing.assert_array_equal(got, want)
    report = []
    np.testing.assert_array_equal(clean.keep_mask(torch.from_numpy(p).cuda(), 6, clean.parse_spec(spec), report), want)
    gap = clean.parse_spec(spec).gap
    label, size, n = surface[1][gap]
    assert report == [clean.components_line(clean.parse_spec(spec), label, size)]
    assert report[0].startswith("components: %s saw %d components, the largest of %d " % (spec, n, size.max()))


def test_a_tie_for_the_largest_goes_to_the_smaller_label():
    block = np.stack(np.meshgrid(*[np.arange(2)] * 3, indexing="ij"), -1).reshape(-1, 3)
    p = np.r_[block + 4, block, [[0, 0, 3]], [[15, 15, 15]]].astype(np.int32)
    assert clean.keep_mask(p, 4, "largest").tolist() == [False] * 8 + [True] * 8 + [False, False]
    assert clean.keep_mask(p[::-1].copy(), 4, "largest").tolist() == [False, False] + [True] * 8 + [False] * 8
    assert clean.keep_mask(p, 4, "largest:2").tolist() == [False] * 8 + [True] * 9 + [False]
    assert clean.keep_mask(p, 4, "component:8").tolist() == [True] * 16 + [False, False]


def test_the_filters_in_order_and_nothing_left(surface):
    p = surface[0]
    specs = ["stat:8:2.0", "largest:2"]
    want = ref.keep_mask_all(p, 6, specs)
    assert 0 < want.sum() < ref.keep_mask(p, 6, specs[1]).sum()         # the first filter took some of the largest component
    report = []
    np.testing.assert_array_equal(clean.keep_mask_all(p, 6, specs, report), want)
    assert len(report) == 1 and report[0].startswith("components: largest:2 saw ")
    kept, _, _, _, mask = clean.clean_cloud(p, None, None, None, 6, specs)
    np.testing.assert_array_equal(mask, want)
    np.testing.assert_array_equal(kept, p[want])
    assert surface[1][1][1].max() == 125
    clean.keep_mask_all(p, 6, ["component:125"])
    with pytest.raises(ValueError, match="every voxel"):
        clean.keep_mask_all(p, 6, ["component:126"])
    with pytest.raises(ValueError, match="component:3100:8 removes every voxel"):
        clean.clean_cloud(p, None, None, None, 6, ["largest:8", "component:3100:8"])


# ---------------------------------------------------------------------------- end to end
FIVE = ("strings", "strings_head", "strings_hyper", "pointnums", "cubepos")
CKPT = "--ckpt_dir=synthetic:0"
STAT, ISLANDS = "stat:20:2.0", "component:100"
SHELL, CLUMP, STRAY = 0, 1, 2


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
    """a scan in scanner units as a binary ply: a sphere shell of radius 1, three dense clumps four to six radii away and 40
    strays; at 7 bits about 2900 voxels, the shell one component of about 2700 and the clumps 60 to 70 voxels each.  With the
    rule's answers for stat alone and for stat, then components."""
    rng = np.random.default_rng(11)
    d = rng.normal(size=(9000, 3))
    shell = d / np.linalg.norm(d, axis=1, keepdims=True) * (1.0 + rng.uniform(-0.01, 0.01, (9000, 1)))
    centres = np.array([[5.0, 0.6, -0.4], [-4.2, 4.4, 0.3], [0.5, -4.6, 4.1]])
    clumps = np.concatenate([c + rng.uniform(-0.12, 0.12, (400, 3)) for c in centres])
    strays = rng.uniform(-4.0, 4.0, (40, 3))
    points = (np.r_[shell, clumps, strays] + (2.0, -1.0, 0.5)).astype(np.float32).astype(np.float64)
    kind = np.r_[np.full(9000, SHELL), np.full(1200, CLUMP), np.full(40, STRAY)]
    order = rng.permutation(len(points))
    points, kind = points[order], kind[order]
    colors = rng.integers(0, 256, (len(points), 3)).astype(np.uint8)
    d = tmp_path_factory.mktemp("islands")
    _write_scan(str(d / "scan.ply"), points, colors)
    stat = clean_ref.voxelize_scan_clean(points, colors, bits=7, clean=[STAT])
    both = ref.voxelize_scan_clean(points, colors, bits=7, clean=[STAT, ISLANDS])
    return d, points, colors, kind, stat, both


def _cubes(p):
    return len(np.unique(np.asarray(p) >> 6, axis=0))


def test_scan_through_the_ingest_cli(scan, monkeypatch, capsys):
    d, points, colors, kind, stat, both = scan
    monkeypatch.chdir(d)
    # the existing filter alone: the strays go, every clump voxel stays; nothing new is printed
    assert stat[10][kind == CLUMP].all() and stat[10][kind == SHELL].all() and not stat[10][kind == STRAY].any()
    ingest.main(["--input", "scan.ply", "--output", "stat.ply", "--bits", "7", "--clean", STAT])
    said = capsys.readouterr().out.splitlines()
    assert len(said) == 3 and said[1].startswith("clean: %s removed 40 of " % STAT) and "components" not in "".join(said)
    got_p, got_c = iop.load_ply_colors("stat.ply")
    np.testing.assert_array_equal(got_p, stat[0])
    np.testing.assert_array_equal(got_c, stat[1])
    # with the component filter behind it exactly the clumps go as well, and the frame is fitted to the shell
    assert both[10][kind == SHELL].all() and not both[10][kind != SHELL].any()
    seen = stat[8]                                                       # what the component filter saw: pass 1's voxels that stat kept
    label, size, n = ref.components(seen, 7, 1)
    assert n == 4 and size.max() > 2000 and sorted(np.unique(size).tolist())[-2] < 100
    ingest.main(["--input", "scan.ply", "--output", "both.ply", "--bits", "7", "--clean", STAT, "--clean", ISLANDS])
    said = capsys.readouterr().out.splitlines()
    refit = ingest.Frame(*both[4])
    assert said[0] == ingest.summary_line(len(points), 0, both[3], refit)
    assert said[1] == "clean: %s %s removed %d of %d voxels (%d input points); 64^3 cubes %d -> %d" % (
        STAT, ISLANDS, both[6], len(both[8]) + both[6], both[7], _cubes(ingest_ref.voxelize_scan(points, bits=7)[0]), _cubes(both[0]))
    assert said[2] == clean.components_line(clean.parse_spec(ISLANDS), label, size)
    assert said[2].startswith("components: component:100 saw 4 components, the largest of %d " % size.max())
    assert said[3] == "wrote both.ply and both.frame" and len(said) == 4
    assert open("both.frame", "rb").read() == ingest.frame_bytes(refit)
    got_p, got_c = iop.load_ply_colors("both.ply")
    np.testing.assert_array_equal(got_p, both[0])
    np.testing.assert_array_equal(got_c, both[1])
    assert both[6] == stat[6] + int((size < 100).sum()) and both[7] == 1240
    assert refit.step < ingest.Frame(*stat[4]).step / 4                 # the resolution the clumps took is back
    assert refit.step == (points[kind == SHELL].max(0) - points[kind == SHELL].min(0)).max() / 127
    out = ingest.voxelize_scan(points, colors, bits=7, clean=[STAT, ISLANDS])
    assert len(out) == 8 and out[4] == refit and out[5:] == both[5:8]
    for k in (0, 1, 3):
        np.testing.assert_array_equal(out[k], both[k])


def test_scan_through_the_codec_cli(scan, monkeypatch, capsys):
    from pcgcv1_amd import test as cli
    d, points, colors, kind, stat, both = scan
    refit = ingest.Frame(*both[4])
    monkeypatch.chdir(d)
    extra = [CKPT, "--colors", "raht"]
    ingest.main(["--input", "scan.ply", "--output", "clean_vox7.ply", "--bits", "7", "--clean", STAT, "--clean", ISLANDS])
    capsys.readouterr()
    cli.main(["compress", "clean_vox7.ply", "ca"] + extra)
    assert "components" not in capsys.readouterr().out
    cli.main(["compress", "scan.ply", "cb", "--voxelize", "7", "--clean", STAT, "--clean", ISLANDS] + extra)
    said = capsys.readouterr().out
    assert "clean=[Spec('%s'), Spec('%s')]" % (STAT, ISLANDS) in said.splitlines()[0]
    assert "clean: %s %s removed %d of %d voxels (%d input points)" % (STAT, ISLANDS, both[6], len(both[8]) + both[6], both[7]) in said
    label, size, _ = ref.components(stat[8], 7, 1)
    lines = said.splitlines()
    at = [k for k, line in enumerate(lines) if line.startswith("clean: ")]
    assert len(at) == 1 and lines[at[0] + 1] == clean.components_line(clean.parse_spec(ISLANDS), label, size)
    assert open("compressed/cb.frame", "rb").read() == ingest.frame_bytes(refit)
    for k in FIVE + ("colors",):
        assert open("compressed/cb." + k, "rb").read() == open("compressed/ca." + k, "rb").read(), k
    cli.main(["decompress", "compressed/cb", "cb_rec.ply", CKPT])
    rec_p, rec_c, _ = iop.load_ply_scan("cb_rec.ply")
    assert rec_c is not None and len(rec_p) > 1000                       # the round trip completes, on the refitted frame's grid
    assert (rec_p >= refit.origin).all() and (rec_p <= refit.origin + refit.R * refit.step).all()
    assert np.abs(rec_p - (2.0, -1.0, 0.5)).max() < 2.5                  # the clumps, four radii out and more, are gone


def test_a_voxelised_ply_through_the_clean_cli(scan, monkeypatch, capsys):
    d, points, colors, kind, stat, both = scan
    monkeypatch.chdir(d)
    ingest.main(["--input", "scan.ply", "--output", "dirty_vox.ply", "--bits", "7"])
    vox_p, vox_c = iop.load_ply_colors("dirty_vox.ply")
    specs = [STAT, "largest"]
    mask = ref.keep_mask_all(vox_p, 7, specs)
    seen = vox_p[clean_ref.keep_mask(vox_p, STAT)]
    label, size, n = ref.components(seen, 7, 1)
    capsys.readouterr()
    clean.main(["--input", "dirty_vox.ply", "--output", "tidy_vox.ply", "--clean", specs[0], "--clean", specs[1]])
    line = clean.summary_line(specs, len(vox_p), int((~mask).sum()), _cubes(vox_p), _cubes(vox_p[mask]))
    assert capsys.readouterr().out == line + "\n" + clean.components_line(clean.parse_spec("largest"), label, size) + "\nwrote tidy_vox.ply\n"
    got_p, got_c = iop.load_ply_colors("tidy_vox.ply")
    np.testing.assert_array_equal(got_p, vox_p[mask])
    np.testing.assert_array_equal(got_c, vox_c[mask])
    assert mask.sum() == size.max() > 2000 and n == 4
    # compress --clean on the voxelised ply: the files of the cleaned ply, the same two lines, and no frame
    from pcgcv1_amd import test as cli
    extra = [CKPT, "--colors", "raht"]
    cli.main(["compress", "tidy_vox.ply", "ta"] + extra)
    assert "components" not in capsys.readouterr().out
    cli.main(["compress", "dirty_vox.ply", "tb", "--clean", specs[0], "--clean", specs[1]] + extra)
    assert line + "\n" + clean.components_line(clean.parse_spec("largest"), label, size) + "\nRead and clean" in capsys.readouterr().out
    for k in FIVE + ("colors",):
        assert open("compressed/tb." + k, "rb").read() == open("compressed/ta." + k, "rb").read(), k
    assert not os.path.exists("compressed/tb.frame")
