"""csrc/render.hip and pcgcv1_amd/render.py on the device against the rule in numpy (tests/_render_ref.py, whose two
statements of hidden-point removal tests/test_render_host.py holds against each other): rgb, index and depth bit for bit,
the launch geometry, ties, clipping, shading by hand, the colour map, compare, and the two command lines."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _render_ref as ref                                                # noqa: E402
from pcgcv1_amd import _lib, render, synthetic                           # noqa: E402
from pcgcv1_amd.dataprocess import inout_points as iop                   # noqa: E402

W, H = 96, 80                     # not square, neither side a multiple of 64
VIEWS = {"front": render.view_matrix("front"), "top": render.view_matrix("top"), "yaw30_pitch20": render.view_matrix("front", 30, 20)}
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _lib.require_gpu()


def _cloud():
    """2 000 float32 points in [0, 64)^3: a third fractional (half of those on odd multiples of 1/32, where p * 16 ends in
    .5 and the rounding goes to even), fifty exact duplicates of earlier points, a random colour each"""
    if "cloud" not in _CACHE:
        rng = np.random.default_rng(2024)
        p = rng.integers(0, 64, (2000, 3)).astype(np.float32)
        p[0:333] = (rng.integers(0, 64 * 16, (333, 3)) * 2 + 1).astype(np.float32) / np.float32(32.0)
        p[333:667] = rng.uniform(0, 63.99, (334, 3)).astype(np.float32)
        p[1950:] = p[rng.integers(0, 1950, 50)]
        p = p[rng.permutation(2000)]
        assert p.min() >= 0 and p.max() < 64 and len(np.unique(p, axis=0)) <= 1950
        assert ((p * 16 - np.floor(p * 16)) == 0.5).any(axis=1).sum() > 300
        _CACHE["cloud"] = (p, rng.integers(0, 256, (2000, 3)).astype(np.uint8))
    return _CACHE["cloud"]


def _zbuffer(key, *args):
    """the reference z-buffer of a case, computed once and left unchanged"""
    if key not in _CACHE:
        z = ref.zbuffer(*args)
        z.setflags(write=False)
        _CACHE[key] = z
    return _CACHE[key]


def _same(got, want, what):
    for name, g, w in zip(("rgb", "index", "depth"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        assert np.array_equal(g, w), (what, name, int((g != w).sum()))


@pytest.mark.parametrize("shade", [0, 64])
@pytest.mark.parametrize("view", sorted(VIEWS))
@pytest.mark.parametrize("point_size", [1, 3, 5, 15])
def test_against_the_reference_bit_for_bit(point_size, view, shade):
    p, c = _cloud()
    R = VIEWS[view]
    window = render.fit_window(p, R, W, H)
    z = _zbuffer(("main", view, point_size), p, R, window, W, H, point_size)
    want = ref.resolve(z, c, (255, 255, 255), (200, 200, 200), shade)
    assert (want[1] >= 0).sum() > 1000 and len(np.unique(want[1])) < 1900          # a picture, with hidden points
    got = render.render(p, c, size=(W, H), view=R, window=window, point_size=point_size, shade=shade, return_buffers=True)
    _same(got, want, (point_size, view, shade))
    plain = render.render(p, None, size=(W, H), view=R, window=window, point_size=point_size, shade=shade, foreground=(10, 200, 90),
                          background=(1, 2, 3))
    assert np.array_equal(plain, ref.resolve(z, None, (1, 2, 3), (10, 200, 90), shade)[0])


def _crowd():
    """300 000 points that all project into 40 x 40 pixels of the image: about 190 points per pixel at point_size 1"""
    if "crowd" not in _CACHE:
        rng = np.random.default_rng(7)
        p = rng.uniform(0, 63.9, (300000, 3)).astype(np.float32)
        c = rng.integers(0, 256, (300000, 3)).astype(np.uint8)
        window = render.Window(0, 1023, 1024, 2560, 28, 20)           # 0.625 pixels per voxel: 64 voxels = 40 pixels
        want = ref.render(p, c, VIEWS["front"], window, W, H, 3, shade=64)
        cov = np.argwhere(want[1] >= 0)
        assert cov.min(0).tolist() == [19, 27] and cov.max(0).tolist() == [60, 68]          # 40 x 40 and the squares' rim
        _CACHE["crowd"] = (p, c, window, want)
    return _CACHE["crowd"]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 300000])
def test_point_counts_around_the_launch_geometry(n):
    """one point, a wave less one, a wave, a wave and one, a workgroup and one; and more points than one pass of the
    grid-stride loop (2 048 workgroups of 256), crowded onto a few pixels"""
    if n == 300000:
        p, c, window, want = _crowd()
        got = render.render(p, c, size=(W, H), view=VIEWS["front"], window=window, point_size=3, shade=64, return_buffers=True)
        return _same(got, want, n)
    p, c = (a[:n] for a in _cloud())
    R = VIEWS["yaw30_pitch20"]
    window = render.fit_window(_cloud()[0], R, W, H)
    want = ref.render(p, c, R, window, W, H, 3, shade=64)
    assert len(np.unique(want[1][want[1] >= 0])) > 0.7 * n
    _same(render.render(p, c, size=(W, H), view=R, window=window, point_size=3, shade=64, return_buffers=True), want, n)


def test_two_runs_give_the_same_bytes():
    p, c, window, want = _crowd()
    runs = [render.render(p, c, size=(W, H), view=VIEWS["front"], window=window, point_size=3, shade=64, return_buffers=True)
            for _ in range(2)]
    for a, b in zip(*runs):
        assert a.tobytes() == b.tobytes()


def test_ties_go_to_the_lower_index_and_depth_beats_order():
    window = render.Window(0, 31 * 16, 16 * 16, 4096, 0, 0)           # one pixel per voxel: px = x, py = 31 - y, d = 256 - 16 z
    red, green = (255, 0, 0), (0, 255, 0)
    for colors in ((red, green), (green, red)):                        # equal pixel, equal depth, either order: index 0
        p = np.array([[10, 10, 5], [10, 10, 5]], np.float32)
        rgb, index, depth = render.render(p, np.array(colors, np.uint8), size=(32, 32), window=window, point_size=1, shade=0,
                                          return_buffers=True)
        assert index[21, 10] == 0 and depth[21, 10] == 176 and rgb[21, 10].tolist() == list(colors[0])
        assert (index >= 0).sum() == 1
    # the nearer point (toward the viewer = +z) comes later in the input and still wins; squares of 3 overlap in part
    p = np.array([[10, 10, 2], [11, 10, 8]], np.float32)
    c = np.array([red, green], np.uint8)
    got = render.render(p, c, size=(32, 32), window=window, point_size=3, shade=0, return_buffers=True)
    _same(got, ref.render(p, c, VIEWS["front"], window, 32, 32, 3), "nearer later")
    assert got[1][20:23, 9:13].tolist() == [[0, 1, 1, 1]] * 3 and got[2][21, 10] == 128 and got[2][21, 9] == 224


def test_clipping_and_untouched_surroundings():
    """a window at 4 pixels per voxel on the middle of the cloud: squares of 5 cross all four borders, most points fall
    outside altogether, and every point in front of the window's plane (d < 0) is dropped.  The outputs are slices of
    larger tensors; what lies before and behind them stays as it was."""
    p, c = _cloud()
    R = VIEWS["front"]
    window = render.Window(20 * 16, 44 * 16, 40 * 16, 16384, 0, 0)
    px, py, d, keep = ref.project(p, R, window)
    assert (d < 0).sum() > 500 and ((px < -2) | (px > W + 1) | (py < -2) | (py > H + 1)).sum() > 1000
    for lo, hi, n in ((px, px, W), (py, py, H)):
        assert ((lo >= -2) & (lo < 0) & keep).any() and ((hi >= n) & (hi < n + 2) & keep).any()      # centre outside, square inside
    want = ref.render(p, c, R, window, W, H, 5, shade=64)
    assert (want[1][0] >= 0).any() and (want[1][-1] >= 0).any() and (want[1][:, 0] >= 0).any() and (want[1][:, -1] >= 0).any()
    assert not np.isin(np.nonzero(~keep)[0], want[1]).any()
    dev = torch.device("cuda")
    pad = 64
    big = [torch.full((pad + H * W * k + pad,), fill, dtype=dt, device=dev)
           for k, fill, dt in ((3, 0xA5, torch.uint8), (1, -77, torch.int32), (1, -77, torch.int32))]
    out = (big[0][pad:pad + H * W * 3].view(H, W, 3), big[1][pad:pad + H * W].view(H, W), big[2][pad:pad + H * W].view(H, W))
    zbuf = render.splat(torch.from_numpy(p).to(dev), R, window, W, H, 5)
    render.resolve(zbuf, W, H, torch.from_numpy(c).to(dev), shade=64, out=out)
    _same([t.cpu().numpy() for t in out], want, "clipped")
    for t, fill in zip(big, (0xA5, -77, -77)):
        t = t.cpu().numpy()
        assert (t[:pad] == fill).all() and (t[-pad:] == fill).all()


def test_empty_cloud_is_the_background():
    rgb, index, depth = render.render(np.zeros((0, 3), np.float32), None, size=(W, H), background=(9, 8, 7), return_buffers=True)
    assert rgb.shape == (H, W, 3) and (rgb == np.array([9, 8, 7], np.uint8)).all()
    assert (index == -1).all() and (depth == -1).all()
    assert np.array_equal(render.render(np.zeros((0, 3)), np.zeros((0, 3), np.uint8), size=(W, H), background=(9, 8, 7)), rgb)


def test_shading_by_hand():
    """one pixel per voxel, px = x, py = 5 - y, d = 160 - 16 z, k = 64:
      A (0,5,10) in the image's corner, d 0, beside B (1,5,8), d 32: A's neighbours outside the image add nothing and B lies
        behind it: obs 0, factor 255.  B sees A 32 in front: factor 255*64 // 96 = 170; (200,100,50) -> (133,67,33)
      C (4,2,10) alone among uncovered pixels: factor 255
      D (4,4,10) d 0, E (5,4,5) d 80, F (6,4,5) d 80, a step of 80: E: 255*64 // 144 = 113, white -> 113; F beside E: 255"""
    window = render.Window(0, 80, 160, 4096, 0, 0)
    p = np.array([[0, 5, 10], [1, 5, 8], [4, 2, 10], [4, 4, 10], [5, 4, 5], [6, 4, 5]], np.float32)
    c = np.array([[255, 255, 255], [200, 100, 50], [10, 20, 30], [255, 255, 255], [255, 255, 255], [90, 80, 70]], np.uint8)
    rgb, index, depth = render.render(p, c, size=(8, 6), window=window, point_size=1, shade=64, background=(0, 0, 0), return_buffers=True)
    assert sorted(index[index >= 0].tolist()) == [0, 1, 2, 3, 4, 5]
    assert [index[0, 0], index[0, 1], index[3, 4], index[1, 4], index[1, 5], index[1, 6]] == [0, 1, 2, 3, 4, 5]
    assert [depth[0, 0], depth[0, 1], depth[1, 5]] == [0, 32, 80]
    assert rgb[0, 0].tolist() == [255, 255, 255]
    assert rgb[0, 1].tolist() == [(200 * 170 + 127) // 255, (100 * 170 + 127) // 255, (50 * 170 + 127) // 255] == [133, 67, 33]
    assert rgb[3, 4].tolist() == [10, 20, 30]
    assert rgb[1, 4].tolist() == [255, 255, 255] and rgb[1, 5].tolist() == [113, 113, 113] and rgb[1, 6].tolist() == [90, 80, 70]
    _same((rgb, index, depth), ref.render(p, c, VIEWS["front"], window, 8, 6, 1, background=(0, 0, 0), shade=64), "by hand")
    off = render.render(p, c, size=(8, 6), window=window, point_size=1, shade=0, background=(0, 0, 0))
    assert off[0, 1].tolist() == [200, 100, 50] and off[1, 5].tolist() == [255, 255, 255]


@pytest.mark.parametrize("n", [1, 65, 10001])
@pytest.mark.parametrize("vmax", [4.0, 0.5])
def test_colormap(n, vmax):
    """0, the float below a bin edge and the edge itself, vmax and ten times vmax, then random values up to 1.2 vmax
    (both scales 256 / vmax are exact in float32, so value * scale is an integer exactly at an edge)"""
    lut = render.colormap_lut()
    edge = np.float32(17 * vmax / 256)
    special = np.array([edge, np.nextafter(edge, np.float32(0)), 0, vmax, 10 * vmax, np.nextafter(np.float32(vmax), np.float32(0))], np.float32)
    rng = np.random.default_rng(n)
    v = np.concatenate([special, rng.uniform(0, 1.2 * vmax, n).astype(np.float32)])[:n]
    want = ref.colormap(v, vmax, lut)
    if n > 1:
        assert want[:6].tolist() == [lut[17].tolist(), lut[16].tolist(), lut[0].tolist(), lut[255].tolist(), lut[255].tolist(), lut[255].tolist()]
    got = render.error_colors(v, vmax)
    assert got.dtype == np.uint8 and got.shape == (n, 3) and np.array_equal(got, want)
    with pytest.raises(ValueError):
        render.error_colors(-v - 1, vmax)


def _surface():
    """a wavy sheet of 55 x 55 = 3 025 voxels cut to 3 000, and a copy without the 200 points of one corner (x < 20, y < 10)
    and with 100 others moved 3 voxels along z"""
    x, y = (a.reshape(-1) for a in np.meshgrid(np.arange(55), np.arange(55), indexing="ij"))
    z = np.rint(20 + 8 * np.sin(x / 9.0) * np.cos(y / 7.0))
    a = np.stack([x, y, z], 1).astype(np.float32)[:3000]
    gone = (a[:, 0] < 20) & (a[:, 1] < 10)
    assert gone.sum() == 200
    b = a[~gone].copy()
    b[np.random.default_rng(5).permutation(len(b))[:100], 2] += 3
    return a, b, gone


def test_compare_panels():
    from pcgcv1_amd import metrics
    a, b, gone = _surface()
    R = VIEWS["yaw30_pitch20"]
    colors = np.random.default_rng(1).integers(0, 256, (len(b), 3)).astype(np.uint8)
    image, figures = render.compare(a, b, colors, size=(W, H), view=R, vmax=4.0, point_size=3, shade=64, return_metrics=True)
    assert image.shape == (H, 3 * W, 3) and image.dtype == np.uint8
    want_figures, detail = metrics.pc_error_float(a, b, None, 1023, per_point=True)
    assert figures == want_figures
    b_unique, first = np.unique(b, axis=0, return_index=True)
    window = render.fit_window([a, b_unique], R, W, H)
    common = dict(size=(W, H), view=R, window=window, point_size=3, shade=64)
    lost = render.error_colors(np.sqrt(detail["1"][0]), 4.0)
    first_panel, index, _ = render.render(a, lost, return_buffers=True, **common)
    assert np.array_equal(image[:, :W], first_panel)
    assert np.array_equal(image[:, W:2 * W], render.render(b_unique, render.error_colors(np.sqrt(detail["2"][0]), 4.0), **common))
    assert np.array_equal(image[:, 2 * W:], render.render(b_unique, colors[first], **common))
    # what the codec lost shows in the first panel: the pixels that show removed points are not all blue (red or green
    # in them), the rest of the sheet away from the moved points is
    shows_gone = (index >= 0) & gone[np.maximum(index, 0)]
    assert shows_gone.sum() > 50
    assert (first_panel[shows_gone][:, :2].max(1) > 0).mean() > 0.8
    kept_exact = (index >= 0) & (detail["1"][0][np.maximum(index, 0)] == 0)
    assert kept_exact.sum() > 500 and not first_panel[kept_exact][:, :2].any()
    # without colours the third panel is the shaded foreground
    plain = render.compare(a, b, size=(W, H), view=R, point_size=3, shade=64)
    assert np.array_equal(plain[:, 2 * W:], render.render(b_unique, None, **common)) and np.array_equal(plain[:, :2 * W], image[:, :2 * W])


def test_command_line(tmp_path, capsys):
    a, b, _ = _surface()
    colors = np.random.default_rng(2).integers(0, 256, (len(b), 3)).astype(np.uint8)
    b = b + np.float32(0.25)                                  # a reconstruction with fractions, as scale != 1 writes them
    iop.write_ply_data(str(tmp_path / "a.ply"), a.astype(np.int32))
    iop.write_ply_colors(str(tmp_path / "b.ply"), b, colors)
    view = ["--size", str(W), str(H), "--yaw", "30", "--pitch", "20", "--up", "z"]
    R = render.view_matrix("front", 30, 20, "z")
    render.main(["--input", str(tmp_path / "b.ply"), "--output", str(tmp_path / "one.png")] + view)
    got = ref.png_pixels((tmp_path / "one.png").read_bytes())
    assert np.array_equal(got, render.render(b, colors, size=(W, H), view=R))
    assert len(np.unique(got.reshape(-1, 3), axis=0)) > 100
    render.main(["--input", str(tmp_path / "b.ply"), "--output", str(tmp_path / "flat.png"), "--no_shade", "--point_size", "5", "--view", "top",
                 "--size", "64", "48"])
    assert np.array_equal(ref.png_pixels((tmp_path / "flat.png").read_bytes()), render.render(b, colors, size=(64, 48), view="top", shade=0, point_size=5))
    capsys.readouterr()
    render.main(["--input", str(tmp_path / "b.ply"), "--output", str(tmp_path / "three.png"), "--compare", str(tmp_path / "a.ply"),
                 "--error_max", "2"] + view)
    out = capsys.readouterr().out
    assert "mseF,PSNR (p2point)" in out and "mse1      (p2point)" in out
    want = render.compare(a, b, colors, size=(W, H), view=R, vmax=2.0)
    assert want.shape == (H, 3 * W, 3) and np.array_equal(ref.png_pixels((tmp_path / "three.png").read_bytes()), want)


def test_decompress_render_flag(tmp_path, monkeypatch):
    """the smallest cloud the other command-line tests code (test_gpu_parity.test_cli_and_eval_end_to_end): decompress
    --render writes the same ply as without the flag, and the png is render() of that ply"""
    from pcgcv1_amd import test as cli
    pts = synthetic.make_cloud(seed=5, res=128, n_shells=3, rmin=0.2, rmax=0.4)
    ply = tmp_path / "tiny_vox7.ply"
    iop.write_ply_data(str(ply), pts)
    monkeypatch.chdir(tmp_path)
    cli.main(["compress", str(ply), "--ckpt_dir=synthetic:7:sparse", "--min_num=20"])
    cli.main(["decompress", "compressed/tiny_vox7", "plain_rec.ply", "--ckpt_dir=synthetic:7:sparse"])
    assert not (tmp_path / "tiny.png").exists()
    cli.main(["decompress", "compressed/tiny_vox7", "--ckpt_dir=synthetic:7:sparse", "--render", "tiny.png"])
    assert (tmp_path / "tiny_vox7_rec.ply").read_bytes() == (tmp_path / "plain_rec.ply").read_bytes()
    rec, colors = iop.load_ply_colors(str(tmp_path / "tiny_vox7_rec.ply"), as_float=True)
    assert colors is None and len(rec) > 1000
    image = ref.png_pixels((tmp_path / "tiny.png").read_bytes())
    assert image.shape == (1024, 1024, 3) and np.array_equal(image, render.render(rec))
    assert 0.05 < (image != 255).any(2).mean() < 0.9
    with pytest.raises(SystemExit):
        cli.main(["compress", str(ply), "--ckpt_dir=synthetic:7:sparse", "--min_num=20", "--render", "x.png"])
