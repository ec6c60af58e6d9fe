"""The host side of pcgcv1_amd/render.py and the numpy statement of its rule (tests/_render_ref.py): the two statements of
hidden-point removal against each other, the named views on a hand-computed point, the view matrix, the colour table and
the png writer.  No GPU."""
import os
import struct
import sys
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _render_ref as ref                                                # noqa: E402
from pcgcv1_amd import render                                            # noqa: E402


@pytest.mark.parametrize("point_size", [1, 3, 5])
def test_minimum_key_and_painting_agree(point_size):
    """np.minimum.at on the keys and painting far to near give the same z-buffer: 500 points, a fifth of them fractional,
    in an image small enough that most pixels see several points and squares cross every border"""
    rng = np.random.default_rng(11)
    pts = rng.integers(0, 32, (500, 3)).astype(np.float32)
    pts[::5] += rng.uniform(-0.5, 0.5, (100, 3)).astype(np.float32)
    R = render.view_matrix("front", 30, 20)
    window = render.fit_window(pts, R, 48, 40, margin=0)
    a = ref.zbuffer(pts, R, window, 48, 40, point_size)
    b = ref.zbuffer_painter(pts, R, window, 48, 40, point_size)
    covered = a != ref.EMPTY
    assert covered.sum() > 300 and len(np.unique(a[covered])) < covered.sum() + 1
    assert 0 < len(np.unique(a[covered] & np.uint64(0xFFFFFFFF))) < 500          # some points are hidden
    assert np.array_equal(a, b)


# p = (3, 5, 9) in a window of 2 pixels per voxel: px = 32 + 2 right, py = 32 - 2 up, d = 256 - 16 toward
_WINDOW = (-256, 256, 256, 8192, 0, 0)
_EXPECT = {                       # view -> (px, py, d), from the rows right, up, toward the viewer of each view
    "front": (38, 22, 112),       # right x = 3, up y = 5, toward z = 9
    "back": (26, 22, 400),        # right -x, up y, toward -z
    "right": (14, 22, 208),       # right -z, up y, toward x
    "left": (50, 22, 304),        # right z, up y, toward -x
    "top": (38, 50, 176),         # right x, up -z, toward y
    "bottom": (38, 14, 336),      # right x, up z, toward -y
}


@pytest.mark.parametrize("view", sorted(_EXPECT))
def test_named_views_put_a_point_on_the_hand_computed_pixel(view):
    px, py, d = _EXPECT[view]
    z = ref.zbuffer(np.array([[3.0, 5.0, 9.0]], np.float32), render.view_matrix(view), _WINDOW, 64, 64, 1)
    assert np.argwhere(z != ref.EMPTY).tolist() == [[py, px]], view
    assert int(z[py, px]) == d << 32, view


def test_up_z_and_quarter_turns():
    """up = "z": right x, up z, toward the viewer -y; yaw 90 from front is the right view, pitch 90 the top view"""
    z = ref.zbuffer(np.array([[3.0, 5.0, 9.0]], np.float32), render.view_matrix("front", up="z"), _WINDOW, 64, 64, 1)
    assert np.argwhere(z != ref.EMPTY).tolist() == [[14, 38]] and int(z[14, 38]) == 336 << 32
    assert np.array_equal(render.view_matrix("front", yaw=90), render.view_matrix("right"))
    assert np.array_equal(render.view_matrix("front", yaw=180), render.view_matrix("back"))
    assert np.array_equal(render.view_matrix("front", yaw=270), render.view_matrix("left"))
    assert np.array_equal(render.view_matrix("front", pitch=90), render.view_matrix("top"))
    assert np.array_equal(render.view_matrix("front", pitch=-90), render.view_matrix("bottom"))
    with pytest.raises(ValueError):
        render.view_matrix("sideways")
    with pytest.raises(ValueError):
        render.view_matrix("front", up="x")


def test_view_matrix_is_orthonormal_to_the_rounding():
    """every entry is within e = 2^-15 of a rotation's: a dot product of two rows is then within 3 (2 e + e^2) of 0 or 1"""
    R = render.view_matrix("front", yaw=30, pitch=20)
    assert R.dtype == np.int64 and R.shape == (3, 3)
    r = R.astype(np.float64) / 16384.0
    e = 0.5 / 16384.0
    err = np.abs(r @ r.T - np.eye(3)).max()
    print("largest |R R^T - I| %.3g, bound %.3g" % (err, 3 * (2 * e + e * e)))
    assert err <= 3 * (2 * e + e * e)
    assert np.linalg.det(r) > 0.999
    assert R[0, 1] == 0 and R[0, 0] == int(np.rint(np.cos(np.deg2rad(30)) * 16384))       # yaw keeps the right axis level


def test_fit_window_and_default_point_size():
    pts = np.array([[0, 0, 0], [100, 50, 7], [20, 10, -3]], np.float32)
    R = render.view_matrix("front")
    w = render.fit_window([pts[:2], pts[2:]], R, 200, 120, margin=10)
    assert w.scale == (100 << 16) // 1601 and (w.u0, w.v1, w.w1) == (0, 800, 112)
    px, py, d, keep = ref.project(pts, R, w)
    assert keep.all() and d.min() == 0
    # centred: the same room left and right, above and below, to within the pixel the halving drops
    assert abs(int(px.min()) - (199 - int(px.max()))) <= 1 and abs(int(py.min()) - (119 - int(py.max()))) <= 1
    assert px.min() >= 10 and py.min() >= 10 and px.max() <= 189 and py.max() <= 109
    assert render.fit_window([np.zeros((0, 3), np.float32)], R, 64, 64) == render.Window(0, 0, 0, 1 << 16, 0, 0)
    with pytest.raises(ValueError):
        render.fit_window(pts, R, 16, 16, margin=8)
    # scale / 4096 = pixels per voxel; the smallest odd p with p >= sqrt(3) scale / 4096: 3 * 2364^2 <= 2^24 < 3 * 2365^2,
    # 3 * 7094^2 <= 9 * 2^24 < 3 * 7095^2
    for scale, want in ((1024, 1), (2364, 1), (2365, 3), (4096, 3), (7094, 3), (7095, 5), (8192, 5), (32768, 15), (409600, 15)):
        assert render.default_point_size(render.Window(0, 0, 0, scale, 0, 0)) == want, scale


def test_colormap_lut_against_the_anchors():
    anchors = [(0, (0, 0, 255)), (64, (0, 255, 255)), (128, (0, 255, 0)), (192, (255, 255, 0)), (255, (255, 0, 0))]
    want = np.zeros((256, 3), np.uint8)
    for (i0, c0), (i1, c1) in zip(anchors[:-1], anchors[1:]):
        for i in range(i0, i1 + 1):
            for ch in range(3):
                v = Fraction(c0[ch]) + Fraction((c1[ch] - c0[ch]) * (i - i0), i1 - i0)
                want[i, ch] = int(np.floor(v + Fraction(1, 2)))                       # half up
    lut = render.colormap_lut()
    assert lut.dtype == np.uint8 and lut.shape == (256, 3)
    assert np.array_equal(lut, want)
    assert lut[0].tolist() == [0, 0, 255] and lut[128].tolist() == [0, 255, 0] and lut[255].tolist() == [255, 0, 0]


def test_launch_wrappers_reject_bad_arguments_before_any_launch():
    """every argument include/pcgc.h rules out comes back as an error with a message, on the host: the pointers below are
    never dereferenced (none of these calls reaches the device, so the test needs none)"""
    import ctypes
    from pcgcv1_amd import _lib
    lib = _lib.hip()
    rot = np.ascontiguousarray(render.view_matrix("front").reshape(9), np.int32)
    buf = np.zeros(64, np.uint64)                             # stands in for every device pointer: aligned, never read
    p, r = _lib.nptr(buf), _lib.nptr(rot)
    need = lib.pcgc_render_workspace_bytes(96, 80)
    assert need == 96 * 80 * 8 and lib.pcgc_render_workspace_bytes(8192, 8192) == 8192 * 8192 * 8
    for w, h in ((0, 80), (96, 0), (8193, 80), (96, 8193), (-1, -1)):
        assert lib.pcgc_render_workspace_bytes(w, h) == 0, (w, h)

    def splat(points=p, n=10, rotation=r, window=(0, 0, 0, 4096, 0, 0), size=(96, 80), point_size=3, ws=p, ws_bytes=need):
        return lib.pcgc_render_splat(points, n, rotation, *window, size[0], size[1], point_size, ws, ws_bytes, None)

    def resolve(ws=p, ws_bytes=need, size=(96, 80), n=10, bg=0xFFFFFF, fg=0, shade=64, rgb=p, index=p, depth=p):
        return lib.pcgc_render_resolve(ws, ws_bytes, size[0], size[1], None, n, bg, fg, shade, rgb, index, depth, None)
    big = np.ascontiguousarray(rot * 2)
    odd, odd2 = ctypes.c_void_p(buf.ctypes.data + 4), ctypes.c_void_p(buf.ctypes.data + 2)
    bad = [splat(points=None), splat(rotation=None), splat(ws=None), splat(size=(0, 80)), splat(size=(96, 8193)), splat(point_size=0),
           splat(point_size=2), splat(point_size=17), splat(point_size=-1), splat(n=-1), splat(n=2 ** 32 - 1), splat(ws_bytes=need - 1),
           splat(ws=odd), splat(rotation=_lib.nptr(big)), splat(window=(2 ** 31, 0, 0, 4096, 0, 0)), splat(window=(0, 0, 0, 0, 0, 0)),
           splat(window=(0, 0, 0, 2 ** 30 + 1, 0, 0)), splat(window=(0, 0, 0, 4096, 2 ** 20 + 1, 0)),
           resolve(ws=None), resolve(rgb=None), resolve(size=(96, 0)), resolve(ws_bytes=need - 1), resolve(n=2 ** 32 - 1),
           resolve(shade=-1), resolve(shade=2 ** 20 + 1), resolve(bg=0x1000000), resolve(index=odd2), resolve(depth=odd2),
           lib.pcgc_colormap(None, 5, 64.0, p, p, None), lib.pcgc_colormap(p, 5, 64.0, None, p, None),
           lib.pcgc_colormap(p, 5, 64.0, p, None, None), lib.pcgc_colormap(p, -1, 64.0, p, p, None),
           lib.pcgc_colormap(p, 5, float("nan"), p, p, None), lib.pcgc_colormap(p, 5, -1.0, p, p, None)]
    assert bad == [-1] * len(bad), bad
    assert splat(point_size=2) == -1 and b"point_size" in lib.pcgc_last_error()
    assert lib.pcgc_colormap(None, 0, 64.0, None, None, None) == 0          # an empty input is a no-op that touches nothing


@pytest.mark.parametrize("width,height", [(1, 1), (3, 2), (96, 80)])
def test_write_png(tmp_path, width, height):
    rng = np.random.default_rng(width)
    img = rng.integers(0, 256, (height, width, 3)).astype(np.uint8)
    name = str(tmp_path / "a.png")
    render.write_png(name, img)
    data = open(name, "rb").read()
    chunks = ref.png_chunks(data)                                    # signature and every chunk's CRC
    assert [k for k, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    assert chunks[0][1] == struct.pack(">IIBBBBB", width, height, 8, 2, 0, 0, 0)
    assert np.array_equal(ref.png_pixels(data), img)
    for bad in (img[:, :, :2], img.astype(np.int32), img[0]):
        with pytest.raises(ValueError):
            render.write_png(name, bad)


def test_write_png_is_read_by_pil(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    img = np.random.default_rng(3).integers(0, 256, (80, 96, 3)).astype(np.uint8)
    name = str(tmp_path / "b.png")
    render.write_png(name, img)
    with Image.open(name) as im:
        assert im.mode == "RGB" and im.size == (96, 80)
        assert np.array_equal(np.asarray(im), img)
