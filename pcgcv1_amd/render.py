"""Point clouds and per-point error maps as images, on the GPU (csrc/render.hip; include/pcgc.h, pcgc_render_*).

The reference looks at its clouds with o3d.visualization.draw_geometries (demo.ipynb:586,596,962,972) and shows decoded
clouds coloured by their error (figs/redandblack.png, figs/phil.png); a headless MI355X node has neither Open3D nor a
display.  Here: an orthographic projection, hidden points removed by a z-buffer of 64-bit atomic minima, eye-dome lighting
on the depth image, and a png written with zlib alone.  Everything after one rounding of the coordinates is integer
arithmetic (DESIGN.md "Rendering"), so an image is defined bit for bit; tests/_render_ref.py is the same rule in numpy.

    python -m pcgcv1_amd.render --input X_rec.ply --output X.png [--compare ORIGINAL.ply] [--view front] [--yaw D --pitch D]
                                [--up y|z] [--size W H] [--point_size P] [--error_max V] [--no_shade]

There is no host fallback: without a GPU every entry point that draws raises, like the rest of the package.
"""
import argparse
import collections
import struct
import zlib

import numpy as np

from . import _lib

Q = 14                            # fraction bits of the view matrix
SUB = 16                          # coordinates are quantised to 1 / SUB voxel
DEFAULT_K = 256                   # eye-dome strength: a summed depth step of 16 voxels halves a pixel (DESIGN.md "Rendering")
MAX_SIDE = 8192
MAX_POINT_SIZE = 15
VIEWS = ("front", "back", "left", "right", "top", "bottom")

# rows right, up, toward the viewer of the named views for up = "y"; right x up = toward the viewer in each
_VIEW_ROWS = {
    "front": ((1, 0, 0), (0, 1, 0), (0, 0, 1)),
    "back": ((-1, 0, 0), (0, 1, 0), (0, 0, -1)),
    "right": ((0, 0, -1), (0, 1, 0), (1, 0, 0)),
    "left": ((0, 0, 1), (0, 1, 0), (-1, 0, 0)),
    "top": ((1, 0, 0), (0, 0, -1), (0, 1, 0)),
    "bottom": ((1, 0, 0), (0, 0, 1), (0, -1, 0)),
}
# up = "z" (ModelNet, lidar): the cloud's z takes the place of y and its -y the place of z first
_UP = {"y": ((1, 0, 0), (0, 1, 0), (0, 0, 1)), "z": ((1, 0, 0), (0, 0, 1), (0, -1, 0))}

Window = collections.namedtuple("Window", "u0 v1 w1 scale ox oy")
Window.__doc__ = """where the projected cloud lands: px = (((t0 - u0) * scale) >> 16) + ox, py = (((v1 - t1) * scale) >> 16) + oy,
d = w1 - t2, with t in 1/16 voxel and scale = pixels per 1/16 voxel in Q16"""


def view_matrix(view="front", yaw=0.0, pitch=0.0, up="y"):
    """-> int64 [3,3], Q14: rows right, up, toward the viewer.  up="y": front is the identity (right = +x, up = +y, toward the
    viewer = +z); back, left, right, top and bottom are its quarter turns (the camera on that side of the cloud).  yaw turns
    the camera about the up axis (90 from front = right), pitch raises it about the right axis (90 from front = top), in
    degrees.  up="z" permutes the axes first.  np.rint(R * 16384) of the float64 rotation; the kernel sees the integers only."""
    if view not in _VIEW_ROWS:
        raise ValueError("view_matrix: view must be one of %s (got %r)" % (", ".join(VIEWS), view))
    if up not in _UP:
        raise ValueError("view_matrix: up must be 'y' or 'z' (got %r)" % (up,))
    cy, sy = np.cos(np.deg2rad(float(yaw))), np.sin(np.deg2rad(float(yaw)))
    cp, sp = np.cos(np.deg2rad(float(pitch))), np.sin(np.deg2rad(float(pitch)))
    turn = np.array([[cy, 0.0, -sy], [0.0, 1.0, 0.0], [sy, 0.0, cy]])
    rise = np.array([[1.0, 0.0, 0.0], [0.0, cp, -sp], [0.0, sp, cp]])
    r = rise @ turn @ np.array(_VIEW_ROWS[view], np.float64) @ np.array(_UP[up], np.float64)
    return np.rint(r * (1 << Q)).astype(np.int64)


def _as_matrix(view):
    if isinstance(view, str):
        return view_matrix(view)
    r = np.asarray(view)
    if r.shape != (3, 3) or not np.issubdtype(r.dtype, np.integer) or int(np.abs(r).max()) > (1 << Q):
        raise ValueError("render: view must be a name (%s) or an integer [3,3] matrix in Q14 (view_matrix)" % ", ".join(VIEWS))
    return r.astype(np.int64)


def _float32_points(points):
    p = np.ascontiguousarray(np.asarray(points), np.float32).reshape(-1, 3)
    if p.size and not (np.abs(p).max() < 32768.0):             # false for a NaN as well
        raise ValueError("render: coordinates must be finite and below 2^15 in magnitude")
    return p


def project(points, R):
    """-> int64 [N,3]: t = (R q + 8192) >> 14 of q = rint(float32(p) * 16), the kernel's rule on the host (fit_window)"""
    q = np.rint(_float32_points(points) * np.float32(SUB)).astype(np.int64)
    return (q @ np.asarray(R, np.int64).T + (1 << (Q - 1))) >> Q


def _extent(cloud, R):
    """-> (lowest, highest) projected coordinates of a cloud, int64 [3] each, or None for an empty one.  A float32 device
    tensor is projected where it lies: R q in float64, exact because |R q| < 2^36, and the shift on the two extremes
    (it is monotone); anything else goes through project on the host."""
    if hasattr(cloud, "is_cuda"):
        import torch
        if cloud.shape[0] == 0:
            return None
        t = torch.round(cloud.reshape(-1, 3).to(torch.float32) * float(SUB)).to(torch.float64) @ torch.from_numpy(
            np.asarray(R, np.float64).T.copy()).to(cloud.device)
        ends = torch.stack([t.amin(0), t.amax(0)]).cpu().numpy().astype(np.int64)
        return (ends[0] + (1 << (Q - 1))) >> Q, (ends[1] + (1 << (Q - 1))) >> Q
    t = project(cloud, R)
    return (t.min(0), t.max(0)) if len(t) else None


def fit_window(clouds, R, width, height, margin=8):
    """The window that centres the union of the clouds' projections under R and fits it into width x height with `margin`
    pixels free on the tighter side: scale = ((min(width, height) - 2 margin) << 16) // (extent + 1) with extent the larger
    of the projected width and height in 1/16 voxel.  Integer arithmetic on the projected extents; share one window among
    the panels of a figure.  `clouds` is one [N,3] array or a list of them (numpy, or float32 device tensors)."""
    if hasattr(clouds, "shape") and len(clouds.shape) == 2:
        clouds = [clouds]
    side = min(int(width), int(height)) - 2 * int(margin)
    if side < 1:
        raise ValueError("fit_window: a margin of %d leaves nothing of a %d x %d image" % (margin, width, height))
    ends = [e for e in (_extent(c, R) for c in clouds) if e is not None]
    if not ends:
        return Window(0, 0, 0, 1 << 16, 0, 0)
    lo = np.min([e[0] for e in ends], axis=0)
    hi = np.max([e[1] for e in ends], axis=0)
    du, dv = int(hi[0] - lo[0]), int(hi[1] - lo[1])
    scale = min(max((side << 16) // (max(du, dv) + 1), 1), 1 << 30)
    ox = (int(width) - 1 - ((du * scale) >> 16)) // 2
    oy = (int(height) - 1 - ((dv * scale) >> 16)) // 2
    return Window(int(lo[0]), int(hi[1]), int(hi[2]), scale, ox, oy)


def default_point_size(window):
    """the smallest odd number not below sqrt(3) x pixels per voxel (a voxel's diagonal: surfaces stay closed in oblique
    views), within 1..15; pixels per voxel = scale * 16 / 2^16, compared in integers"""
    for p in range(1, MAX_POINT_SIZE, 2):
        if p * p * (1 << 24) >= 3 * window.scale * window.scale:
            return p
    return MAX_POINT_SIZE


def _rgb24(color, what):
    c = [int(v) for v in color]
    if len(c) != 3 or min(c) < 0 or max(c) > 255:
        raise ValueError("render: %s must be three values within 0..255 (got %r)" % (what, color))
    return (c[0] << 16) | (c[1] << 8) | c[2]


def splat(points_d, R, window, width, height, point_size, workspace=None):
    """pcgc_render_splat on a float32 [N,3] device tensor -> the z-buffer (a uint8 device tensor of
    pcgc_render_workspace_bytes), for resolve"""
    import torch
    lib = _lib.hip()
    nbytes = int(lib.pcgc_render_workspace_bytes(int(width), int(height)))
    if nbytes == 0:
        raise ValueError("render: width and height must lie within 1..%d (got %d x %d)" % (MAX_SIDE, width, height))
    if workspace is None:
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=points_d.device)
    rot = np.ascontiguousarray(np.asarray(R).reshape(9), np.int32)
    w = Window(*window)
    _lib.check(lib.pcgc_render_splat(_lib.dptr(points_d) if points_d.shape[0] else None, points_d.shape[0], _lib.nptr(rot), int(w.u0),
                                     int(w.v1), int(w.w1), int(w.scale), int(w.ox), int(w.oy), int(width), int(height), int(point_size),
                                     _lib.dptr(workspace), workspace.numel(), _lib.stream()), "pcgc_render_splat")
    return workspace


def resolve(workspace, width, height, colors_d=None, background=(255, 255, 255), foreground=(200, 200, 200), shade=DEFAULT_K, out=None,
            buffers=True):
    """pcgc_render_resolve of a z-buffer -> (rgb uint8 [H,W,3], index int32 [H,W] or None, depth int32 [H,W] or None), device
    tensors.  out = (rgb, index, depth): write into these contiguous tensors instead (index and depth may be None)."""
    import torch
    dev = workspace.device
    if out is None:
        out = (torch.empty((height, width, 3), dtype=torch.uint8, device=dev),
               torch.empty((height, width), dtype=torch.int32, device=dev) if buffers else None,
               torch.empty((height, width), dtype=torch.int32, device=dev) if buffers else None)
    rgb, index, depth = out
    for t, shape, dtype in ((rgb, (height, width, 3), torch.uint8), (index, (height, width), torch.int32), (depth, (height, width), torch.int32)):
        if t is not None and (tuple(t.shape) != shape or t.dtype != dtype):
            raise ValueError("render: an output tensor of shape %s / %s where %s / %s belongs" % (tuple(t.shape), t.dtype, shape, dtype))
    n = 0 if colors_d is None else int(colors_d.shape[0])
    _lib.check(_lib.hip().pcgc_render_resolve(_lib.dptr(workspace), workspace.numel(), int(width), int(height), _lib.dptr(colors_d), n,
                                              _rgb24(background, "background"), _rgb24(foreground, "foreground"), int(shade),
                                              _lib.dptr(rgb), _lib.dptr(index), _lib.dptr(depth), _lib.stream()), "pcgc_render_resolve")
    return rgb, index, depth


def render(points, colors=None, *, size=(1024, 1024), view="front", window=None, point_size=None, background=(255, 255, 255),
           foreground=(200, 200, 200), shade=DEFAULT_K, return_buffers=False):
    """points [N,3] (any float32-representable coordinates below 2^15, N may be 0), colors uint8 [N,3] or None -> the image,
    uint8 [H,W,3] (numpy), size = (W, H).  view: a name or a view_matrix; window: a fit_window (None: fitted to this cloud);
    point_size: odd, 1..15 (None: default_point_size); shade: eye-dome strength, 0 = off.  colors=None draws every point
    in `foreground`.  return_buffers=True: -> (rgb, index int32 [H,W] = the point each pixel shows, -1 for background,
    depth int32 [H,W] = its distance from the window's front in 1/16 voxel, -1 for background)."""
    import torch
    dev = _lib.require_gpu()
    width, height = int(size[0]), int(size[1])
    R = _as_matrix(view)
    p = _float32_points(points)
    p_d = torch.from_numpy(p).to(dev)
    if window is None:
        window = fit_window([p_d], R, width, height)
    if point_size is None:
        point_size = default_point_size(Window(*window))
    colors_d = None
    if colors is not None:
        c = np.ascontiguousarray(colors, np.uint8).reshape(-1, 3)
        if len(c) != len(p):
            raise ValueError("render: %d points, %d colours" % (len(p), len(c)))
        colors_d = torch.from_numpy(c).to(dev) if len(c) else None
    zbuf = splat(p_d, R, window, width, height, point_size)
    rgb, index, depth = resolve(zbuf, width, height, colors_d, background, foreground, shade, buffers=return_buffers)
    if return_buffers:
        return rgb.cpu().numpy(), index.cpu().numpy(), depth.cpu().numpy()
    return rgb.cpu().numpy()


_ANCHORS = ((0, (0, 0, 255)), (64, (0, 255, 255)), (128, (0, 255, 0)), (192, (255, 255, 0)), (255, (255, 0, 0)))


def colormap_lut():
    """-> uint8 [256,3]: blue, cyan, green, yellow, red at entries 0, 64, 128, 192, 255, between them integer linear
    interpolation rounded half up"""
    lut = np.zeros((256, 3), np.uint8)
    for (i0, c0), (i1, c1) in zip(_ANCHORS[:-1], _ANCHORS[1:]):
        span = i1 - i0
        for i in range(i0, i1 + 1):
            lut[i] = [(2 * (a * (i1 - i) + b * (i - i0)) + span) // (2 * span) for a, b in zip(c0, c1)]
    return lut


def error_colors(values, vmax):
    """per-point figures (finite, >= 0) -> uint8 [N,3] through pcgc_colormap: entry min(255, floor(float32(v) * scale)) of
    colormap_lut with scale = float32(256 / vmax); vmax and beyond are red"""
    import torch
    dev = _lib.require_gpu()
    v = np.ascontiguousarray(values, np.float32).reshape(-1)
    if not (float(vmax) > 0):
        raise ValueError("error_colors: vmax must be positive (got %r)" % (vmax,))
    if v.size and not (np.isfinite(v).all() and v.min() >= 0):
        raise ValueError("error_colors: values must be finite and not negative")
    out = torch.empty((len(v), 3), dtype=torch.uint8, device=dev)
    if len(v):
        v_d, lut_d = torch.from_numpy(v).to(dev), torch.from_numpy(colormap_lut()).to(dev)       # named: both live until the launch
        _lib.check(_lib.hip().pcgc_colormap(_lib.dptr(v_d), len(v), float(np.float32(256.0 / float(vmax))), _lib.dptr(lut_d),
                                            _lib.dptr(out), _lib.stream()), "pcgc_colormap")
    return out.cpu().numpy()


def compare(original, decoded, decoded_colors=None, *, size=(1024, 1024), view="front", vmax=4.0, point_size=None,
            background=(255, 255, 255), foreground=(200, 200, 200), shade=DEFAULT_K, resolution=1023, return_metrics=False):
    """Three panels of `size` side by side -> uint8 [H, 3 W, 3], in one window and view:
      the original coloured by each point's distance to the decoded cloud (what the codec lost),
      the decoded cloud coloured by each point's distance to the original (what it invented),
      the decoded cloud in its own colours (decoded_colors uint8 [N,3]), or shaded `foreground` without them.
    Distances are metrics.pc_error_float's per-point figures (square roots taken here), in voxels; vmax and beyond are red.
    The decoded cloud is drawn as pc_error_float measures it: without duplicate points, in np.unique's order.
    return_metrics=True: -> (image, the dict of D1 figures)."""
    from .metrics import pc_error_float
    a = _float32_points(original)
    b, first = np.unique(_float32_points(decoded), axis=0, return_index=True)
    figures, detail = pc_error_float(a, b, None, resolution, per_point=True)
    width, height = int(size[0]), int(size[1])
    R = _as_matrix(view)
    window = fit_window([a, b], R, width, height)
    if point_size is None:
        point_size = default_point_size(window)
    own = None
    if decoded_colors is not None:
        own = np.ascontiguousarray(decoded_colors, np.uint8).reshape(-1, 3)
        if len(own) != len(np.asarray(decoded).reshape(-1, 3)):
            raise ValueError("compare: %d decoded points, %d colours" % (len(np.asarray(decoded).reshape(-1, 3)), len(own)))
        own = own[first]
    common = dict(size=(width, height), view=R, window=window, point_size=point_size, background=background, foreground=foreground,
                  shade=shade)
    panels = [render(a, error_colors(np.sqrt(detail["1"][0]), vmax), **common),
              render(b, error_colors(np.sqrt(detail["2"][0]), vmax), **common),
              render(b, own, **common)]
    image = np.concatenate(panels, axis=1)
    return (image, figures) if return_metrics else image


def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def png_bytes(rgb):
    """uint8 [H,W,3] -> an 8-bit RGB png: every scanline with filter type 0, one IDAT chunk"""
    a = np.asarray(rgb)
    if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("write_png: an image is uint8 [H,W,3] with H, W >= 1 (got %s %s)" % (a.dtype, a.shape))
    h, w = a.shape[:2]
    lines = np.zeros((h, 1 + 3 * w), np.uint8)                # the leading 0 of a line = filter type none
    lines[:, 1:] = a.reshape(h, 3 * w)
    return (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) +
            _chunk(b"IDAT", zlib.compress(lines.tobytes(), 6)) + _chunk(b"IEND", b""))


def write_png(filename, rgb):
    data = png_bytes(rgb)
    with open(filename, "wb") as f:
        f.write(data)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="render a point cloud (.ply) to a png on the GPU",
                                 formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    ap.add_argument("--input", required=True, help="the cloud to draw (.ply, with or without colours; fractions are kept)")
    ap.add_argument("--output", required=True, help="the png to write")
    ap.add_argument("--compare", default="", metavar="ORIGINAL.ply",
                    help="draw three panels instead: the original and --input coloured by their distance to each other, and --input itself")
    ap.add_argument("--view", default="front", choices=VIEWS)
    ap.add_argument("--yaw", type=float, default=0.0, help="degrees about the up axis, from --view")
    ap.add_argument("--pitch", type=float, default=0.0, help="degrees about the right axis, from --view")
    ap.add_argument("--up", default="y", choices=("y", "z"))
    ap.add_argument("--size", type=int, nargs=2, default=(1024, 1024), metavar=("W", "H"), help="pixels (of each panel)")
    ap.add_argument("--point_size", type=int, default=0, help="odd, 1..15; 0 = from the scale: sqrt(3) x pixels per voxel")
    ap.add_argument("--error_max", type=float, default=4.0, help="--compare: the distance in voxels that is drawn red")
    ap.add_argument("--no_shade", action="store_true", help="no eye-dome lighting")
    return ap.parse_args(argv)


def main(argv=None):
    from .dataprocess.inout_points import load_ply_colors
    args = parse_args(argv)
    points, colors = load_ply_colors(args.input, as_float=True)
    common = dict(size=tuple(args.size), view=view_matrix(args.view, args.yaw, args.pitch, args.up), point_size=args.point_size or None,
                  shade=0 if args.no_shade else DEFAULT_K)
    if args.compare:
        original, _ = load_ply_colors(args.compare, as_float=True)
        image, figures = compare(original, points, colors, vmax=args.error_max, return_metrics=True, **common)
        for key in sorted(figures):
            print("{}: {:.6g}".format(key, figures[key]))
    else:
        image = render(points, colors, **common)
    write_png(args.output, image)
    print("{}: {} x {} png of {} points".format(args.output, image.shape[1], image.shape[0], len(points)))


if __name__ == "__main__":
    main()
