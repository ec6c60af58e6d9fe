"""The rendering rule of include/pcgc.h (pcgc_render_*) in numpy, for the tests of csrc/render.hip.

Two statements of hidden-point removal: `zbuffer` takes the minimum key per pixel with np.minimum.at, as the kernel's
atomics do; `zbuffer_painter` paints the points in descending key order so that the last write to a pixel wins.  They
share the projection and nothing else.  `resolve` is the shading, `colormap` the table look-up in float32 operations,
`png_pixels` reads a png back with zlib alone."""
import struct
import zlib

import numpy as np

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def project(points, R, window):
    """-> (px, py, d, keep) per point, int64: the rule up to the clipping in depth (and of coordinates outside the contract)"""
    u0, v1, w1, scale, ox, oy = (int(v) for v in window)
    f = np.rint(np.asarray(points, np.float32).reshape(-1, 3) * np.float32(16.0))           # float32 product, half to even
    ok = np.all(np.abs(f) <= 524288.0, axis=1)                                              # false for a NaN
    q = np.where(ok[:, None], f, 0).astype(np.int64)
    t = (q @ np.asarray(R, np.int64).reshape(3, 3).T + 8192) >> 14
    px = (((t[:, 0] - u0) * scale) >> 16) + ox
    py = (((v1 - t[:, 1]) * scale) >> 16) + oy
    d = w1 - t[:, 2]
    return px, py, d, ok & (d >= 0) & (d < (1 << 31))


def _covered(px, py, d, keep, width, height, point_size):
    """-> (flat pixel index, key) of every (point, covered pixel) pair inside the image"""
    idx = np.nonzero(keep)[0]
    key = (d[idx].astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint64)
    h = point_size // 2
    pix, keys = [], []
    for dy in range(-h, h + 1):
        for dx in range(-h, h + 1):
            x, y = px[idx] + dx, py[idx] + dy
            inside = (x >= 0) & (x < width) & (y >= 0) & (y < height)
            pix.append((y * width + x)[inside])
            keys.append(key[inside])
    return np.concatenate(pix) if pix else np.zeros(0, np.int64), np.concatenate(keys) if keys else np.zeros(0, np.uint64)


def zbuffer(points, R, window, width, height, point_size):
    """uint64 [H,W]: per pixel the smallest key (d << 32 | index) of the points whose square covers it, all ones where none does"""
    assert point_size % 2 == 1 and 1 <= point_size <= 15
    pix, keys = _covered(*project(points, R, window), width, height, point_size)
    z = np.full(width * height, EMPTY, np.uint64)
    np.minimum.at(z, pix, keys)
    return z.reshape(height, width)


def zbuffer_painter(points, R, window, width, height, point_size):
    """the same image by painting: points from the farthest (and, at equal depth, the highest index) to the nearest, each
    overwriting its whole square"""
    px, py, d, keep = project(points, R, window)
    z = np.full((height, width), EMPTY, np.uint64)
    h = point_size // 2
    for i in sorted(np.nonzero(keep)[0].tolist(), key=lambda i: (int(d[i]), i), reverse=True):
        x0, x1 = max(int(px[i]) - h, 0), min(int(px[i]) + h, width - 1)
        y0, y1 = max(int(py[i]) - h, 0), min(int(py[i]) + h, height - 1)
        if x0 <= x1 and y0 <= y1:
            z[y0:y1 + 1, x0:x1 + 1] = np.uint64((int(d[i]) << 32) | i)
    return z


def resolve(z, colors=None, background=(255, 255, 255), foreground=(200, 200, 200), shade=0):
    """-> (rgb uint8 [H,W,3], index int32 [H,W], depth int32 [H,W])"""
    height, width = z.shape
    covered = z != EMPTY
    d = (z >> np.uint64(32)).astype(np.int64)
    i = (z & np.uint64(0xFFFFFFFF)).astype(np.int64)
    base = np.empty((height, width, 3), np.int64)
    base[:] = np.asarray(foreground, np.int64)
    if colors is not None and len(colors):
        base[covered] = np.asarray(colors, np.int64).reshape(-1, 3)[i[covered]]
    factor = np.full((height, width), 255, np.int64)
    if shade > 0:
        obs = np.zeros((height, width), np.int64)
        dp = np.pad(d, 1)
        cp = np.pad(covered, 1)                                # outside the image: not covered
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dy or dx:
                    dn = dp[1 + dy:1 + dy + height, 1 + dx:1 + dx + width]
                    cn = cp[1 + dy:1 + dy + height, 1 + dx:1 + dx + width]
                    obs += np.where(cn, np.maximum(d - dn, 0), 0)
        factor = (255 * shade) // (shade + obs)
    rgb = (base * factor[:, :, None] + 127) // 255
    rgb[~covered] = np.asarray(background, np.int64)
    return rgb.astype(np.uint8), np.where(covered, i, -1).astype(np.int32), np.where(covered, d, -1).astype(np.int32)


def render(points, colors, R, window, width, height, point_size, background=(255, 255, 255), foreground=(200, 200, 200), shade=0):
    return resolve(zbuffer(points, R, window, width, height, point_size), colors, background, foreground, shade)


def colormap(values, vmax, lut):
    """lut[min(255, floor(float32(v) * scale))] with scale = float32(256 / vmax), every operation in float32"""
    scale = np.float32(256.0 / float(vmax))
    f = np.floor(np.asarray(values, np.float32) * scale)
    return np.asarray(lut)[np.minimum(f, np.float32(255.0)).astype(np.int64)]


def png_chunks(data):
    """[(type, body)] of a png, with the signature and every chunk's CRC checked"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, out = 8, []
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        crc, = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(kind + body) & 0xFFFFFFFF, kind
        out.append((kind, body))
        pos += 12 + n
    assert pos == len(data)
    return out


def png_pixels(data):
    """the pixels of an 8-bit RGB png whose scanlines all have filter type 0, by zlib alone"""
    chunks = png_chunks(data)
    assert chunks[0][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    w, h, depth, colour, compression, filt, interlace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, compression, filt, interlace) == (8, 2, 0, 0, 0)
    raw = zlib.decompress(b"".join(body for kind, body in chunks if kind == b"IDAT"))
    lines = np.frombuffer(raw, np.uint8).reshape(h, 1 + 3 * w)
    assert not lines[:, 0].any()
    return lines[:, 1:].reshape(h, w, 3)
