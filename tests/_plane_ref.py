"""The plane rule (include/pcgc.h, pcgc_plane_count and pcgc_plane_select; pcgcv1_amd/clean.py) in numpy: seeded
draws, exact integer scoring, the least-squares refit, the decision and the filter's mask, and the refit of the frame on top of
tests/_clean_ref.py.  Also the scene: a tilted table with a sphere resting on it.  Not collected by pytest."""
import math

import numpy as np

import _clean_ref as clean_ref
import _components_ref as components_ref

DEFAULT_FRAC, DEFAULT_DRAWS, DEFAULT_SEED = 0.05, 1024, 0


def threshold(D2, nn):
    """T with |s| <= T exactly 2 |s| <= D2 sqrt(nn), in Python integers"""
    return math.isqrt(D2 * D2 * int(nn)) // 2


def draw_planes(points, D2, draws, seed):
    """step 1 -> int64 [draws,5]: (a, b, c, d, T) per draw, T = -1 for a repeated or collinear triple"""
    p = np.asarray(points, np.int64).reshape(-1, 3)
    tri = np.random.default_rng(seed).integers(0, len(p), (draws, 3))
    planes = np.empty((draws, 5), np.int64)
    for h, (i0, i1, i2) in enumerate(tri):
        u, v = p[i1] - p[i0], p[i2] - p[i0]
        a, b, c = (int(u[1] * v[2] - u[2] * v[1]), int(u[2] * v[0] - u[0] * v[2]), int(u[0] * v[1] - u[1] * v[0]))
        nn = a * a + b * b + c * c
        planes[h] = (a, b, c, a * int(p[i0][0]) + b * int(p[i0][1]) + c * int(p[i0][2]), threshold(D2, nn) if nn else -1)
    return planes


def inliers(points, bits, plane):
    """-> bool [n]: |a x + b y + c z - d| <= T in int64, never for a point outside the grid"""
    p = np.asarray(points, np.int64).reshape(-1, 3)
    a, b, c, d, T = [np.int64(v) for v in plane]
    s = a * p[:, 0] + b * p[:, 1] + c * p[:, 2] - d
    return (np.abs(s) <= T) & ((p >= 0) & (p < (1 << bits))).all(1)


def counts(points, bits, planes, rows=32):
    """step 2's scores -> int32 [K], a few planes at a time against all the points"""
    p = np.asarray(points, np.int64).reshape(-1, 3)
    planes = np.asarray(planes, np.int64).reshape(-1, 5)
    inside = ((p >= 0) & (p < (1 << bits))).all(1)
    out = np.zeros(len(planes), np.int32)
    for h in range(0, len(planes), rows):
        q = planes[h:h + rows]
        s = p @ q[:, :3].T - q[:, 3]
        out[h:h + rows] = ((np.abs(s) <= q[:, 4]) & inside[:, None]).sum(0)
    return out


def sums(points, mask):
    """the ten int64 sums over the rows of the mask: N, x, y, z, x^2, y^2, z^2, xy, xz, yz"""
    p = np.asarray(points, np.int64).reshape(-1, 3)[np.asarray(mask, bool)]
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.array([len(p), x.sum(), y.sum(), z.sum(), (x * x).sum(), (y * y).sum(), (z * z).sum(), (x * y).sum(), (x * z).sum(),
                     (y * z).sum()], np.int64)


def refit(ten, D2):
    """step 3 on the host -> (plane int64 [5], nq: the normal as three Python integers)"""
    N, sx, sy, sz, xx, yy, zz, xy, xz, yz = [int(v) for v in ten]
    mu = np.array([sx, sy, sz], np.float64) / N
    cov = np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]], np.float64) / N - np.outer(mu, mu)
    w, vec = np.linalg.eigh(cov)
    nq = [int(c) for c in np.rint(65536.0 * vec[:, int(np.argmin(w))]).astype(np.int64)]
    nn = N * N * sum(c * c for c in nq)
    return np.array([N * nq[0], N * nq[1], N * nq[2], nq[0] * sx + nq[1] * sy + nq[2] * sz, threshold(D2, nn)], np.int64), nq


def segment(points, bits, D2, frac=DEFAULT_FRAC, draws=DEFAULT_DRAWS, seed=DEFAULT_SEED):
    """steps 1 to 4 -> (plane int64 [5] | None, its inliers bool [n], info as clean.segment_plane's)"""
    p = np.asarray(points, np.int64).reshape(-1, 3)
    planes = draw_planes(p, D2, draws, seed)
    score = counts(p, bits, planes)
    best = int(np.argmax(score))
    info = dict(n=len(p), draws=draws, best_count=int(score[best]), count=0, dropped=False)
    if score[best] == 0:
        return None, np.zeros(len(p), bool), info
    plane, mask = planes[best], inliers(p, bits, planes[best])
    again = refit(sums(p, mask), D2)[0]
    again_mask = inliers(p, bits, again)
    if again_mask.sum() >= mask.sum():
        plane, mask = again, again_mask
    info["count"] = int(mask.sum())
    info["dropped"] = bool(info["count"] >= frac * len(p))
    return plane, mask, info


def parse_spec(text):
    f = text.split(":")
    if f[0] != "plane":
        return components_ref.parse_spec(text)
    D2 = 2 * float(f[1])
    assert D2 == int(D2)
    return ("plane", int(D2), float(f[2]) if len(f) > 2 else DEFAULT_FRAC, int(f[3]) if len(f) > 3 else DEFAULT_DRAWS,
            int(f[4]) if len(f) > 4 else DEFAULT_SEED)


def largest_mask(points, bits):
    """`largest` at G = 1 on a cloud too large for _components_ref's all pairs: scipy's 26-connected labels on the dense grid.
    They are numbered in raster order, which is key order, so the first of the largest is the one with the smallest label."""
    from scipy import ndimage
    p = np.asarray(points, np.int64).reshape(-1, 3)
    grid = np.zeros((1 << bits,) * 3, bool)
    grid[p[:, 0], p[:, 1], p[:, 2]] = True
    label = ndimage.label(grid, structure=np.ones((3, 3, 3)))[0][p[:, 0], p[:, 1], p[:, 2]]
    return label == np.argmax(np.bincount(label))


def keep_mask(points, bits, spec):
    kind = parse_spec(spec)
    if kind == ("largest", 1):
        return largest_mask(points, bits)
    if kind[0] != "plane":
        return components_ref.keep_mask(points, bits, spec)
    _, mask, info = segment(points, bits, *kind[1:])
    return ~mask if info["dropped"] else np.ones(len(mask), bool)


def keep_mask_all(points, bits, specs):
    """the filters in order, each on what the one before kept -> bool [n]"""
    points = np.asarray(points)
    alive = np.arange(len(points))
    for spec in specs:
        alive = alive[keep_mask(points[alive], bits, spec)]
    mask = np.zeros(len(points), bool)
    mask[alive] = True
    return mask


def voxelize_scan_clean(points, colors=None, normals=None, bits=None, voxel_size=None, clean=()):
    """_clean_ref.voxelize_scan_clean with the plane filter among the specs: the same refit around this module's masks.  No
    mask depends on the grid as long as it holds every voxel, so the bits of the largest coordinate serve."""
    saved = clean_ref.keep_mask_all
    clean_ref.keep_mask_all = lambda vox, specs: keep_mask_all(vox, max(1, int(np.max(vox)).bit_length()), specs)
    try:
        return clean_ref.voxelize_scan_clean(points, colors, normals, bits, voxel_size, clean)
    finally:
        clean_ref.keep_mask_all = saved


SCENE_VOXELS, SCENE_TABLE = 41014, 27247


def scene_samples(bits=7, seed=0):
    """-> (samples float64 [260000,3] in cells, is_table bool): a square table over the middle 0.8 of the grid in x and y, tilted by
    the slopes 0.13 and -0.21 about the height 0.3 res at its centre, 200 000 samples; a sphere shell of radius 0.18 res whose lowest
    point rests on the table's centre, 60 000 samples; Gaussian noise of 0.4 cell on every coordinate"""
    res = 1 << bits
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0.1 * res, 0.9 * res, (200000, 2))
    table = np.c_[xy, 0.3 * res + 0.13 * (xy[:, 0] - res / 2) - 0.21 * (xy[:, 1] - res / 2)]
    d = rng.normal(size=(60000, 3))
    shell = np.array([res / 2, res / 2, 0.3 * res + 0.18 * res]) + 0.18 * res * d / np.linalg.norm(d, axis=1, keepdims=True)
    p = np.r_[table, shell]
    return p + rng.normal(0, 0.4, p.shape), np.r_[np.ones(len(table), bool), np.zeros(len(shell), bool)]


def scene(bits=7, seed=0):
    """the samples floored to voxels, clipped to the grid, made unique -> (voxels int32 [n,3] in np.unique's order, is_table bool
    [n]: the voxel holds a table sample).  bits = 7, seed = 0: SCENE_VOXELS voxels, SCENE_TABLE of them table"""
    res = 1 << bits
    p, from_table = scene_samples(bits, seed)
    v = np.clip(np.floor(p), 0, res - 1).astype(np.int32)
    vox, inverse = np.unique(v, axis=0, return_inverse=True)
    is_table = np.zeros(len(vox), bool)
    is_table[np.asarray(inverse).reshape(-1)[from_table]] = True
    return vox, is_table
