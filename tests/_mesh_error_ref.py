"""The point-to-mesh rule in numpy (include/pcgc.h, pcgc_meshdist_*): the text of the header, one numpy
operation per written step (numpy neither contracts nor reorders), and brute force over every triangle.  The device
(csrc/meshdist.hip) and the host copy of csrc/point_triangle.h are held to this bit for bit."""
import math

import numpy as np


def sub(x, y):
    return x - y


def dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def cross(x, y):
    return np.stack([x[..., 1] * y[..., 2] - x[..., 2] * y[..., 1],
                     x[..., 2] * y[..., 0] - x[..., 0] * y[..., 2],
                     x[..., 0] * y[..., 1] - x[..., 1] * y[..., 0]], -1)


def vmin(x, y):
    return np.where(x < y, x, y)


def seg(p, u, v):
    """the squared distance from p to the segment u v; arrays [..., 3] that broadcast"""
    p, u, v = (np.asarray(x, np.float64) for x in (p, u, v))
    e, w = sub(v, u), sub(p, u)
    l, s = dot(e, e), dot(w, e)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(l > 0, s / l, 0.0)
    t = np.where(t < 0, 0.0, t)
    t = np.where(t > 1, 1.0, t)
    r = w - t[..., None] * e
    return dot(r, r)


def face(p, a, b, c):
    """-> (counts, value) of the face term"""
    p, a, b, c = (np.asarray(x, np.float64) for x in (p, a, b, c))
    n = cross(sub(b, a), sub(c, a))
    nn = dot(n, n)
    u, v, w = sub(a, p), sub(b, p), sub(c, p)
    n = np.broadcast_to(n, np.broadcast_shapes(n.shape, u.shape))
    counts = (nn > 0) & (dot(n, cross(u, v)) >= 0) & (dot(n, cross(v, w)) >= 0) & (dot(n, cross(w, u)) >= 0)
    dn = dot(n, sub(p, a))
    with np.errstate(divide="ignore", invalid="ignore"):
        value = dn * dn / nn
    return counts, value


def d2(p, a, b, c):
    """the rule: arrays [..., 3] that broadcast -> float64 [...]"""
    m = vmin(seg(p, a, b), seg(p, b, c))
    m = vmin(m, seg(p, c, a))
    counts, value = face(p, a, b, c)
    return np.where(counts & (value < m), value, m)


def brute(points, vertices, triangles, max_dist=None, rows=64):
    """-> (best float64 [N], nearest int32 [N]): every point against every triangle; the smallest index among equal minima; with
    a gate, best = +inf and nearest = -1 for a point with best > max_dist * max_dist"""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    a, b, c = v[t[:, 0]][None], v[t[:, 1]][None], v[t[:, 2]][None]
    best, nearest = np.empty(len(p)), np.empty(len(p), np.int32)
    for at in range(0, len(p), rows):
        d = d2(p[at:at + rows, None, :], a, b, c)
        k = np.argmin(d, 1)                                              # the first of equal minima
        best[at:at + rows], nearest[at:at + rows] = d[np.arange(len(k)), k], k
    if max_dist is not None:
        far = best > np.float64(max_dist) * np.float64(max_dist)
        best[far], nearest[far] = np.inf, -1
    return best, nearest


def figures(best):
    """-> (points, far, mse, max): the mean as the correctly rounded quotient of the exact sum (math.fsum)"""
    best = np.asarray(best, np.float64)
    near = best[np.isfinite(best)]
    if not len(near):
        return len(best), len(best), float("nan"), float("nan")
    return len(best), len(best) - len(near), math.fsum(near.tolist()) / len(near), float(near.max())


def pair_count(vertices, triangles, h):
    """the (cell, triangle) pairs of cells of edge h: every triangle in each cell its axis-aligned bounding box overlaps"""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    corners = v[t]                                                        # [T, 3 corners, 3]
    lo, hi = np.floor(corners.min(1) / h), np.floor(corners.max(1) / h)
    return int(np.prod(hi - lo + 1, 1).sum())


def bounds(vertices, triangles):
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    corners = v[np.asarray(triangles, np.int64).reshape(-1)]
    return corners.min(0), corners.max(0)
