"""The cleaning rule (include/pcgc.h, pcgc_clean_neighbors; pcgcv1_amd/clean.py) in numpy: brute-force integer
distances between all pairs, isqrt16 through math.isqrt, the two filters, and the refit of the frame on top of
tests/_ingest_ref.py.  Not collected by pytest."""
import math

import numpy as np

import _ingest_ref as ingest_ref

DEFAULT_RADIUS = 8


def isqrt16(d2):
    return math.isqrt(int(d2) << 32)


def neighbor_statistics(points, k, radius, rows=256):
    """points int [n,3], distinct -> (S int64 [n], cnt int32 [n]).  A few rows at a time against all the others."""
    p = np.asarray(points, np.int64).reshape(-1, 3)
    n, r2 = len(p), radius * radius
    table = np.array([isqrt16(d) for d in range(r2 + 1)], np.int64)
    far = np.int64((radius + 1) << 16)
    S, cnt = np.zeros(n, np.int64), np.zeros(n, np.int32)
    for a in range(0, n, rows):
        d2 = ((p[a:a + rows, None, :] - p[None, :, :]) ** 2).sum(-1)
        d2[np.arange(len(d2)), np.arange(a, a + len(d2))] = r2 + 1                # not its own neighbour
        inside = d2 <= r2
        cnt[a:a + rows] = inside.sum(1)
        if k:
            nearest = np.sort(np.where(inside, d2, r2 + 1), axis=1)[:, :k]        # fewer than k columns when n <= k
            terms = np.where(nearest <= r2, table[np.minimum(nearest, r2)], far)
            S[a:a + rows] = terms.sum(1) + (k - nearest.shape[1]) * far
    return S, cnt


def parse_spec(text):
    f = text.split(":")
    if f[0] == "radius":
        return ("radius", int(f[1]), int(f[2]))
    return ("stat", int(f[1]), float(f[2]), int(f[3]) if len(f) > 3 else DEFAULT_RADIUS)


def keep_mask(points, spec):
    spec = parse_spec(spec)
    if spec[0] == "radius":
        return neighbor_statistics(points, 0, spec[1])[1] >= spec[2]
    S = neighbor_statistics(points, spec[1], spec[3])[0]
    return S <= np.mean(S) + spec[2] * np.std(S)


def keep_mask_all(points, specs):
    """the filters in order, each on what the one before kept -> bool [n]"""
    points = np.asarray(points)
    alive = np.arange(len(points))
    for spec in specs:
        alive = alive[keep_mask(points[alive], spec)]
    mask = np.zeros(len(points), bool)
    mask[alive] = True
    return mask


def voxelize_scan_clean(points, colors=None, normals=None, bits=None, voxel_size=None, clean=()):
    """-> (points, colors, normals, counts, (origin, step, bits), n_dropped, n_removed_voxels, n_removed_points, pass 1's kept
    voxels, pass 1's frame, the mask of the input rows that were kept): fit, quantise, merge, filter; drop the rows of the
    removed voxels; fit again on the kept rows, quantise and merge again.  No second cleaning pass."""
    points = np.asarray(points, np.float64)
    frame1 = ingest_ref.fit_frame(points, bits, voxel_size)
    n_dropped = ingest_ref.bounds(points)[2]
    _, keys = ingest_ref.quantize(points, *frame1)
    vox = ingest_ref.merge(keys, frame1[2])[0]
    keep = keep_mask_all(vox, clean)
    res = 2 ** frame1[2]
    vox_keys = (vox[:, 0].astype(np.int64) * res + vox[:, 1]) * res + vox[:, 2]
    row_keep = np.isin(keys, vox_keys[keep])                               # a dropped row's key is -1: in no voxel
    kept = points[row_keep]
    frame2 = ingest_ref.fit_frame(kept, bits, voxel_size)
    _, keys2 = ingest_ref.quantize(kept, *frame2)
    pts, counts, c, nrm = ingest_ref.merge(keys2, frame2[2], None if colors is None else np.asarray(colors)[row_keep],
                                           None if normals is None else np.asarray(normals)[row_keep])
    return (pts, c, nrm, counts, frame2, n_dropped, int((~keep).sum()), int(len(points) - n_dropped - row_keep.sum()), vox[keep],
            frame1, row_keep)
