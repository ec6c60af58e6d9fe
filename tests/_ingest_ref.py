"""The ingest rule (include/pcgc.h, pcgc_ingest_*; pcgcv1_amd/ingest.py) in numpy: frame fitting, quantisation,
the merge of the points of one voxel (count, exact colour mean, normalised integer normal sum) and the inverse map.  All
position arithmetic is float64, one numpy operation per step in the stated order.  Not collected by pytest."""
import numpy as np

MAX_BITS = 12
ONE = 2.0 ** 30          # fixed point of the normal sums


def finite_rows(points):
    return np.isfinite(np.asarray(points, np.float64)).all(1)


def bounds(points):
    """-> (min float64 [3], max float64 [3], n_dropped) over the rows without a non-finite coordinate"""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    keep = finite_rows(p)
    if not keep.any():
        raise ValueError("no row with three finite coordinates")
    return p[keep].min(0), p[keep].max(0), int((~keep).sum())


def fit_frame(points, bits=None, voxel_size=None):
    """-> (origin float64 [3], step, bits).  + 0.0 turns a -0.0 minimum into +0.0 (min does not order the two zeros)"""
    if (bits is None) == (voxel_size is None):
        raise ValueError("give bits or voxel_size, one of them")
    lo, hi, _ = bounds(points)
    if bits is not None:
        if not 1 <= bits <= MAX_BITS:
            raise ValueError("bits outside 1..12")
        ext = float((hi - lo).max())
        return lo + 0.0, (ext / (2 ** bits - 1) if ext != 0 else 1.0), int(bits)
    s = float(voxel_size)
    if not (np.isfinite(s) and s > 0):
        raise ValueError("voxel_size must be positive")
    origin = np.floor(lo / s) * s + 0.0
    qmax = float(np.floor((hi - origin) / s + 0.5).max())       # quantisation is monotone: the largest coordinate of all
    if not qmax < 2 ** MAX_BITS:
        raise ValueError("extent %r at voxel size %r needs more than 12 bits" % (float((hi - lo).max()), s))
    return origin, s, max(1, int(qmax).bit_length())


def quantize(points, origin, step, bits):
    """-> (q int32 [n,3], keys int64 [n]); a row with a non-finite coordinate has q = -1 and key -1"""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    keep = finite_rows(p)
    R, res = 2 ** bits - 1, 2 ** bits
    with np.errstate(invalid="ignore", over="ignore"):
        t = p - np.asarray(origin, np.float64)
        t = t / np.float64(step)
        t = t + 0.5
        t = np.floor(t)
    q = np.where(keep[:, None], np.clip(np.where(keep[:, None], t, 0.0), 0, R), -1).astype(np.int32)
    keys = np.where(keep, (q[:, 0].astype(np.int64) * res + q[:, 1]) * res + q[:, 2], -1)
    return q, keys


def merge(keys, bits, colors=None, normals=None):
    """-> (points int32 [m,3], counts int32 [m], colors uint8 [m,3] | None, normals float32 [m,3] | None), rows in ascending key;
    a key outside [0, res^3) contributes nothing"""
    keys = np.asarray(keys, np.int64)
    res = 2 ** bits
    ok = (keys >= 0) & (keys < res ** 3)
    uk, inv = np.unique(keys[ok], return_inverse=True)
    inv = inv.reshape(-1)
    m = len(uk)
    pts = np.stack([uk // (res * res), (uk // res) % res, uk % res], -1).astype(np.int32)
    counts = np.zeros(m, np.int64)
    np.add.at(counts, inv, 1)
    out_c = out_n = None
    if colors is not None:
        sums = np.zeros((m, 3), np.int64)
        np.add.at(sums, inv, np.asarray(colors, np.uint8)[ok].astype(np.int64))
        out_c = ((2 * sums + counts[:, None]) // (2 * counts[:, None])).astype(np.uint8)
    if normals is not None:
        c = np.asarray(normals, np.float32)[ok].astype(np.float64)
        c = np.where(np.isfinite(c), c, 0.0)
        c = np.clip(c, -1.0, 1.0)
        fixed = np.rint(c * ONE).astype(np.int64)
        sums = np.zeros((m, 3), np.int64)
        np.add.at(sums, inv, fixed)
        v = sums.astype(np.float64)
        length = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
        with np.errstate(invalid="ignore", divide="ignore"):
            out_n = np.where(length[:, None] == 0, 0.0, v / length[:, None]).astype(np.float32)
    return pts, counts.astype(np.int32), out_c, out_n


def apply_frame(q, origin, step):
    return np.asarray(origin, np.float64) + np.asarray(q).astype(np.float64) * np.float64(step)


def voxelize_scan(points, colors=None, normals=None, frame=None, bits=None, voxel_size=None):
    """-> (points, colors, normals, counts, (origin, step, bits), n_dropped)"""
    if frame is None:
        frame = fit_frame(points, bits, voxel_size)
    n_dropped = bounds(points)[2]
    _, keys = quantize(points, *frame)
    pts, counts, c, n = merge(keys, frame[2], colors, normals)
    return pts, c, n, counts, frame, n_dropped
