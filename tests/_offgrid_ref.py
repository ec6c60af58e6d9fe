"""The off-grid D1 / D2 rule (include/pcgc.h, pcgc_offgrid_*; metrics.pc_error_off_grid) in numpy by brute force over all
pairs: no k-d tree, no cell grid, no cap on ties.  Small clouds only (the pair matrix is dense)."""
import numpy as np

TIE = 1e-8               # on squared distances, absolute
FIX = 2.0 ** 40          # fixed point of the normal sums


def scaled_back(points, scale):
    """what process.py makes of a cloud at a rate with that scale: round(float32 * scale), unique, then * float(1 / scale)"""
    p = np.round(np.asarray(points).astype("float32") * scale)
    return np.unique(p, axis=0).astype("float32") * float(1 / scale)


def _delta(p, q):
    """p - q per pair and axis, float64 [len(p), len(q), 3], from the float32 coordinates"""
    p, q = (np.asarray(x, np.float32).astype(np.float64) for x in (p, q))
    return p[:, None, :] - q[None, :, :]


def dist2(p, q):
    d = _delta(p, q)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def search(p, q):
    """-> (best float64 [len(p)], tie bool [len(p), len(q)]): the minimal squared distance and every q within TIE of it"""
    d2 = dist2(p, q)
    best = d2.min(1)
    return best, np.abs(d2 - best[:, None]) < TIE


def transfer_normals(tie, normals_p):
    """normals of the target, float64 [len(q), 3]: the int64 sum of rint(n 2^40) over the points that chose it / 2^40 / count"""
    fixed = np.rint(np.asarray(normals_p, np.float32).astype(np.float64) * FIX).astype(np.int64)
    sums, count = tie.T.astype(np.int64) @ fixed, tie.sum(0)
    return np.where(count[:, None] > 0, sums.astype(np.float64) / FIX / np.maximum(count, 1)[:, None], 0.0)


def plane(p, q, normals_q, tie):
    """per point of p the mean over its tied q of ((p - q) . n_q)^2, the dot product as (dx nx + dy ny) + dz nz"""
    d, n = _delta(p, q), np.asarray(normals_q, np.float64)
    dot = (d[..., 0] * n[None, :, 0] + d[..., 1] * n[None, :, 1]) + d[..., 2] * n[None, :, 2]
    return np.where(tie, dot * dot, 0.0).sum(1) / tie.sum(1)


def one_way(p, q, normals_q=None):
    """-> dict(best, n_ties, tie, plane (or None)) of the direction p -> q"""
    best, tie = search(p, q)
    return {"best": best, "tie": tie, "n_ties": tie.sum(1).astype(np.int32),
            "plane": None if normals_q is None else plane(p, q, normals_q, tie)}


def pc_error(a, b, normals_a=None, resolution=1023):
    """the dict of metrics.pc_error_off_grid (B deduplicated as float32 rows), plus the per-point parts under "_1", "_2" and
    B's transferred normals under "_normals_b" (np.unique's order)"""
    a = np.asarray(a, np.float32)
    b = np.unique(np.asarray(b, np.float32), axis=0)
    ab = one_way(a, b)
    nb = na = None
    if normals_a is not None:
        na = np.asarray(normals_a, np.float32).astype(np.float64)
        nb = transfer_normals(ab["tie"], normals_a)
        ab["plane"] = plane(a, b, nb, ab["tie"])
    ba = one_way(b, a, na)
    peak = float(resolution)

    def psnr(m):
        return float("inf") if m == 0 else 10.0 * np.log10(3.0 * peak * peak / m)
    out = {"_1": ab, "_2": ba, "_normals_b": nb, "_b": b}
    for what, key in (("p2point", "best"),) + ((("p2plane", "plane"),) if normals_a is not None else ()):
        m1, m2 = float(ab[key].mean()), float(ba[key].mean())
        h1, h2 = float(ab[key].max()), float(ba[key].max())
        out.update({"mse1      (%s)" % what: m1, "mse2      (%s)" % what: m2, "mseF      (%s)" % what: max(m1, m2),
                    "mse1,PSNR (%s)" % what: psnr(m1), "mse2,PSNR (%s)" % what: psnr(m2), "mseF,PSNR (%s)" % what: psnr(max(m1, m2)),
                    "h.       1(%s)" % what: h1, "h.       2(%s)" % what: h2, "h.        (%s)" % what: max(h1, h2)})
    return out


def _dense(seed, res, n):
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from _clouds import dense
    return dense(seed, res, n)[0]


def _normals(seed, n):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(n, 3)) * rng.uniform(0.5, 2.0, (n, 1))).astype(np.float32)


def _scaled_case(seed, res, n, scale, drop):
    a = _dense(seed, res, n)
    b = scaled_back(a, scale)
    if drop:
        b = b[~(np.random.default_rng(7).random(len(b)) < 0.3)]
    return a.astype(np.float32), b, _normals(100 + seed, len(a))


def cases():
    """name -> (A float32, B float32, normals of A float32): the seeded pairs the off-grid tests share"""
    rng = np.random.default_rng(11)
    fa, fb = rng.uniform(0, 20, (800, 3)).astype(np.float32), rng.uniform(0, 20, (600, 3)).astype(np.float32)
    twelve = np.array([[2 + s * 1.5 if k == i else 2 + t * 1.5 if k == j else 2 for k in range(3)]
                       for i, j in ((0, 1), (0, 2), (1, 2)) for s in (-1, 1) for t in (-1, 1)], np.float32)
    one = np.array([[1.0, 0.5, -0.25]], np.float32)
    # a rod 1500 long across zero: more than 1024 unit cells, so the search takes cells of edge 2, with a negative origin
    rod = np.array([1500.0, 8.0, 8.0]), np.array([-700.3, -3.0, 0.0])
    ra, rb = ((rng.uniform(0, 1, (n, 3)) * rod[0] + rod[1]).astype(np.float32) for n in (500, 400))
    return {
        "s5_8": _scaled_case(1, 24, 1500, 0.625, True),
        "s3_4": _scaled_case(2, 24, 1500, 0.75, True),
        "s8_5": _scaled_case(3, 16, 600, 1.6, False),
        "far": (np.zeros((1, 3), np.float32), np.array([[39.5, 39.25, 39.75]], np.float32), one),
        "twelve_ties": (np.array([[2, 2, 2]], np.float32), twelve, one),
        "both_float": (fa, fb, rng.normal(size=(800, 3)).astype(np.float32)),
        "rod_edge_2": (ra, rb, rng.normal(size=(500, 3)).astype(np.float32)),
    }
