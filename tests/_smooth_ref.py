"""The smoothing rule of include/pcgc.h (pcgc_smooth_step) and pcgcv1_amd/smooth.py in numpy: what the device must equal bit
for bit.  Candidate neighbours come from a k-d tree with a little slack; membership is decided by the rule's own d2.  The
Jacobi loop of csrc/jacobi3.h is restated operation for operation, vectorised over the points with masks."""
import numpy as np
from scipy.spatial import cKDTree

SCALE = 65536.0


def pairs(g, radius):
    """-> (i, j) int64, sorted by i: every ordered pair with d2(g_i, g_j) <= radius * radius, i == j included"""
    g64 = np.asarray(g, np.float32).astype(np.float64).reshape(-1, 3)
    n = len(g64)
    und = cKDTree(g64).query_pairs(float(radius) * (1.0 + 1e-9) + 1e-9, output_type="ndarray").astype(np.int64).reshape(-1, 2)
    i = np.concatenate([np.arange(n), und[:, 0], und[:, 1]])
    j = np.concatenate([np.arange(n), und[:, 1], und[:, 0]])
    d = g64[i] - g64[j]
    keep = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) <= float(radius) * float(radius)
    i, j = i[keep], j[keep]
    order = np.argsort(i, kind="stable")
    return i[order], j[order]


def moments(g, radius):
    """-> (K int32 [n], S int64 [n,3], Q int64 [n,6]: c00 c01 c02 c11 c12 c22)"""
    g64 = np.asarray(g, np.float32).astype(np.float64).reshape(-1, 3)
    n = len(g64)
    i, j = pairs(g, radius)
    o = np.rint((g64[j] - g64[i]) * SCALE).astype(np.int64)
    K = np.bincount(i, minlength=n).astype(np.int32)
    first = np.concatenate([[0], np.cumsum(K.astype(np.int64))[:-1]])           # every point is its own neighbour: K >= 1
    terms = np.stack([o[:, 0], o[:, 1], o[:, 2], o[:, 0] * o[:, 0], o[:, 0] * o[:, 1], o[:, 0] * o[:, 2], o[:, 1] * o[:, 1],
                      o[:, 1] * o[:, 2], o[:, 2] * o[:, 2]], 1)
    sums = np.add.reduceat(terms, first, axis=0)
    return K, sums[:, :3].copy(), sums[:, 3:].copy()


def jacobi3(a):
    """a float64 [n,3,3] symmetric (destroyed) -> v [n,3,3]: eigenvalues on a's diagonal, eigenvectors in v's columns"""
    n = len(a)
    v = np.zeros((n, 3, 3))
    v[:, 0, 0] = v[:, 1, 1] = v[:, 2, 2] = 1.0
    done = np.zeros(n, bool)
    with np.errstate(all="ignore"):
        for sweep in range(32):
            done |= (a[:, 0, 1] == 0.0) & (a[:, 0, 2] == 0.0) & (a[:, 1, 2] == 0.0)
            if done.all():
                break
            for p, q in ((0, 1), (0, 2), (1, 2)):
                apq = a[:, p, q].copy()
                act = ~done & (apq != 0.0)
                if sweep > 3:
                    gg = 100.0 * np.abs(apq)
                    app, aqq = np.abs(a[:, p, p]), np.abs(a[:, q, q])
                    small = act & (app + gg == app) & (aqq + gg == aqq)
                    a[small, p, q] = 0.0
                    a[small, q, p] = 0.0
                    act &= ~small
                r = np.nonzero(act)[0]
                if not len(r):
                    continue
                x = a[r]
                theta = (x[:, q, q] - x[:, p, p]) / (2.0 * apq[r])
                t = np.where(theta >= 0.0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                for k in range(3):                               # a <- a J (columns p, q)
                    akp, akq = x[:, k, p].copy(), x[:, k, q].copy()
                    x[:, k, p] = c * akp - s * akq
                    x[:, k, q] = s * akp + c * akq
                for k in range(3):                               # a <- J^T a (rows p, q)
                    apk, aqk = x[:, p, k].copy(), x[:, q, k].copy()
                    x[:, p, k] = c * apk - s * aqk
                    x[:, q, k] = s * apk + c * aqk
                x[:, p, q] = 0.0
                x[:, q, p] = 0.0
                a[r] = x
                w = v[r]
                for k in range(3):
                    vkp, vkq = w[:, k, p].copy(), w[:, k, q].copy()
                    w[:, k, p] = c * vkp - s * vkq
                    w[:, k, q] = s * vkp + c * vkq
                v[r] = w
    return v


def step(g, radius, kmin, negate=False):
    """One pass -> (out float32 [n,3], moved uint8 [n], K int32 [n], S int64 [n,3], Q int64 [n,6]).  negate: every normal
    with the other sign, which must not change a bit."""
    g = np.ascontiguousarray(np.asarray(g), np.float32).reshape(-1, 3)
    assert np.isfinite(g).all()
    K, S, Q = moments(g, radius)
    out = g.copy()
    moved = (K >= int(kmin)).astype(np.uint8)
    r = np.nonzero(moved)[0]
    if len(r):
        dk = K[r].astype(np.float64)
        m = S[r].astype(np.float64) / dk[:, None]
        q = Q[r].astype(np.float64) / dk[:, None]
        a = np.empty((len(r), 3, 3))
        a[:, 0, 0] = q[:, 0] - m[:, 0] * m[:, 0]
        a[:, 0, 1] = a[:, 1, 0] = q[:, 1] - m[:, 0] * m[:, 1]
        a[:, 0, 2] = a[:, 2, 0] = q[:, 2] - m[:, 0] * m[:, 2]
        a[:, 1, 1] = q[:, 3] - m[:, 1] * m[:, 1]
        a[:, 1, 2] = a[:, 2, 1] = q[:, 4] - m[:, 1] * m[:, 2]
        a[:, 2, 2] = q[:, 5] - m[:, 2] * m[:, 2]
        v = jacobi3(a)
        a00, a11, a22 = a[:, 0, 0], a[:, 1, 1], a[:, 2, 2]
        jx = np.where(a11 < a00, np.where(a22 < a11, 2, 1), np.where(a22 < a00, 2, 0))
        nrm = v[np.arange(len(r)), :, jx]
        nrm = nrm / np.sqrt((nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1]) + nrm[:, 2] * nrm[:, 2])[:, None]
        if negate:
            nrm = -nrm
        t = (m[:, 0] * nrm[:, 0] + m[:, 1] * nrm[:, 1]) + m[:, 2] * nrm[:, 2]
        d = t / SCALE
        out[r] = (g[r].astype(np.float64) + d[:, None] * nrm).astype(np.float32)
    return out, moved, K, S, Q


def chain(g, radius, iters, kmin, negate=False):
    """`iters` passes, each on the output of the one before -> (g' float32 [n,3], moved bool [n]: some pass moved the row)"""
    g = np.ascontiguousarray(np.asarray(g), np.float32).reshape(-1, 3)
    any_moved = np.zeros(len(g), bool)
    for _ in range(int(iters)):
        g, moved = step(g, radius, kmin, negate)[:2]
        any_moved |= moved != 0
    return g, any_moved


def to_grid(points, origin, step_):
    return ((np.asarray(points, np.float64).reshape(-1, 3) - np.asarray(origin, np.float64)) / np.float64(step_)).astype(np.float32)


def scan(points, origin, step_, radius, iters, kmin):
    """pcgcv1_amd.smooth.smooth_scan: -> (p' float64 [n,3], moved bool [n]); a row no pass moved, or with a coordinate that is
    not finite, keeps its bits"""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    out = p.copy()
    finite = np.isfinite(p).all(1)
    moved_all = np.zeros(len(p), bool)
    if finite.any():
        g2, moved = chain(to_grid(p[finite], origin, step_), radius, iters, kmin)
        rows = np.nonzero(finite)[0][moved]
        out[rows] = np.asarray(origin, np.float64) + g2[moved].astype(np.float64) * np.float64(step_)
        moved_all[rows] = True
    return out, moved_all


# ---------------------------------------------------------------------------- what it is for: the figures of a thinned cloud
def voxels(points, origin, step_, bits):
    """ingest's quantisation -> the number of occupied voxels"""
    q = np.clip(np.floor((np.asarray(points, np.float64) - np.asarray(origin, np.float64)) / np.float64(step_) + 0.5), 0, 2 ** bits - 1)
    return len(np.unique(q.astype(np.int64), axis=0))


def rms_to(points, dense_tree):
    d = dense_tree.query(np.asarray(points, np.float64))[0]
    return float(np.sqrt((d * d).mean()))
