"""A stencil statement of the nearest-cell rules of csrc/voxel_grid.h for clouds too large for an N x M distance matrix.

The brute-force references (tests/test_gpu_d1d2_exact.py _dist2 / _plane, tests/_color_ref.py) are quadratic.  Here both
clouds lie inside one block of side S <= 160 at any integer offset, the searched cloud is a dense S^3 boolean array, and the
offsets within d^2 <= max_d2 are tried in the order for_each_at_distance documents: d^2 ascending, then dx ascending, dy
ascending, z + dz before z - dz.  A query is done at the first d^2 that hits; every hit at that d^2 is one of its tied nearest
targets.  Every query must find a target within max_d2 (an assertion: the inputs of the GPU tests keep queries near their
targets, since the device search walks Chebyshev shells at cubic cost).

tied(queries, targets) is the search; the functions below derive from it what the kernels of csrc/tail.hip and csrc/color.hip
compute, integers exactly and float64 sums in the kernels' per-point order.  tests/test_grid_ref_host.py pins all of it to the
brute-force references on their small cases.
"""
import numpy as np

MAX_SIDE = 160
NORMAL_FIX = 2.0 ** 40


def offsets(max_d2=9):
    """int64 [K,3] and their d^2 [K]: every offset with d^2 <= max_d2, sorted by (d^2, dx, dy, z + dz before z - dz)"""
    r = int(np.floor(np.sqrt(max_d2)))
    g = np.arange(-r, r + 1)
    d = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.int64)
    d2 = (d * d).sum(1)
    d, d2 = d[d2 <= max_d2], d2[d2 <= max_d2]
    order = np.lexsort((-d[:, 2], d[:, 1], d[:, 0], d2))
    return d[order], d2[order]


class Tied(object):
    """best int64 [n]: the squared distance of every query to its nearest target; (qi, tj) int64 [P]: the pairs of a query
    and each of its tied nearest targets (indices into the arrays given), sorted by query, a query's pairs in the order of
    for_each_at_distance; count int64 [n] = pairs per query"""

    def __init__(self, best, qi, tj, n_targets):
        self.best, self.qi, self.tj, self.n_targets = best, qi, tj, n_targets
        self.count = np.bincount(qi, minlength=len(best)).astype(np.int64)


def tied(queries, targets, max_d2=9):
    q, t = np.asarray(queries, np.int64).reshape(-1, 3), np.asarray(targets, np.int64).reshape(-1, 3)
    off, off_d2 = offsets(max_d2)
    pad = int(np.abs(off).max())
    lo = np.minimum(q.min(0), t.min(0))
    side = int((np.maximum(q.max(0), t.max(0)) - lo).max()) + 1
    assert side <= MAX_SIDE, "the clouds span %d cells; the dense block holds %d" % (side, MAX_SIDE)
    w = side + 2 * pad
    index = np.full(w * w * w, -1, np.int32)                                # the target's index per cell of the padded block
    tf = ((t[:, 0] - lo[0] + pad) * w + (t[:, 1] - lo[1] + pad)) * w + (t[:, 2] - lo[2] + pad)
    index[tf] = np.arange(len(t), dtype=np.int32)
    assert len(np.unique(tf)) == len(t), "the target cloud holds duplicate points"
    qf = ((q[:, 0] - lo[0] + pad) * w + (q[:, 1] - lo[1] + pad)) * w + (q[:, 2] - lo[2] + pad)
    shift = (off[:, 0] * w + off[:, 1]) * w + off[:, 2]
    best = np.full(len(q), -1, np.int64)
    active = np.arange(len(q))
    qi, tj, ko = [], [], []
    for level in np.unique(off_d2):
        if active.size == 0:
            break
        found = np.zeros(active.size, bool)
        for k in np.flatnonzero(off_d2 == level):
            j = index[qf[active] + shift[k]]
            hit = j >= 0
            qi.append(active[hit])
            tj.append(j[hit].astype(np.int64))
            ko.append(np.full(int(hit.sum()), k, np.int64))
            found |= hit
        best[active[found]] = level
        active = active[~found]
    assert active.size == 0, "%d queries have no target within d^2 <= %d" % (active.size, max_d2)
    qi, tj, ko = np.concatenate(qi), np.concatenate(tj), np.concatenate(ko)
    order = np.lexsort((ko, qi))
    return Tied(best, qi[order], tj[order], len(t))


# ------------------------------------------------------------------------------------------------------------ D1 / D2
def d1(td):
    """-> (mse, largest squared distance) as pcgc_d1_mse writes them: integer sums, one division"""
    return float(np.float64(int(td.best.sum())) / np.float64(len(td.best))), float(td.best.max())


def transfer_normals(td, normals_q):
    """pcgc_d2_transfer_normals: per target the mean of the normals of the queries that chose it, by the integer rule
    llrint(n 2^40) summed in int64, float32(float64(sum) / 2^40 / count); zero where no query chose it -> float32 [m,3]"""
    fixed = np.rint(np.asarray(normals_q, np.float32).astype(np.float64) * NORMAL_FIX).astype(np.int64)
    sums = np.zeros((td.n_targets, 3), np.int64)
    np.add.at(sums, td.tj, fixed[td.qi])
    count = np.bincount(td.tj, minlength=td.n_targets)
    return np.where(count[:, None] > 0, sums.astype(np.float64) / NORMAL_FIX / np.maximum(count, 1)[:, None], 0.0).astype(np.float32)


def plane(td, queries, targets, normals_t):
    """per query: the mean over its tied targets of ((p - q) . normal(q))^2 in float64, summed in the tie order"""
    e = (np.asarray(queries, np.int64)[td.qi] - np.asarray(targets, np.int64)[td.tj]).astype(np.float64)
    n = np.asarray(normals_t, np.float32).astype(np.float64)[td.tj]
    d = e[:, 0] * n[:, 0] + e[:, 1] * n[:, 1] + e[:, 2] * n[:, 2]
    return np.bincount(td.qi, weights=d * d, minlength=len(td.best)) / td.count


def d2(td, queries, targets, normals_t):
    """-> (mse, max) of pcgc_d2_mse"""
    p = plane(td, queries, targets, normals_t)
    return float(p.mean()), float(p.max())


# ------------------------------------------------------------------------------------------------------------ colours
def _color_sums(index, pick, colors, n):
    """int64 [n,3]: per `index` value the sum of colors[pick] (exact: float64 sums of integers far below 2^53)"""
    c = np.asarray(colors, np.int64)[pick]
    return np.stack([np.bincount(index, weights=c[:, k], minlength=n) for k in range(3)], -1).astype(np.int64)


def _rounded_mean(s, n):
    return (2 * s + n[:, None]) // (2 * n[:, None])


def recolor(s_to_t, t_to_s, source_colors):
    """The rule of tests/_color_ref.py recolor from the two searches (source -> target, target -> source)
    -> (colours uint8 [N_T,3], |B(t)| int32 [N_T])"""
    n_t = s_to_t.n_targets
    back = np.bincount(s_to_t.tj, minlength=n_t).astype(np.int64)
    sums = _color_sums(s_to_t.tj, s_to_t.qi, source_colors, n_t)
    fwd = _color_sums(t_to_s.qi, t_to_s.tj, source_colors, n_t)
    use_back = back > 0
    s = np.where(use_back[:, None], sums, fwd)
    n = np.where(use_back, back, t_to_s.count)
    return _rounded_mean(s, n).astype(np.uint8), back.astype(np.int32)


def yuv_bt709(rgb):
    c = np.asarray(rgb, np.float64) / 255.0
    r, g, b = c[:, 0], c[:, 1], c[:, 2]
    return np.stack([0.2126 * r + 0.7152 * g + 0.0722 * b,
                     -0.1146 * r - 0.3854 * g + 0.5 * b + 0.5,
                     0.5 * r - 0.4542 * g - 0.0458 * b + 0.5], -1)


def color_mse(a_to_b, colors_a, colors_b):
    """one direction of pcgc_color_mse -> float64 [3]"""
    near = _rounded_mean(_color_sums(a_to_b.qi, a_to_b.tj, colors_b, len(a_to_b.best)), a_to_b.count)
    return ((yuv_bt709(colors_a) - yuv_bt709(near)) ** 2).mean(0)
