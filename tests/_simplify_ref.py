"""The simplification rule (include/pcgc.h, pcgc_simplify_*; pcgcv1_amd/surface.py: simplify) in numpy, float64, in
the expression order the header states: vertex clustering over cubes of `cell` voxels, one vertex per cube placed at the minimum
of the summed squared distances to the planes of the triangles that touch the cube, and the triangles as the image of the input
2-chain.  np.add.at adds element by element in the order of its arguments, which is what makes the sums the rule's.  Also the
cluster-mean placement (a yardstick for the tests only) and the measures the tests assert.  Not collected by pytest."""
import numpy as np

from _smooth_ref import jacobi3

MAX_CELL = 64
RANK_EPS = 1e-3
REPORT_KEYS = ("cell", "clusters", "vertices_in", "triangles_in", "degenerate", "cancelled", "merged", "folded", "fallback", "unused")


def canonical(triangles):
    """step 0: every triangle rotated so that its smallest index comes first, the rows sorted"""
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    first = np.argmin(t, 1)
    t = np.stack([t[np.arange(len(t)), (first + s) % 3] for s in range(3)], 1)
    return t[np.lexsort((t[:, 2], t[:, 1], t[:, 0]))]


def check_input(vertices, triangles, bits, cell):
    v = np.ascontiguousarray(np.asarray(vertices, np.float64).reshape(-1, 3))
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    if int(bits) != bits or not 1 <= bits <= 12:
        raise ValueError("simplify: bits = %r outside 1..12" % (bits,))
    if int(cell) != cell or not 1 <= cell <= MAX_CELL:
        raise ValueError("simplify: cell = %r outside 1..%d" % (cell, MAX_CELL))
    res = 1 << int(bits)
    if not (np.isfinite(v).all() and (v >= -2.0).all() and (v < res + 2.0).all()):
        raise ValueError("simplify: a vertex is not finite or outside [-2, %d)" % (res + 2))
    if len(t) and (t.min() < 0 or t.max() >= len(v)):
        raise ValueError("simplify: a triangle names a vertex outside 0..%d" % (len(v) - 1))
    return v, t, int(bits), int(cell)


def clusters(v, bits, cell):
    """step 1 -> (keys int64 [K] ascending, rank int64 [V], centre float64 [K,3])"""
    res = 1 << bits
    M = (res + 4 + cell - 1) // cell
    c = np.floor((v + 2.0) / np.float64(cell)).astype(np.int64)
    key = (c[:, 0] * M + c[:, 1]) * M + c[:, 2]
    keys, rank = np.unique(key, return_inverse=True)
    c = np.stack([keys // (M * M), keys // M % M, keys % M], 1)
    return keys, rank.reshape(-1), (c.astype(np.float64) + 0.5) * np.float64(cell) - 2.0


def quadric_terms(q0, q1, q2):
    """step 2, one triangle per row, q relative to the cluster's centre -> [n,9]: a00 a01 a02 a11 a12 a22 b0 b1 b2"""
    e1, e2 = q1 - q0, q2 - q0
    nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    d = -((nx * q0[:, 0] + ny * q0[:, 1]) + nz * q0[:, 2])
    return np.stack([nx * nx, nx * ny, nx * nz, ny * ny, ny * nz, nz * nz, nx * d, ny * d, nz * d], 1)


def place(Q, m, cell):
    """step 3: Q float64 [K,9], m float64 [K,3] -> (x float64 [K,3] relative to the centre, fallback bool [K])"""
    K = len(Q)
    A = np.empty((K, 3, 3))
    A[:, 0, 0], A[:, 1, 1], A[:, 2, 2] = Q[:, 0], Q[:, 3], Q[:, 5]
    A[:, 0, 1] = A[:, 1, 0] = Q[:, 1]
    A[:, 0, 2] = A[:, 2, 0] = Q[:, 2]
    A[:, 1, 2] = A[:, 2, 1] = Q[:, 4]
    r = np.stack([(-Q[:, 6 + i]) - ((A[:, i, 0] * m[:, 0] + A[:, i, 1] * m[:, 1]) + A[:, i, 2] * m[:, 2]) for i in range(3)], 1)
    a = A.copy()
    E = jacobi3(a)
    lam = np.stack([a[:, 0, 0], a[:, 1, 1], a[:, 2, 2]], 1)
    lmax = np.maximum(np.maximum(lam[:, 0], lam[:, 1]), lam[:, 2])
    threshold = RANK_EPS * lmax
    s = np.zeros((K, 3))
    with np.errstate(all="ignore"):
        for i in range(3):
            use = lam[:, i] > threshold
            t = ((E[:, 0, i] * r[:, 0] + E[:, 1, i] * r[:, 1]) + E[:, 2, i] * r[:, 2]) / lam[:, i]
            for j in range(3):
                s[:, j] = np.where(use, s[:, j] + E[:, j, i] * t, s[:, j])
    x = m + s
    fallback = ~(lmax > 0.0) | (np.abs(x) > np.float64(cell) / 2.0).any(1)
    return np.where(fallback[:, None], m, x), fallback


def place_clusters(items):
    """steps 2 and 3 on hand-made clusters, what tests/surface_quadric_check.cpp feeds csrc/surface_quadric.h: items = a list of
    (cell, centre [3], vertices [nv,3], triangles [nt,3,3] of corner coordinates) -> (placed float64 [n,3], fallback bool [n])"""
    out, flags = [], []
    for cell, o, vs, ts in items:
        o = np.asarray(o, np.float64)
        vs = np.asarray(vs, np.float64).reshape(-1, 3)
        ts = np.asarray(ts, np.float64).reshape(-1, 3, 3)
        Q, s = np.zeros((1, 9)), np.zeros((1, 3))
        if len(ts):
            np.add.at(Q, np.zeros(len(ts), np.int64), quadric_terms(ts[:, 0] - o, ts[:, 1] - o, ts[:, 2] - o))
        np.add.at(s, np.zeros(len(vs), np.int64), vs - o)
        x, fb = place(Q, s / np.float64(len(vs)), cell)
        out.append(o + x[0])
        flags.append(bool(fb[0]))
    return np.array(out).reshape(-1, 3), np.array(flags, bool)


def simplify(vertices, triangles, bits, cell, placement="quadric", vertex_map=False):
    """-> (vertices float64 [V',3], triangles int32 [T',3], report dict).  placement 'mean': every cluster at the mean of its
    vertices, the plain vertex clustering the quadric is measured against.  vertex_map: a fourth value, int64 [V], the output
    vertex every input vertex went to, -1 where its cluster was removed."""
    v, t, bits, cell = check_input(vertices, triangles, bits, cell)
    t = canonical(t)
    T = len(t)
    keys, rank, centre = clusters(v, bits, cell)
    K = len(keys)
    # the mean, in ascending vertex index
    s, count = np.zeros((K, 3)), np.zeros(K, np.int64)
    np.add.at(s, rank, v - centre[rank])
    np.add.at(count, rank, 1)
    m = s / count[:, None].astype(np.float64)
    # the quadric: a triangle once for each distinct cluster of its corners, every cluster's in ascending canonical position
    tr = rank[t].reshape(-1, 3)
    first = np.ones((T, 3), bool)
    first[:, 1] = tr[:, 1] != tr[:, 0]
    first[:, 2] = (tr[:, 2] != tr[:, 0]) & (tr[:, 2] != tr[:, 1])
    pos, k = np.nonzero(first)                                           # row-major: ascending position
    cl = tr[pos, k]
    Q = np.zeros((K, 9))
    if len(pos):
        q = v[t[pos]] - centre[cl][:, None, :]
        np.add.at(Q, cl, quadric_terms(q[:, 0], q[:, 1], q[:, 2]))
    x, fallback = place(Q, m, cell)
    if placement == "mean":
        x = m
    elif placement != "quadric":
        raise ValueError(placement)
    placed = centre + x
    # the triangles as a chain
    deg = (tr[:, 0] == tr[:, 1]) | (tr[:, 1] == tr[:, 2]) | (tr[:, 0] == tr[:, 2])
    a = tr[~deg]
    f = np.argmin(a, 1) if len(a) else np.zeros(0, np.int64)
    a = np.stack([a[np.arange(len(a)), (f + s_) % 3] for s_ in range(3)], 1).reshape(-1, 3)
    sign = np.where(a[:, 1] < a[:, 2], 1, -1).astype(np.int64)
    un = np.stack([a[:, 0], np.minimum(a[:, 1], a[:, 2]), np.maximum(a[:, 1], a[:, 2])], 1)
    triples, inv = np.unique(un, axis=0, return_inverse=True)            # rows ascending in (a, lo, hi)
    triples = triples.reshape(-1, 3)
    mult, total = np.zeros(len(triples), np.int64), np.zeros(len(triples), np.int64)
    np.add.at(mult, inv.reshape(-1), sign)
    np.add.at(total, inv.reshape(-1), 1)
    live = mult != 0
    kept = triples[live]
    tri = np.where((mult[live] > 0)[:, None], kept, kept[:, [0, 2, 1]]).reshape(-1, 3)
    used = np.unique(tri)
    report = dict(cell=cell, clusters=K, vertices_in=len(v), triangles_in=T, degenerate=int(deg.sum()), cancelled=int((~live).sum()),
                  merged=int((total > 1).sum()), folded=int((np.abs(mult) >= 2).sum()), fallback=int(fallback.sum()), unused=K - len(used))
    out = placed[used], np.searchsorted(used, tri).astype(np.int32).reshape(-1, 3), report
    if not vertex_map:
        return out
    index = np.full(K, -1, np.int64)
    index[used] = np.arange(len(used))
    return out + (index[rank],)


# ---------------------------------------------------------------------------------------------------------------- measures
def edge_balance(triangles):
    """-> (undirected edges int64 [E,2], balance int64 [E]: traversals a -> b minus b -> a with a < b, count int64 [E])"""
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    d = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    s = np.where(d[:, 0] < d[:, 1], 1, -1)
    und, inv = np.unique(np.sort(d, 1), axis=0, return_inverse=True)
    balance, count = np.zeros(len(und), np.int64), np.zeros(len(und), np.int64)
    np.add.at(balance, inv.reshape(-1), s)
    np.add.at(count, inv.reshape(-1), 1)
    return und.reshape(-1, 2), balance, count
