"""The surface rule (include/pcgc.h, pcgc_surface_*; pcgcv1_amd/surface.py) in numpy, float64, in the expression
order the header states: orientation of estimated normals by Jacobi rounds over the link graph, the moving-least-squares signed
distance on the half-offset lattice, and marching tetrahedra over the Kuhn cut of every candidate cell.  Also the shapes the
tests share and the mesh measures they assert.  Not collected by pytest."""
import itertools

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

DEFAULT_TAU = (0.9, 0.0)
PERMS = list(itertools.permutations(range(3)))
DIRS = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)]


def keys(points, bits):
    p = np.asarray(points, np.int64).reshape(-1, 3)
    res = np.int64(1) << bits
    return (p[:, 0] * res + p[:, 1]) * res + p[:, 2]


def vertex_keys(k, bits):
    """lattice vertices k in [-2, res]^3 -> their key on the padded lattice of res + 3 per axis"""
    k = np.asarray(k, np.int64).reshape(-1, 3) + 2
    side = (np.int64(1) << bits) + 3
    return (k[:, 0] * side + k[:, 1]) * side + k[:, 2]


def vertex_of_key(key, bits):
    key = np.asarray(key, np.int64)
    side = (np.int64(1) << bits) + 3
    return np.stack([key // (side * side), key // side % side, key % side], -1) - 2


def _index_map(points, bits, pad):
    """dense int32 map over [-pad, res + pad)^3: the row of the voxel there, or -1"""
    res = 1 << bits
    m = np.full((res + 2 * pad,) * 3, -1, np.int32)
    p = np.asarray(points, np.int64) + pad
    m[p[:, 0], p[:, 1], p[:, 2]] = np.arange(len(p), dtype=np.int32)
    return m


def _links(points, bits, gap):
    """nbr int32 [n, (2G+1)^3 - 1]: the rows of the linked voxels in ascending key order (offsets ascending), -1 where none"""
    p = np.asarray(points, np.int64).reshape(-1, 3)
    m = _index_map(p, bits, gap)
    cols = []
    for o in itertools.product(range(-gap, gap + 1), repeat=3):
        if o != (0, 0, 0):
            q = p + gap + o
            cols.append(m[q[:, 0], q[:, 1], q[:, 2]])
    return np.stack(cols, 1)


def components(points, bits, gap=1):
    """pcgc_clean_components' label (the smallest key of the component) and the number of components, through the link table"""
    p = np.asarray(points, np.int64).reshape(-1, 3)
    n = len(p)
    nbr = _links(p, bits, gap)
    i, o = np.nonzero(nbr >= 0)
    graph = coo_matrix((np.ones(len(i), np.int8), (i, nbr[i, o])), shape=(n, n))
    n_components, comp = connected_components(graph, directed=False)
    smallest = np.full(n_components, np.iinfo(np.int64).max)
    np.minimum.at(smallest, comp, keys(p, bits))
    return smallest[comp], int(n_components)


def check_tau(tau):
    tau = tuple(float(t) for t in tau)
    if not 1 <= len(tau) <= 8 or tau[-1] != 0.0 or not all(0.0 <= t <= 1.0 for t in tau):
        raise ValueError("surface: the stage thresholds %r must be 1 to 8 values within [0, 1], the last of them 0.0" % (tau,))
    return tau


def orient(points, normals, bits, mode="propagate", gap=1, tau=DEFAULT_TAU, view=None):
    """-> (sign int8 [n], rounds)"""
    p = np.asarray(points, np.int64).reshape(-1, 3)
    nr = np.asarray(normals, np.float32).reshape(-1, 3).astype(np.float64)
    n = len(p)
    if mode == "given":
        return np.ones(n, np.int8), 0
    if mode == "view":
        X, Y, Z = (np.float64(v) for v in view)
        d = (nr[:, 0] * (X - p[:, 0]) + nr[:, 1] * (Y - p[:, 1])) + nr[:, 2] * (Z - p[:, 2])
        return np.where(d < 0, -1, 1).astype(np.int8), 0
    tau = check_tau(tau)
    label, _ = components(p, bits, gap)
    key = keys(p, bits)
    order = np.lexsort((key, label))
    last = np.r_[label[order][1:] != label[order][:-1], True]           # the largest key of every label
    sign = np.zeros(n, np.int8)
    seeds = order[last]
    sign[seeds] = np.where(nr[seeds, 0] < 0, -1, 1)
    nbr = _links(p, bits, gap)
    j = np.maximum(nbr, 0)
    c = (nr[:, None, 0] * nr[j, 0] + nr[:, None, 1] * nr[j, 1]) + nr[:, None, 2] * nr[j, 2]
    rounds, k = 0, 0
    while (sign == 0).any():
        rounds += 1
        todo = np.nonzero(sign == 0)[0]
        usable = (nbr[todo] >= 0) & (sign[j[todo]] != 0)
        a = np.where(usable, np.abs(c[todo]), -1.0)
        best = np.argmax(a, 1)                                           # the first of equal |c|: the smallest key
        ab = a[np.arange(len(todo)), best]
        take = ab >= tau[k]                                              # -1 (no set neighbour) is below every threshold
        new = sign.copy()
        jb = j[todo, best]
        new[todo[take]] = (sign[jb] * np.where(c[todo, best] >= 0, 1, -1))[take]
        k = 0 if take.any() else k + 1
        sign = new
    return sign, rounds


def oriented(normals, sign):
    return np.asarray(sign, np.float64)[:, None] * np.asarray(normals, np.float32).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------- lattice
def cells_and_vertices(points, bits):
    """candidate cells c (int64 [C,3], in [-1, res]^3) and lattice vertices k (int64 [V,3], in [-2, res]^3), each in key order"""
    p = np.asarray(points, np.int64).reshape(-1, 3)
    res = 1 << bits
    occ = np.zeros((res + 2,) * 3, bool)
    for o in itertools.product((-1, 0, 1), repeat=3):
        q = p + 1 + o
        occ[q[:, 0], q[:, 1], q[:, 2]] = True
    cells = np.argwhere(occ) - 1
    ver = np.zeros((res + 3,) * 3, bool)
    for o in itertools.product((0, 1), repeat=3):
        q = cells + 1 + o                                                # k + 2 = c - 1 + o + 2
        ver[q[:, 0], q[:, 1], q[:, 2]] = True
    return cells, np.argwhere(ver) - 2


def implicit(points, oriented_normals, bits, radius=3):
    """-> (vertex keys int64 [V] ascending, f float64 [V])"""
    if not 3 <= radius <= 8:
        raise ValueError("surface: radius = %r outside 3..8" % (radius,))
    p = np.asarray(points, np.int64).reshape(-1, 3)
    N = np.asarray(oriented_normals, np.float64).reshape(-1, 3)
    R = int(radius)
    _, k = cells_and_vertices(p, bits)
    pad = R + 3
    m = _index_map(p, bits, pad)
    num, W = np.zeros(len(k)), np.zeros(len(k))
    for o in itertools.product(range(-R, R + 2), repeat=3):              # ascending (ox, oy, oz)
        dd = [1 - 2 * v for v in o]                                      # (2k + 1) - 2q with q = k + o
        d2 = dd[0] * dd[0] + dd[1] * dd[1] + dd[2] * dd[2]
        if d2 > 4 * R * R:
            continue
        q = k + pad + o
        row = m[q[:, 0], q[:, 1], q[:, 2]]
        hit = np.nonzero(row >= 0)[0]
        if not len(hit):
            continue
        row = row[hit]
        t = np.float64(1.0) - np.float64(d2) / np.float64(4 * R * R + 1)
        w = t * t
        num[hit] += w * ((N[row, 0] * dd[0] + N[row, 1] * dd[1]) + N[row, 2] * dd[2])
        W[hit] += w
    return vertex_keys(k, bits), 0.5 * num / W


# ---------------------------------------------------------------------------------------------------------------- tetrahedra
def perm_sign(pi):
    return -1 if sum(pi[a] > pi[b] for a in range(len(pi)) for b in range(a + 1, len(pi))) % 2 else 1


def tet_corners(pi):
    """the four corners of the Kuhn tetrahedron of pi as offsets from v0"""
    c = [np.zeros(3, np.int64)]
    for axis in pi:
        nxt = c[-1].copy()
        nxt[axis] += 1
        c.append(nxt)
    return np.array(c)


def tet_triangles(pi, mask):
    """triangles of one tetrahedron whose corners with bit set in `mask` (bit i = corner i in the tetrahedron's order) are
    inside -> a list of triangles, each three lattice edges (a, b) of tetrahedron-local corner indices with a < b"""
    I = [i for i in range(4) if mask >> i & 1]
    O = [i for i in range(4) if not mask >> i & 1]
    if len(I) == 1:
        tris = [[(I[0], O[0]), (I[0], O[1]), (I[0], O[2])]]
    elif len(I) == 3:
        tris = [[(I[0], O[0]), (I[1], O[0]), (I[2], O[0])]]
    elif len(I) == 2:
        A, B, C, D = (I[0], O[0]), (I[0], O[1]), (I[1], O[1]), (I[1], O[0])
        tris = [[A, B, C], [A, C, D]]
    else:
        return []
    if perm_sign(pi) * perm_sign(I + O) < 0:                             # the combinatorial winding: no floating-point test
        tris = [[t[0], t[2], t[1]] for t in tris]
    return [[(min(e), max(e)) for e in t] for t in tris]


def edge_ids(a, d, bits):
    """lattice edge from vertex a (int64 [..,3]) in direction d (a DIRS entry) -> int64 id"""
    return vertex_keys(a, bits) * 7 + DIRS.index(tuple(int(v) for v in d))


def marching_tetrahedra(cells, vkeys, f, bits):
    """-> (vertices float64 [V,3] in ascending edge id, triangles int32 [T,3], edge ids int64 [V])"""
    corner = np.array(list(itertools.product((0, 1), repeat=3)), np.int64)
    v0 = np.asarray(cells, np.int64) - 1
    fc = np.empty((len(v0), 2, 2, 2))
    for o in corner:
        at = np.searchsorted(vkeys, vertex_keys(v0 + o, bits))
        fc[:, o[0], o[1], o[2]] = f[at]
    inside = fc < 0
    tri_ids = []
    for pi in PERMS:
        tc = tet_corners(pi)
        mask = sum(inside[:, tc[i, 0], tc[i, 1], tc[i, 2]].astype(np.int64) << i for i in range(4))
        for m in range(1, 15):
            sel = np.nonzero(mask == m)[0]
            if not len(sel):
                continue
            for tri in tet_triangles(pi, m):
                tri_ids.append(np.stack([edge_ids(v0[sel] + tc[a], tc[b] - tc[a], bits) for a, b in tri], 1))
    tri_ids = np.concatenate(tri_ids) if tri_ids else np.zeros((0, 3), np.int64)
    ids = np.unique(tri_ids)
    a = vertex_of_key(ids // 7, bits)
    d = np.array(DIRS, np.int64)[ids % 7]
    fa = f[np.searchsorted(vkeys, vertex_keys(a, bits))]
    fb = f[np.searchsorted(vkeys, vertex_keys(a + d, bits))]
    t = fa / (fa - fb)
    vertices = (a.astype(np.float64) + 0.5) + t[:, None] * d.astype(np.float64)
    return vertices, np.searchsorted(ids, tri_ids).astype(np.int32), ids


def reconstruct(points, normals, bits, radius=3, mode="propagate", gap=1, tau=DEFAULT_TAU, view=None):
    """-> (vertices, triangles, report dict)"""
    sign, rounds = orient(points, normals, bits, mode, gap, tau, view)
    vkeys, f = implicit(points, oriented(normals, sign), bits, radius)
    cells, _ = cells_and_vertices(points, bits)
    vertices, triangles, _ = marching_tetrahedra(cells, vkeys, f, bits)
    return vertices, triangles, dict(sign=sign, rounds=rounds, vertex_keys=vkeys, f=f, cells=len(cells))


# ---------------------------------------------------------------------------------------------------------------- measures
def canonical(triangles):
    t = np.asarray(triangles).reshape(-1, 3)
    first = np.argmin(t, 1)
    t = np.stack([t[np.arange(len(t)), (first + s) % 3] for s in range(3)], 1)
    return t[np.lexsort((t[:, 2], t[:, 1], t[:, 0]))]


def edge_census(triangles):
    """-> (undirected edges [E,2], how many triangles hold each, the largest multiplicity of a directed edge)"""
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    d = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    _, dcount = np.unique(d, axis=0, return_counts=True)
    und, ucount = np.unique(np.sort(d, 1), axis=0, return_counts=True)
    return und, ucount, int(dcount.max()) if len(dcount) else 0


def euler(vertices, triangles):
    und, _, _ = edge_census(triangles)
    return len(vertices) - len(und) + len(triangles)


def boundary_loops(triangles):
    """the number of closed loops the boundary edges (held by one triangle) form, and the number of such edges"""
    und, ucount, _ = edge_census(triangles)
    b = und[ucount == 1]
    if not len(b):
        return 0, 0
    ids, inv = np.unique(b, return_inverse=True)
    inv = inv.reshape(-1, 2)
    graph = coo_matrix((np.ones(len(inv), np.int8), (inv[:, 0], inv[:, 1])), shape=(len(ids), len(ids)))
    return int(connected_components(graph, directed=False)[0]), len(b)


def signed_volume(vertices, triangles):
    v = np.asarray(vertices, np.float64)[np.asarray(triangles)]
    return float(np.einsum("ij,ij->i", v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6.0)


# ---------------------------------------------------------------------------------------------------------------- shapes
def _voxels(samples):
    return np.unique(np.rint(samples).astype(np.int64), axis=0).astype(np.int32)


def sphere(centre, r, n=200000, seed=1):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    return _voxels(np.asarray(centre, np.float64) + r * d / np.linalg.norm(d, axis=1, keepdims=True))


def torus(centre=(15.5, 15.5, 15.5), R=9.0, r=4.2, n=200000, seed=2):
    rng = np.random.default_rng(seed)
    u, v = rng.uniform(0, 2 * np.pi, (2, n))
    s = np.stack([(R + r * np.cos(v)) * np.cos(u), (R + r * np.cos(v)) * np.sin(u), r * np.sin(v)], 1)
    return _voxels(np.asarray(centre, np.float64) + s)


def paraboloid(n=100000, seed=3):
    """an open patch z = 8 + (x^2 + y^2) / 24 over a disc of radius 10 about (15.5, 15.5)"""
    rng = np.random.default_rng(seed)
    rr, a = 10.0 * np.sqrt(rng.uniform(0, 1, n)), rng.uniform(0, 2 * np.pi, n)
    x, y = rr * np.cos(a), rr * np.sin(a)
    return _voxels(np.stack([15.5 + x, 15.5 + y, 8.0 + (x * x + y * y) / 24.0], 1))


def sphere_normals(points, centre):
    d = np.asarray(points, np.float64) - np.asarray(centre, np.float64)
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
