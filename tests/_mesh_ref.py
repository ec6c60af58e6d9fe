"""numpy restatement of the mesh -> point cloud rules of include/pcgc.h (pcgc_mesh_area_cdf, pcgc_mesh_sample,
pcgc_mesh_voxelize, pcgc_estimate_normals), written from those rules, and a few generated test meshes.  Not collected
(no test_ prefix): imported by tests/test_mesh_host.py and tests/test_gpu_mesh2pc.py."""
import numpy as np

_GOLDEN = np.uint64(0x9E3779B97F4A7C15)
_MIX1 = np.uint64(0xBF58476D1CE4E5B9)
_MIX2 = np.uint64(0x94D049BB133111EB)


# ---------------------------------------------------------------------------------------------------------- sampling
def area_cdf(v, t):
    v = np.asarray(v, np.float64)
    t = np.asarray(t, np.int64)
    p0, p1, p2 = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    e, f = p1 - p0, p2 - p0
    cx = e[:, 1] * f[:, 2] - e[:, 2] * f[:, 1]
    cy = e[:, 2] * f[:, 0] - e[:, 0] * f[:, 2]
    cz = e[:, 0] * f[:, 1] - e[:, 1] * f[:, 0]
    return np.cumsum(0.5 * np.sqrt((cx * cx + cy * cy) + cz * cz))


def uniforms(seed, n):
    """-> [3, n] draws: u_k of sample i from the (3i + k + 1)-th splitmix64 output of `seed`"""
    i = np.arange(n, dtype=np.uint64)
    out = np.empty((3, n), np.float64)
    for k in range(3):
        z = np.uint64(seed) + (np.uint64(3) * i + np.uint64(k + 1)) * _GOLDEN
        z = (z ^ (z >> np.uint64(30))) * _MIX1
        z = (z ^ (z >> np.uint64(27))) * _MIX2
        z = z ^ (z >> np.uint64(31))
        out[k] = (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    return out


def sample(v, t, n, seed, rot=None):
    v = np.asarray(v, np.float64)
    t = np.asarray(t, np.int64)
    cdf = area_cdf(v, t)
    u0, u1, u2 = uniforms(seed, n)
    total = cdf[-1]
    tri = np.searchsorted(cdf, u0 * total, side="right")
    tri[tri == len(cdf)] = np.searchsorted(cdf, total, side="left")
    s = np.sqrt(u1)
    a, b, c = 1.0 - s, s * (1.0 - u2), s * u2
    tt = t[tri]
    p = (a[:, None] * v[tt[:, 0]] + b[:, None] * v[tt[:, 1]]) + c[:, None] * v[tt[:, 2]]
    if rot is not None:
        m = np.asarray(rot, np.float64)
        p = np.stack([(p[:, 0] * m[0, k] + p[:, 1] * m[1, k]) + p[:, 2] * m[2, k] for k in range(3)], -1)
    return p


def voxelize(p, resolution):
    p = np.asarray(p, np.float64)
    m = p.min()
    s = p - m
    big = s.max()
    q = np.round(s / big * resolution) if big > 0 else np.zeros_like(s)
    return np.unique(q.astype(np.int64), axis=0).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------- normals
def offset_table(radius):
    r2 = int(np.floor(radius * radius))
    r = int(np.floor(np.sqrt(r2)))
    g = np.arange(-r, r + 1)
    d = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    d2 = (d * d).sum(1)
    d, d2 = d[d2 <= r2], d2[d2 <= r2]
    order = np.lexsort((d[:, 2], d[:, 1], d[:, 0], d2))
    return d[order].astype(np.int64)


def neighbour_cov(points, radius=10, max_nn=20):
    """-> (C int64 [N,6] as c00 c01 c02 c11 c12 c22, K int64 [N]) per input point"""
    pts = np.asarray(points, np.int64).reshape(-1, 3)
    res = int(pts.max()) + 1
    key = (pts[:, 0] * res + pts[:, 1]) * res + pts[:, 2]
    keys, inv = np.unique(key, return_inverse=True)
    cells = np.stack([keys // (res * res), (keys // res) % res, keys % res], -1)
    n = len(keys)
    K = np.zeros(n, np.int64)
    S = np.zeros((n, 3), np.int64)
    Q = np.zeros((n, 6), np.int64)
    active = np.arange(n)
    for d in offset_table(radius):
        if active.size == 0:
            break
        q = cells[active] + d
        inb = np.all((q >= 0) & (q < res), 1)
        kq = (q[:, 0] * res + q[:, 1]) * res + q[:, 2]
        pos = np.minimum(np.searchsorted(keys, kq), n - 1)
        idx = active[inb & (keys[pos] == kq)]
        K[idx] += 1
        S[idx] += d
        Q[idx] += np.array([d[0] * d[0], d[0] * d[1], d[0] * d[2], d[1] * d[1], d[1] * d[2], d[2] * d[2]])
        active = active[K[active] < max_nn]
    C = K[:, None] * Q - np.stack([S[:, 0] * S[:, 0], S[:, 0] * S[:, 1], S[:, 0] * S[:, 2], S[:, 1] * S[:, 1],
                                   S[:, 1] * S[:, 2], S[:, 2] * S[:, 2]], -1)
    inv = inv.reshape(-1)
    return C[inv], K[inv]


def full(c6):
    c = np.asarray(c6)
    return np.stack([np.stack([c[..., 0], c[..., 1], c[..., 2]], -1), np.stack([c[..., 1], c[..., 3], c[..., 4]], -1),
                     np.stack([c[..., 2], c[..., 4], c[..., 5]], -1)], -2)


def _sign(n):
    """flip each row so that its first component with |c| > 1e-6 is positive"""
    big = np.abs(n) > 1e-6
    first = np.argmax(big, axis=1)
    lead = n[np.arange(len(n)), first]
    flip = big.any(1) & (lead < 0)
    return np.where(flip[:, None], -n, n)


def normals_from_cov(C6, K):
    """-> (normals float64 [N,3], eigenvalues float64 [N,3] ascending, kind [N]: 0 eigenvector, 1 K < 3, 2 collinear)"""
    C = full(C6)
    K = np.asarray(K)
    n = len(K)
    lam, V = np.linalg.eigh(C.astype(np.float64)) if n else (np.zeros((0, 3)), np.zeros((0, 3, 3)))
    out = V[:, :, 0].copy()
    rank1 = np.ones(n, bool)                                  # every 2x2 minor zero (exact, int64)
    for r0, r1 in ((0, 1), (0, 2), (1, 2)):
        for c0, c1 in ((0, 1), (0, 2), (1, 2)):
            rank1 &= C[:, r0, c0] * C[:, r1, c1] - C[:, r0, c1] * C[:, r1, c0] == 0
    kind = np.where(K < 3, 1, np.where(rank1, 2, 0))
    line = kind == 2
    if line.any():
        Cl = C[line]
        r = np.argmax(np.stack([Cl[:, 0, 0], Cl[:, 1, 1], Cl[:, 2, 2]], 1), axis=1)         # first maximum
        u = Cl[np.arange(len(Cl)), r].astype(np.float64)
        j = np.argmin(np.abs(u), axis=1)                                                  # first minimum
        out[line] = np.cross(u, np.eye(3)[j])
    out = out / np.sqrt((out[:, 0] * out[:, 0] + out[:, 1] * out[:, 1]) + out[:, 2] * out[:, 2])[:, None]
    out = _sign(out)
    out[kind == 1] = (0.0, 0.0, 1.0)
    return out, lam, kind


# ---------------------------------------------------------------------------------------------------------- meshes
def icosphere(level=2, radius=1.0):
    p = (1 + 5 ** 0.5) / 2
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p),
         (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(level):
        cache, nf = {}, []

        def mid(a, b):
            k = (min(a, b), max(a, b))
            if k not in cache:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                cache[k] = len(v) - 1
            return cache[k]
        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v) * radius, np.array(f, np.int32)


def box(size=(2.0, 1.0, 0.5)):
    sx, sy, sz = size
    v = np.array([(x, y, z) for x in (0, sx) for y in (0, sy) for z in (0, sz)], np.float64)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    t = [(q[0], q[i], q[i + 1]) for q in quads for i in (1, 2)]
    return v, np.array(t, np.int32)


def torus(R=3.0, r=1.0, nu=48, nv=24):
    u, w = np.meshgrid(np.arange(nu) * 2 * np.pi / nu, np.arange(nv) * 2 * np.pi / nv, indexing="ij")
    v = np.stack([(R + r * np.cos(w)) * np.cos(u), (R + r * np.cos(w)) * np.sin(u), r * np.sin(w)], -1).reshape(-1, 3)
    idx = np.arange(nu * nv).reshape(nu, nv)
    a, b = idx, np.roll(idx, -1, 0)
    c, d = np.roll(b, -1, 1), np.roll(a, -1, 1)
    t = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])
    return v, t.astype(np.int32)


def quad_soup(seed=5):
    """random quads split in two, with zero-area triangles (repeated and collinear corners) and duplicated triangles,
    a zero-area one last"""
    rng = np.random.default_rng(seed)
    v = rng.uniform(-4, 4, (40, 3))
    t = [(4 * i, 4 * i + 1, 4 * i + 2) for i in range(10)] + [(4 * i, 4 * i + 2, 4 * i + 3) for i in range(10)]
    v = np.concatenate([v, [[0, 0, 0], [1, 1, 1], [2, 2, 2]]])
    t += [(0, 0, 1), (40, 41, 42), (3, 5, 5)] + t[:5] + [(40, 41, 42)]
    return v, np.array(t, np.int32)
