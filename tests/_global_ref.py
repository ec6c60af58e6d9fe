"""The global-alignment rule (include/pcgc.h, pcgc_feature_* and pcgc_ransac_score; pcgcv1_amd/register.py) in
numpy: keypoints, the sign-invariant integer descriptor by brute force over all pairs, the nearest descriptor, the inlier
count of a pose, the seeded draws with their batched Kabsch solve, and the five-sphere fixture the tests share.  All position
arithmetic is float64, one numpy operation per step in the stated order.  Small clouds only.  Not collected by pytest."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ingest_ref as iref                                               # noqa: E402
from _register_ref import rodrigues, transform                           # noqa: E402

BINS = 11
N_BINS = 3 * BINS            # 33 counters per keypoint
ROW = 36                     # bytes of a descriptor row: 33 bins and three zero bytes
DRAW_BATCH = 16384           # triples per call of the generator: part of the rule, the stream depends on it
EDGE_RATIO = 0.9


# ---------------------------------------------------------------------------- keypoints
def unit_normals(normals):
    """register._unit_normals: normalised in float64, a non-finite or zero normal becomes 0 -> float32"""
    v = np.asarray(normals, np.float64).reshape(-1, 3)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        u = v / np.linalg.norm(v, axis=1, keepdims=True)
    u[~np.isfinite(u).all(1)] = 0.0
    return u.astype(np.float32)


def keypoints(points, normals, feature_voxel):
    """points float32 [n,3] in grid units, normals [n,3] -> (kp float32 [m,3], unit normals float32 [m,3]): one keypoint per
    occupied cell of edge feature_voxel (ingest's frame, quantise and merge), at the cell's position, rows in ascending key"""
    p = np.asarray(points, np.float32).astype(np.float64).reshape(-1, 3)
    origin, step, bits = iref.fit_frame(p, voxel_size=feature_voxel)
    _, keys = iref.quantize(p, origin, step, bits)
    vox, _, _, nrm = iref.merge(keys, bits, None, np.asarray(normals, np.float32).reshape(-1, 3))
    return iref.apply_frame(vox, origin, step).astype(np.float32), unit_normals(nrm)


# ---------------------------------------------------------------------------- 1, 2: the descriptor
def _usable(normals):
    n = np.asarray(normals, np.float32).reshape(-1, 3)
    return np.isfinite(n).all(1) & (n != 0).any(1)


def _bin(f):
    x = f * 11.0
    return np.where(x < 10.0, np.floor(np.where(x < 10.0, x, 0.0)), 10.0).astype(np.int64)


def neighbours(kp, normals, r, chunk=256):
    """-> (rows, cols) of every ordered pair i, j with 0 < d2 <= r * r and both normals usable, and per pair (dx, dy, dz, d2)
    with d = p_i - p_j.  Brute force over all pairs of rows whose x lie within r + 1 of each other (the rest are further than r
    apart whatever the rounding), in chunks of rows taken in the order of x."""
    p = np.asarray(kp, np.float32).astype(np.float64)
    ok = _usable(normals)
    r2 = float(r) * float(r)
    with np.errstate(invalid="ignore"):
        order = np.argsort(np.where(np.isfinite(p[:, 0]), p[:, 0], np.inf), kind="stable")
    xs = p[order, 0]
    out = []
    for i0 in range(0, len(p), chunk):
        rows_i = order[i0:i0 + chunk]
        a = p[rows_i]
        c0, c1 = np.searchsorted(xs, a[0, 0] - (r + 1.0), "left"), np.searchsorted(xs, a[-1, 0] + (r + 1.0), "right")
        if not np.isfinite(a[:, 0]).all():
            c0, c1 = 0, len(p)
        cols_i = order[c0:c1]
        q = p[cols_i]
        with np.errstate(invalid="ignore", over="ignore"):
            dx, dy, dz = (a[:, None, k] - q[None, :, k] for k in range(3))
            d2 = (dx * dx + dy * dy) + dz * dz
            rows, cols = np.nonzero((d2 > 0) & (d2 <= r2) & ok[rows_i, None] & ok[None, cols_i])
        out.append((rows_i[rows], cols_i[cols], dx[rows, cols], dy[rows, cols], dz[rows, cols], d2[rows, cols]))
    return tuple(np.concatenate([o[k] for o in out]) for k in range(6))


def pairs(kp, normals, r, nb=None):
    """-> (S uint32 [n,33], k int32 [n]); nb: neighbours(kp, normals, r) when the caller has it"""
    n = len(kp)
    nrm = np.asarray(normals, np.float32).astype(np.float64).reshape(-1, 3)
    rows, cols, dx, dy, dz, d2 = neighbours(kp, normals, r) if nb is None else nb
    length = np.sqrt(d2)
    ux, uy, uz = dx / length, dy / length, dz / length
    ni, nj = nrm[rows], nrm[cols]
    f1 = np.abs((ni[:, 0] * ux + ni[:, 1] * uy) + ni[:, 2] * uz)
    f2 = np.abs((nj[:, 0] * ux + nj[:, 1] * uy) + nj[:, 2] * uz)
    f3 = np.abs((ni[:, 0] * nj[:, 0] + ni[:, 1] * nj[:, 1]) + ni[:, 2] * nj[:, 2])
    S = np.zeros(n * N_BINS, np.int64)
    for block, f in enumerate((f1, f2, f3)):
        S += np.bincount(rows * N_BINS + block * BINS + _bin(f), minlength=n * N_BINS)
    return S.reshape(n, N_BINS).astype(np.uint32), np.bincount(rows, minlength=n).astype(np.int32)


def combine(kp, normals, r, S, k, nb=None):
    """-> (feat uint8 [n,36], valid bool [n])"""
    n = len(kp)
    rows, cols = (neighbours(kp, normals, r) if nb is None else nb)[:2]
    S64, k64 = np.asarray(S).astype(np.uint64), np.asarray(k).astype(np.uint64)
    # the sums over the neighbours through bincount in float64: every one is an integer below 2^53 for clouds this small
    Sf, kf = np.asarray(S).astype(np.float64), np.asarray(k).astype(np.float64)
    assert len(rows) * max(1.0, float(Sf.max(initial=0.0)), float(kf.max(initial=0.0))) < 2.0 ** 53
    G = k64[:, None] * S64 + np.stack([np.bincount(rows, weights=Sf[cols, b], minlength=n) for b in range(N_BINS)], 1).astype(np.uint64)
    T = k64 * k64 + np.bincount(rows, weights=kf[cols], minlength=n).astype(np.uint64)
    valid = T > 0
    Ts = np.where(valid, T, np.uint64(1))[:, None]
    feat = np.zeros((n, ROW), np.uint8)
    feat[:, :N_BINS] = np.where(valid[:, None], (G * np.uint64(255) + Ts // np.uint64(2)) // Ts, np.uint64(0)).astype(np.uint8)
    return feat, valid


def features(kp, normals, r, detail=False):
    nb = neighbours(kp, normals, r)
    S, k = pairs(kp, normals, r, nb)
    feat, valid = combine(kp, normals, r, S, k, nb)
    return (feat, valid, S, k) if detail else (feat, valid)


# ---------------------------------------------------------------------------- 3: the nearest descriptor
def match(fs, vs, ft, vt, chunk=1024):
    """-> (j int32 [n], dist uint32 [n]): per valid source row the valid target row with the smallest sum of squared byte
    differences over the 33 bins, the lowest index among equals; -1 and 0xFFFFFFFF for an invalid row or without a valid target"""
    a = np.asarray(fs, np.uint8)[:, :N_BINS].astype(np.float64)          # every figure below 2^22: float64 holds it exactly
    b = np.asarray(ft, np.uint8)[:, :N_BINS].astype(np.float64)
    vs, vt = np.asarray(vs).astype(bool), np.asarray(vt).astype(bool)
    j, dist = np.full(len(a), -1, np.int32), np.full(len(a), 0xFFFFFFFF, np.uint32)
    cand = np.nonzero(vt)[0]
    if not len(cand):
        return j, dist
    bc = b[cand]
    nb = (bc * bc).sum(1)
    for i0 in range(0, len(a), chunk):
        ac = a[i0:i0 + chunk]
        d = ((ac * ac).sum(1)[:, None] + nb[None, :]) - 2.0 * (ac @ bc.T)
        best = d.argmin(1)                                   # the first of equals, and cand ascends
        use = vs[i0:i0 + chunk]
        j[i0:i0 + chunk][use] = cand[best][use]
        dist[i0:i0 + chunk][use] = d[np.arange(len(best)), best][use].astype(np.uint32)
    return j, dist


# ---------------------------------------------------------------------------- 4: the inlier count
def inlier_mask(pose, P, Q, dist):
    """pose = 12 doubles, R row-major then t -> bool [C]: d2(p', q) <= dist * dist with p' the moved point in float32"""
    pose = np.asarray(pose, np.float64).reshape(12)
    with np.errstate(invalid="ignore", over="ignore"):
        moved = transform(P, pose[:9].reshape(3, 3), pose[9:]).astype(np.float64)
        q = np.asarray(Q, np.float32).astype(np.float64)
        dx, dy, dz = (moved[:, k] - q[:, k] for k in range(3))
        return ((dx * dx + dy * dy) + dz * dz) <= float(dist) * float(dist)


def score(poses, P, Q, dist):
    """-> int32 [K]"""
    return np.array([int(inlier_mask(pose, P, Q, dist).sum()) for pose in np.asarray(poses, np.float64).reshape(-1, 12)], np.int32)


# ---------------------------------------------------------------------------- the draws and their solve (host rule)
def draw_triples(rng, n_corr, count):
    return rng.integers(0, n_corr, size=(count, 3))


def _edges(x, tri):
    """float64 [K,3]: the lengths of the edges 0-1, 1-2, 2-0 of the triangles tri [K,3] of the points x"""
    a = np.asarray(x, np.float32).astype(np.float64)[tri]
    d = a - a[:, (1, 2, 0), :]
    return np.sqrt((d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2])


def keep_triples(tri, P, Q, min_edge):
    """bool [K]: distinct indices, every source edge >= min_edge, every source edge and its target edge within 0.9 of each other"""
    distinct = (tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 2] != tri[:, 0])
    es, et = _edges(P, tri), _edges(Q, tri)
    return distinct & (es >= float(min_edge)).all(1) & (et >= EDGE_RATIO * es).all(1) & (es >= EDGE_RATIO * et).all(1)


def kabsch(a, b):
    """a, b float64 [K,M,3] -> (R [K,3,3], t [K,3]) with b ~ R a + t: solve_point's rule, batched"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    m = float(a.shape[1])
    mu_a, mu_b = a.sum(1) / m, b.sum(1) / m
    H = np.einsum("kmi,kmj->kij", a - mu_a[:, None, :], b - mu_b[:, None, :])
    U, _, Vt = np.linalg.svd(H)
    V, Ut = np.swapaxes(Vt, 1, 2), np.swapaxes(U, 1, 2)
    d = np.sign(np.linalg.det(V @ Ut))
    D = np.zeros_like(H)
    D[:, 0, 0] = D[:, 1, 1] = 1.0
    D[:, 2, 2] = d
    R = V @ D @ Ut
    return R, mu_b - np.einsum("kij,kj->ki", R, mu_a)


def hypotheses(P, Q, min_edge, draws, seed):
    """-> (poses float64 [K,12], draw int64 [K]): the kept triples' finite poses in draw order"""
    rng = np.random.default_rng(seed)
    P64, Q64 = np.asarray(P, np.float32).astype(np.float64), np.asarray(Q, np.float32).astype(np.float64)
    poses, index = [], []
    for d0 in range(0, int(draws), DRAW_BATCH):
        tri = draw_triples(rng, len(P), min(DRAW_BATCH, int(draws) - d0))
        kept = np.nonzero(keep_triples(tri, P, Q, min_edge))[0]
        if not len(kept):
            continue
        R, t = kabsch(P64[tri[kept]], Q64[tri[kept]])
        pose = np.concatenate([R.reshape(-1, 9), t], 1)
        fine = np.isfinite(pose).all(1)
        poses.append(pose[fine])
        index.append(kept[fine] + d0)
    if not poses:
        return np.zeros((0, 12)), np.zeros(0, np.int64)
    return np.concatenate(poses), np.concatenate(index)


def correspondences(src_kp, src_feat, src_valid, tgt_kp, tgt_feat, tgt_valid):
    """-> (P float32 [C,3], Q float32 [C,3], source rows int64 [C], target rows int64 [C])"""
    j, _ = match(src_feat, src_valid, tgt_feat, tgt_valid)
    rows = np.nonzero(j >= 0)[0]
    return np.asarray(src_kp, np.float32)[rows], np.asarray(tgt_kp, np.float32)[j[rows]], rows, j[rows].astype(np.int64)


def ransac(P, Q, corr_dist, min_edge, draws, seed, min_inliers, score_fn=score, detail=False):
    """the host rule of register.global_align on correspondences P -> Q"""
    if len(P) < 3:
        raise ValueError("fewer than 3 valid correspondences")
    poses, draw = hypotheses(P, Q, min_edge, draws, seed)
    if not len(poses):
        raise ValueError("no triple kept")
    counts = score_fn(poses, P, Q, corr_dist)
    w = int(np.argmax(counts))                               # the first of equals: the lowest draw
    inl = inlier_mask(poses[w], P, Q, corr_dist)
    P64, Q64 = np.asarray(P, np.float32).astype(np.float64), np.asarray(Q, np.float32).astype(np.float64)
    R, t = kabsch(P64[inl][None], Q64[inl][None])
    refined = np.concatenate([R.reshape(9), t.reshape(3)])
    n_in = int(score_fn(refined[None], P, Q, corr_dist)[0]) if np.isfinite(refined).all() else 0
    if n_in < min_inliers:
        raise ValueError("a winner below min_inliers")
    out = {"R": R[0], "t": t[0], "inliers": n_in, "correspondences": len(P), "hypotheses": len(poses), "draw": int(draw[w]),
           "draws": int(draws), "raw_inliers": int(counts[w]), "raw_pose": poses[w]}
    if detail:
        out["poses"], out["counts"], out["pose_draws"] = poses, counts, draw
    return out


def global_align(source, target, source_normals, target_normals, feature_voxel, radius, corr_dist, min_edge, draws=100000, seed=0,
                 min_inliers=20, detail=False):
    ks, ns = keypoints(source, source_normals, feature_voxel)
    kt, nt = keypoints(target, target_normals, feature_voxel)
    fs, vs, Ss, ksrc = features(ks, ns, radius, detail=True)
    ft, vt, St, ktgt = features(kt, nt, radius, detail=True)
    P, Q, rows, cols = correspondences(ks, fs, vs, kt, ft, vt)
    out = ransac(P, Q, corr_dist, min_edge, draws, seed, min_inliers, detail=detail)
    if detail:
        out.update(P=P, Q=Q, rows=rows, cols=cols, source_kp=ks, source_kp_normals=ns, target_kp=kt, target_kp_normals=nt,
                   source_feat=(fs, vs), target_feat=(ft, vt), source_pairs=(Ss, ksrc), target_pairs=(St, ktgt))
    return out


# ---------------------------------------------------------------------------- the fixture
CENTRES = np.array([[40.0, 40.0, 40.0], [54.0, 44.0, 38.0], [34.0, 54.0, 46.0], [42.0, 30.0, 52.0], [28.0, 34.0, 30.0]])
RADII = np.array([14.0, 8.0, 7.0, 6.0, 5.0])
FEATURE_VOXEL, RADIUS, CORR_DIST, MIN_EDGE, DRAWS, SEED, MIN_INLIERS = 0.125, 8.0, 2.0, 6.0, 100000, 0, 20
POSE_SEED = 1
FAR = 4.0                    # a hypothesis that leaves a source point further from its place is a wrong one


def spheres(seed, n=6000):
    """n points on the union of the five spheres (each sphere with probability ~ radius^2, uniform on it), those inside another
    sphere dropped -> (points float64 [m,3], outward unit normals with a random sign per point float64 [m,3])"""
    rng = np.random.default_rng(seed)
    m = 2 * n                                                # about three candidates in four survive: the first n of them
    which = rng.choice(len(RADII), size=m, p=RADII ** 2 / (RADII ** 2).sum())
    u = rng.normal(size=(m, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    x = CENTRES[which] + RADII[which, None] * u
    inside = np.zeros(m, bool)
    for c, r in zip(CENTRES, RADII):
        inside |= np.linalg.norm(x - c, axis=1) < r - 1e-9
    sign = rng.choice([-1.0, 1.0], size=m)
    keep = np.nonzero(~inside)[0][:n]
    return x[keep], (u * sign[:, None])[keep]


def fixture_pose(seed=POSE_SEED):
    """a turn of 84 .. 162 degrees about a random axis through the big sphere's centre, and up to 30 voxels per axis"""
    rng = np.random.default_rng(seed)
    axis = rng.normal(size=3)
    R = rodrigues(axis / np.linalg.norm(axis) * math.radians(rng.uniform(84.0, 162.0)))
    return R, CENTRES[0] - R @ CENTRES[0] + rng.uniform(-30.0, 30.0, size=3)


def fixture(pose_seed=POSE_SEED, seeds=(11, 22)):
    """-> dict(source float32, source_normals float32, source_true float64 (where each source point belongs), target float32,
    target_normals float32, R, t (source = R source_true + t))"""
    (a, na), (b, nb) = spheres(seeds[0]), spheres(seeds[1])
    lo = (CENTRES[:, 0] - RADII).min()
    hi = (CENTRES[:, 0] + RADII).max()
    keep_a, keep_b = a[:, 0] > lo + 0.25 * (hi - lo), b[:, 0] < hi - 0.25 * (hi - lo)
    a, na, b, nb = a[keep_a], na[keep_a], b[keep_b], nb[keep_b]
    R, t = fixture_pose(pose_seed)
    return {"source": (a @ R.T + t).astype(np.float32), "source_normals": (na @ R.T).astype(np.float32), "source_true": a,
            "target": b.astype(np.float32), "target_normals": nb.astype(np.float32), "R": R, "t": t}


def point_error(R, t, fx):
    """the largest distance of a source point under (R, t) from its true place"""
    return float(np.linalg.norm(fx["source"].astype(np.float64) @ np.asarray(R).T + np.asarray(t) - fx["source_true"], axis=1).max())


def fixture_align(fx=None, detail=True, **kw):
    fx = fixture() if fx is None else fx
    args = dict(feature_voxel=FEATURE_VOXEL, radius=RADIUS, corr_dist=CORR_DIST, min_edge=MIN_EDGE, draws=DRAWS, seed=SEED,
                min_inliers=MIN_INLIERS)
    args.update(kw)
    return global_align(fx["source"], fx["target"], fx["source_normals"], fx["target_normals"], detail=detail, **args)
