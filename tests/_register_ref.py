"""The registration rule (include/pcgc.h, pcgc_register_*; pcgcv1_amd/register.py) in numpy: one ICP step by
brute force over all pairs with exactly rounded sums, the two solves, the coarse-to-fine loop, and the seeded surface the
tests share.  Small clouds only."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _offgrid_ref import TIE                                             # noqa: E402

N_SUMS = 45
MIN_PAIRS = {"point": 3, "plane": 6}
COND_LIMIT = 1e12


# ---------------------------------------------------------------------------- one step
def transform(points, R, t):
    """float32 [n,3]: float32(((R[r,0] x + R[r,1] y) + R[r,2] z) + t[r]) in float64, one operation at a time"""
    p = np.asarray(points, np.float32).astype(np.float64)
    R, t = np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)
    out = np.empty(p.shape, np.float32)
    for r in range(3):
        out[:, r] = (((R[r, 0] * p[:, 0] + R[r, 1] * p[:, 1]) + R[r, 2] * p[:, 2]) + t[r]).astype(np.float32)
    return out


def _pair_terms(a, b, n, w):
    """the terms of sums 2..44 for pairs (a, b float64 [k,3], n float64 [k,3] or None, w [k]) -> list of 43 arrays [k]"""
    terms = [w * a[:, r] for r in range(3)] + [w * b[:, r] for r in range(3)]
    terms += [(w * a[:, r]) * b[:, c] for r in range(3) for c in range(3)]
    if n is None:
        return terms + [np.zeros(0)] * 28
    d = a - b
    res = (d[:, 0] * n[:, 0] + d[:, 1] * n[:, 1]) + d[:, 2] * n[:, 2]
    J = [a[:, 1] * n[:, 2] - a[:, 2] * n[:, 1], a[:, 2] * n[:, 0] - a[:, 0] * n[:, 2], a[:, 0] * n[:, 1] - a[:, 1] * n[:, 0],
         n[:, 0], n[:, 1], n[:, 2]]
    terms += [(w * J[r]) * J[c] for r in range(6) for c in range(r, 6)]
    terms += [(w * J[r]) * res for r in range(6)]
    return terms + [(w * res) * res]


def step(source, target, normals, R, t, c, max_dist, chunk=2048):
    """One step -> dict: S float64 [45] (every sum exactly rounded, math.fsum), abs [45] = the sum of |term|, terms [45] = the
    number of terms, best float64 [n], ties int32 [n] (0 outside the gate).  Brute force over all pairs, in row chunks."""
    moved = transform(source, R, t).astype(np.float64)
    q = np.asarray(target, np.float32).astype(np.float64)
    nq = None if normals is None else np.asarray(normals, np.float32).astype(np.float64)
    c = np.asarray(c, np.float64).reshape(3)
    gate2 = float(max_dist) * float(max_dist)
    best, ties = np.empty(len(moved)), np.zeros(len(moved), np.int32)
    parts = [[] for _ in range(N_SUMS)]
    for i0 in range(0, len(moved), chunk):
        p = moved[i0:i0 + chunk]
        dx, dy, dz = (p[:, None, k] - q[None, :, k] for k in range(3))
        d2 = (dx * dx + dy * dy) + dz * dz
        bst = d2.min(1)
        best[i0:i0 + chunk] = bst
        used = bst <= gate2
        tie = (np.abs(d2 - bst[:, None]) < TIE) & used[:, None]
        cnt = tie.sum(1)
        ties[i0:i0 + chunk] = cnt
        rows, cols = np.nonzero(tie)
        parts[1].append(bst[used])
        w = 1.0 / cnt[rows].astype(np.float64)
        for k, v in enumerate(_pair_terms(p[rows] - c, q[cols] - c, None if nq is None else nq[cols], w)):
            parts[2 + k].append(v)
    S, absum, count = np.zeros(N_SUMS), np.zeros(N_SUMS), np.zeros(N_SUMS, np.int64)
    n_used = int((ties > 0).sum())
    S[0], absum[0], count[0] = n_used, n_used, n_used
    for k in range(1, N_SUMS):
        v = np.concatenate(parts[k]) if parts[k] else np.zeros(0)
        S[k], absum[k], count[k] = math.fsum(v.tolist()), math.fsum(np.abs(v).tolist()), len(v)
    return {"S": S, "abs": absum, "terms": count, "best": best, "ties": ties}


def bound(ref_step):
    """per sum, the most any order of float64 additions can differ from the exact sum, doubled: 2 (terms - 1) 2^-53 sum |term|"""
    return 2.0 * np.maximum(ref_step["terms"] - 1, 0) * 2.0 ** -53 * ref_step["abs"]


# ---------------------------------------------------------------------------- the solves
def rodrigues(v):
    """the exact rotation about v by |v|"""
    v = np.asarray(v, np.float64)
    theta = float(np.linalg.norm(v))
    if theta == 0.0:
        return np.eye(3)
    k = v / theta
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(theta) * K + (1.0 - math.cos(theta)) * (K @ K)


def solve_point(S):
    n = S[0]
    mu_a, mu_b = S[2:5] / n, S[5:8] / n
    H = S[8:17].reshape(3, 3) - n * np.outer(mu_a, mu_b)
    U, _, Vt = np.linalg.svd(H)
    d = np.sign(np.linalg.det(Vt.T @ U.T))
    dR = Vt.T @ np.diag([1.0, 1.0, d]) @ U.T
    return dR, mu_b - dR @ mu_a


def plane_system(S):
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = S[17:38]
    return A + np.triu(A, 1).T, -S[38:44]


def solve_plane(S):
    A, g = plane_system(S)
    if not np.isfinite(A).all() or np.linalg.cond(A) > COND_LIMIT:
        raise ValueError("degenerate")
    x = np.linalg.solve(A, g)
    return rodrigues(x[:3]), x[3:]


def compose(R, t, c, dR, dt):
    return dR @ R, dR @ (t - c) + dt + c


def angle(dR):
    v = np.array([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]])
    return math.atan2(float(np.linalg.norm(v)) / 2.0, (float(np.trace(dR)) - 1.0) / 2.0)


# ---------------------------------------------------------------------------- the loop
def icp(source, target, normals=None, metric="plane", max_dist=(4.0, 2.0, 1.0), iters=50, tol=1e-3, init=None):
    """-> dict(R, t, iterations [per stage], converged, n_used, fitness, rmse, plane_rmse | None)"""
    q = np.asarray(target, np.float32).astype(np.float64)
    lo, hi = q.min(0), q.max(0)
    c = np.rint((lo + hi) / 2.0)
    rho = float(np.linalg.norm(hi - lo)) / 2.0
    R, t = (np.eye(3), np.zeros(3)) if init is None else (np.array(init[0], np.float64), np.array(init[1], np.float64))
    nrm = normals if metric == "plane" else None
    iterations, converged = [], True
    for gate in max_dist:
        done = False
        k = 0
        while k < iters and not done:
            S = step(source, target, nrm, R, t, c, gate)["S"]
            if S[0] < MIN_PAIRS[metric]:
                raise ValueError("too few pairs")
            dR, dt = solve_plane(S) if metric == "plane" else solve_point(S)
            R, t = compose(R, t, c, dR, dt)
            k += 1
            done = angle(dR) * rho + float(np.linalg.norm(dt)) < tol
        iterations.append(k)
        converged = converged and done
    S = step(source, target, nrm, R, t, c, max_dist[-1])["S"]
    n_used = int(S[0])
    return {"R": R, "t": t, "iterations": iterations, "converged": converged, "n_used": n_used, "fitness": n_used / len(source),
            "rmse": math.sqrt(S[1] / n_used) if n_used else float("nan"),
            "plane_rmse": math.sqrt(S[44] / n_used) if metric == "plane" and n_used else None}


# ---------------------------------------------------------------------------- the surface
CENTRE = np.array([16.0, 16.0, 16.0])
RADII = np.array([10.0, 8.5, 7.0])


def _bump(u):
    """radius factor per unit direction u [n,3]: smooth, no rotational or mirror symmetry"""
    return (1.0 + 0.07 * np.sin(3.0 * u[:, 0] + 0.5) * np.cos(2.0 * u[:, 1] - 0.3) + 0.06 * np.sin(4.0 * u[:, 2] + 2.0 * u[:, 0] + 1.1)
            + 0.05 * np.cos(5.0 * u[:, 1] + 3.0 * u[:, 2] - 0.7))


def _implicit(x):
    """zero on the surface, growing outwards"""
    y = (x - CENTRE) / RADII
    r = np.linalg.norm(y, axis=1)
    return r - _bump(y / r[:, None])


def surface(seed, n):
    """-> (points float64 [n,3] on a bumpy ellipsoid of radius about 10 in a 32-cell box, unit outward normals float64 [n,3])"""
    rng = np.random.default_rng(seed)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    x = CENTRE + RADII * u * _bump(u)[:, None]
    g = np.stack([(_implicit(x + e) - _implicit(x - e)) / 2e-5 for e in np.eye(3) * 1e-5], 1)
    return x, g / np.linalg.norm(g, axis=1, keepdims=True)


def known_pose():
    """5 degrees about (1, 2, 3) through the centre, then (1, -0.75, 0.5) -> (R, t) with x' = R x + t"""
    axis = np.array([1.0, 2.0, 3.0]) / math.sqrt(14.0)
    R = rodrigues(axis * math.radians(5.0))
    return R, CENTRE - R @ CENTRE + np.array([1.0, -0.75, 0.5])


def overlap_pair(n=2500, seeds=(101, 202)):
    """Two independent samplings of the surface; the source lacks the low quarter in x, the target the high quarter, and the
    source is moved by known_pose().  -> dict(source float32, source_true float64 (where each source point belongs), target
    float32, target_normals float32)"""
    (a, _), (b, nb) = surface(seeds[0], n), surface(seeds[1], n)
    lo, hi = CENTRE[0] - RADII[0], CENTRE[0] + RADII[0]
    a = a[a[:, 0] > lo + 0.25 * (hi - lo)]
    keep = b[:, 0] < hi - 0.25 * (hi - lo)
    R, t = known_pose()
    src = (a @ R.T + t).astype(np.float32)
    return {"source": src, "source_true": a, "target": b[keep].astype(np.float32), "target_normals": nb[keep].astype(np.float32)}


def three_scans(n=2500, seeds=(341, 342, 343), unit=0.01):
    """Three samplings in slabs along x, 0 .. 45 %, 25 .. 75 % and 55 .. 100 % of the extent: scan 2 overlaps scan 1 and not
    scan 0.  Scans 1 and 2 are moved by small poses of their own, and all coordinates are in scanner units of `unit` per
    voxel.  -> list of (points float64, colors uint8, None), and the poses [(R, t)] that moved them, in voxels.
    The seeds are ones with which every stage of both registrations ends by the stopping rule on voxels of unit / 2 when
    the target's normals are estimated on its voxels: with such normals, of ten seed triples tried about half had a stage
    that ended in a cycle of two poses a few 0.001 voxel apart instead, which the rule reports as not converged (DESIGN.md
    §7h).  At that voxel size most voxels hold one point, so few of them have a point within 1e-3 of a face."""
    lo, ext = CENTRE[0] - RADII[0] * 1.2, 2.4 * RADII[0]
    slabs = ((0.0, 0.45), (0.25, 0.75), (0.55, 1.0))
    Rk, tk = known_pose()
    half = rodrigues(np.array([0.02, -0.03, 0.025]))
    poses = [(np.eye(3), np.zeros(3)), (Rk, tk), (half, CENTRE - half @ CENTRE + np.array([-0.6, 0.5, 0.8]))]
    scans = []
    for seed, (s0, s1), (R, t) in zip(seeds, slabs, poses):
        x, _ = surface(seed, n)
        x = x[(x[:, 0] >= lo + s0 * ext) & (x[:, 0] <= lo + s1 * ext)]
        col = np.clip(np.rint((x - CENTRE) * 8.0 + 128.0), 0, 255).astype(np.uint8)
        scans.append(((x @ R.T + t) * unit, col, None))
    return scans, poses
