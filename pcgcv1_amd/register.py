"""Overlapping scans into one cloud: rigid registration (ICP, point-to-plane and point-to-point) on the GPU, then the merge
of pcgcv1_amd/ingest.py.

    python -m pcgcv1_amd.register --input a.ply b.ply c.ply --output merged_vox10.ply --bits 10     # or --voxel_size S
                                  [--metric plane|point] [--max_dist 4,2,1] [--iters 50] [--tol 1e-3] [--estimate_normals]
                                  [--init poses.json] [--clean SPEC] [--min_fitness 0.3]

writes the voxelised ply and merged_vox10.frame as pcgcv1_amd.ingest would for the union of the aligned scans, and
merged_vox10.poses.json: per input the 4x4 pose in the scan's own units and what the loop reports.

The rule (include/pcgc.h, pcgc_register_*; tests/_register_ref.py restates it in numpy).  ICP runs in grid
units, neighbouring surface points about 1 apart.  One step (csrc/offgrid.hip) moves the source by the trial pose, finds
every tied nearest neighbour in the target with the off-grid search, keeps the points within max_dist and reduces them to 45
float64 sums in a fixed order.  The solve is numpy float64 on the host: Kabsch for point-to-point, the 6x6 normal equations
with an exact Rodrigues rotation for point-to-plane.  max_dist is a coarse-to-fine schedule: with one wide gate the points
beyond the overlap pair with the target's rim and pull the pose.  A start further off than the first gate bridges is the
caller's job (init): there is no global alignment here.
"""
import argparse
import json
import math
import os

import numpy as np

from . import _lib

N_SUMS = 45
MIN_PAIRS = {"point": 3, "plane": 6}
COND_LIMIT = 1e12
DEFAULT_MAX_DIST = (4.0, 2.0, 1.0)


# ---------------------------------------------------------------------------- the solves (host, float64)
def rodrigues(v):
    """the exact rotation about v by |v| radians"""
    v = np.asarray(v, np.float64).reshape(3)
    theta = float(np.linalg.norm(v))
    if theta == 0.0:
        return np.eye(3)
    k = v / theta
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + math.sin(theta) * K + (1.0 - math.cos(theta)) * (K @ K)


def _check_pairs(S, metric, max_dist):
    if not S[0] >= MIN_PAIRS[metric]:
        raise ValueError("icp: nothing lies within max_dist = %g of the target (%d source points do, %s mode needs %d): give a "
                         "closer init or a wider first gate" % (max_dist, int(S[0]), metric, MIN_PAIRS[metric]))


def solve_point(S):
    """Kabsch on the sums of one step -> (dR, dt) about the centre"""
    S = np.asarray(S, np.float64)
    n = S[0]
    mu_a, mu_b = S[2:5] / n, S[5:8] / n
    H = S[8:17].reshape(3, 3) - n * np.outer(mu_a, mu_b)
    U, _, Vt = np.linalg.svd(H)
    d = np.sign(np.linalg.det(Vt.T @ U.T))
    dR = Vt.T @ np.diag([1.0, 1.0, d]) @ U.T
    return dR, mu_b - dR @ mu_a


def plane_system(S):
    """-> (A symmetric 6x6 from S[17:38], g = -S[38:44])"""
    S = np.asarray(S, np.float64)
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = S[17:38]
    return A + np.triu(A, 1).T, -S[38:44]


def solve_plane(S):
    """the point-to-plane normal equations A x = g -> (dR = the exact rotation of x[:3], dt = x[3:])"""
    A, g = plane_system(S)
    cond = np.linalg.cond(A) if np.isfinite(A).all() else float("inf")
    if not cond <= COND_LIMIT:
        raise ValueError("icp: the point-to-plane system is singular (condition %.3g): the matched surface does not fix all six "
                         "motions, as a plane, a sphere or too few pairs do not; use metric='point' or scans with more shape" % cond)
    x = np.linalg.solve(A, g)
    return rodrigues(x[:3]), x[3:]


def compose(R, t, c, dR, dt):
    """the step (dR, dt) about the centre c applied after the pose (R, t)"""
    return dR @ R, dR @ (t - c) + dt + c


def rotation_angle(dR):
    v = np.array([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]])
    return math.atan2(float(np.linalg.norm(v)) / 2.0, (float(np.trace(dR)) - 1.0) / 2.0)


def pose_matrix(R, t):
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)
    return M


def pose_to_scan_units(R, t, frame):
    """a pose between grid coordinates g = (p - origin) / step of `frame` -> the same motion of the scan's own p"""
    R = np.asarray(R, np.float64).reshape(3, 3)
    return R, frame.origin - R @ frame.origin + frame.step * np.asarray(t, np.float64).reshape(3)


def pose_from_scan_units(R, t, frame):
    R = np.asarray(R, np.float64).reshape(3, 3)
    return R, (np.asarray(t, np.float64).reshape(3) - frame.origin + R @ frame.origin) / frame.step


# ---------------------------------------------------------------------------- one step on the device
def _unit_normals(normals, n):
    """float32 [n,3]: normalised in float64, a non-finite or zero normal becomes 0"""
    v = np.asarray(normals, np.float64).reshape(-1, 3)
    if len(v) != n:
        raise ValueError("icp: %d target normals for %d target points" % (len(v), n))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        u = v / np.linalg.norm(v, axis=1, keepdims=True)
    u[~np.isfinite(u).all(1)] = 0.0
    return u.astype(np.float32)


def _float32_cloud(points, what):
    p = np.ascontiguousarray(np.asarray(points), np.float32).reshape(-1, 3)
    if not len(p):
        raise ValueError("icp: the %s cloud has no points" % what)
    return p


class Matcher(object):
    """A target cloud prepared once on the device (pcgc_register_prepare), and steps of a source cloud against it.
    source, target: float32 [n,3] / [m,3] in grid units; target_normals float [m,3] or None (point-to-point sums only)."""

    def __init__(self, source, target, target_normals=None):
        import torch
        from .metrics import _OffgridTarget
        dev = _lib.require_gpu()
        self.source = _float32_cloud(source, "source")
        target = _float32_cloud(target, "target")
        try:                       # the cells come from the target alone: the source moves, and the step itself refuses what no cell holds
            self.cells = _OffgridTarget(target, target, dev)
        except ValueError as e:
            raise ValueError(str(e).replace("pc_error_float", "icp"))
        self.n, self.m = len(self.source), len(target)
        self.source_d = torch.from_numpy(self.source).to(dev)
        self.order = None                                      # source_d[i] = source[order[i]] once sort_source has run
        self.normals_d = None
        if target_normals is not None:
            self.normals_d = torch.from_numpy(_unit_normals(target_normals, self.m)).to(dev)[self.cells.order].contiguous()
        t64 = target.astype(np.float64)
        self.lo, self.hi = t64.min(0), t64.max(0)
        lib = _lib.hip()
        self.ws = torch.empty(int(lib.pcgc_register_workspace_bytes(self.cells.res, self.m)), dtype=torch.uint8, device=dev)
        self.out = torch.empty(N_SUMS, dtype=torch.float64, device=dev)
        _lib.check(lib.pcgc_register_prepare(_lib.dptr(self.cells.points), self.m, *self.cells.grid(), _lib.dptr(self.ws),
                                             self.ws.numel(), _lib.stream()), "pcgc_register_prepare")

    def sort_source(self, R, t):
        """Reorder the source by the cell each point starts in under the pose (R, t): a wave's lanes then walk neighbouring
        cells (one step at 1 M points: 11.6 -> 6.6 ms, profiles/register_bench.txt).  Only the order of the sums changes,
        so their last bits; per-point outputs keep the caller's order."""
        import torch
        dev = self.source_d.device
        moved = self.source_d.to(torch.float64) @ torch.from_numpy(np.asarray(R, np.float64).reshape(3, 3).T.copy()).to(dev)
        moved += torch.from_numpy(np.asarray(t, np.float64).reshape(3)).to(dev)
        cell = torch.floor(torch.nan_to_num(moved, nan=0.0) / self.cells.h) - torch.tensor(self.cells.origin, dtype=torch.float64, device=dev)
        cell = cell.clamp_(0, self.cells.res - 1).to(torch.int64)
        order = torch.sort((cell[:, 0] * self.cells.res + cell[:, 1]) * self.cells.res + cell[:, 2], stable=True)[1]
        self.source_d = self.source_d[order].contiguous()
        self.order = order if self.order is None else self.order[order]

    @property
    def centre(self):
        return np.rint((self.lo + self.hi) / 2.0)

    @property
    def radius(self):
        return float(np.linalg.norm(self.hi - self.lo)) / 2.0

    def step(self, R, t, c, max_dist, with_normals=True, per_point=False):
        """-> S float64 [45]; per_point=True: (S, best float64 [n], ties int32 [n]).  RuntimeError when a moved coordinate
        is a NaN or out of every cell's reach."""
        import torch
        R9 = np.ascontiguousarray(np.asarray(R, np.float64).reshape(9))
        t3 = np.ascontiguousarray(np.asarray(t, np.float64).reshape(3))
        c3 = np.ascontiguousarray(np.asarray(c, np.float64).reshape(3))
        dev = self.source_d.device
        best = torch.empty(self.n, dtype=torch.float64, device=dev) if per_point else None
        ties = torch.empty(self.n, dtype=torch.int32, device=dev) if per_point else None
        _lib.check(_lib.hip().pcgc_register_step(
            _lib.dptr(self.source_d), self.n, _lib.dptr(self.cells.points), self.m, _lib.dptr(self.normals_d if with_normals else None),
            *self.cells.grid(), _lib.nptr(R9), _lib.nptr(t3), _lib.nptr(c3), float(max_dist), _lib.dptr(self.out), _lib.dptr(best),
            _lib.dptr(ties), _lib.dptr(self.ws), self.ws.numel(), _lib.stream()), "pcgc_register_step")
        S = self.out.cpu().numpy().copy()
        if np.isnan(S).any():
            raise RuntimeError("pcgc_register_step: a moved source coordinate is not finite or leaves every cell's reach, or the "
                               "target breaks the cell rule (include/pcgc.h)")
        if per_point:
            if self.order is not None:
                best, ties = torch.empty_like(best).index_copy_(0, self.order, best), torch.empty_like(ties).index_copy_(0, self.order, ties)
            return S, best.cpu().numpy(), ties.cpu().numpy()
        return S


# ---------------------------------------------------------------------------- the loop
def _schedule(max_dist):
    gates = [float(g) for g in (max_dist if isinstance(max_dist, (tuple, list, np.ndarray)) else (max_dist,))]
    if not gates or not all(np.isfinite(g) and g > 0 for g in gates):
        raise ValueError("icp: max_dist must be positive distances in grid units (got %r)" % (max_dist,))
    return gates


def check_arguments(metric, have_normals, estimate_normals=False, iters=50, tol=1e-3):
    """the argument errors of icp / register_scans, before any work"""
    if metric not in MIN_PAIRS:
        raise ValueError("icp: metric must be 'plane' or 'point' (got %r)" % (metric,))
    if metric == "plane" and not have_normals and not estimate_normals:
        raise ValueError("icp: metric='plane' needs the target's normals: give them, estimate them (estimate_normals / "
                         "--estimate_normals), or use metric='point'")
    if int(iters) < 1 or not (np.isfinite(tol) and tol > 0):
        raise ValueError("icp: iters must be at least 1 and tol positive (got %r, %r)" % (iters, tol))


def icp(source, target, target_normals=None, metric="plane", max_dist=DEFAULT_MAX_DIST, iters=50, tol=1e-3, init=None):
    """Align `source` to `target` (float32 [n,3] / [m,3], grid units) from the pose init = (R, t), identity when None ->
    dict: R, t (target ~ R source + t), iterations (per stage), converged, n_used, fitness = n_used / n, rmse =
    sqrt(sum of best / n_used), plane_rmse (plane mode, else None).  Each entry of max_dist is a stage of at most `iters`
    steps that ends when the last step moved no point of the target's bounding box by `tol`; one more step at the final
    pose gives the figures.  ValueError: nothing within max_dist, or a singular point-to-plane system."""
    check_arguments(metric, target_normals is not None, False, iters, tol)
    gates = _schedule(max_dist)
    plane = metric == "plane"
    m = Matcher(source, target, target_normals if plane else None)
    c, rho = m.centre, m.radius
    R, t = (np.eye(3), np.zeros(3)) if init is None else (np.array(init[0], np.float64).reshape(3, 3), np.array(init[1], np.float64).reshape(3))
    iterations, converged = [], True
    for gate in gates:
        k, done = 0, False
        m.sort_source(R, t)                                    # once per stage: the pose moves little within one
        while k < int(iters) and not done:
            S = m.step(R, t, c, gate, plane)
            _check_pairs(S, metric, gate)
            dR, dt = solve_plane(S) if plane else solve_point(S)
            R, t = compose(R, t, c, dR, dt)
            k += 1
            done = rotation_angle(dR) * rho + float(np.linalg.norm(dt)) < tol
        iterations.append(k)
        converged = converged and done
    S = m.step(R, t, c, gates[-1], plane)
    n_used = int(S[0])
    return {"R": R, "t": t, "iterations": iterations, "converged": converged, "n_used": n_used, "fitness": n_used / m.n,
            "rmse": math.sqrt(S[1] / n_used) if n_used else float("nan"),
            "plane_rmse": (math.sqrt(S[44] / n_used) if n_used else float("nan")) if plane else None}


# ---------------------------------------------------------------------------- several scans
def to_grid(points, frame):
    """g = (p - origin) / step in float64, then float32: the grid units ICP runs in (may leave [0, R])"""
    return ((np.asarray(points, np.float64).reshape(-1, 3) - frame.origin) / np.float64(frame.step)).astype(np.float32)


def estimated_target_normals(points, frame):
    """normals for a float cloud that has none: its voxels on `frame` (ingest's quantise and merge), metrics.estimate_normals
    on them, and every point takes its voxel's -> float32 [n,3]"""
    import torch
    from . import ingest, metrics
    _, keys = ingest.quantize(points, frame)
    vox, _, _, _, n_out = ingest.merge_device(keys, frame.bits)
    vox = vox[:int(n_out.item())]
    nrm = torch.from_numpy(metrics.estimate_normals(vox)).to(keys.device)
    res = 1 << frame.bits
    vox_keys = (vox[:, 0].long() * res + vox[:, 1].long()) * res + vox[:, 2].long()
    return nrm[torch.searchsorted(vox_keys, keys).clamp_(max=len(vox_keys) - 1)].cpu().numpy()


def _finite_scan(k, scan):
    points, colors, normals = (tuple(scan) + (None, None))[:3]
    p = np.asarray(points, np.float64).reshape(-1, 3)
    keep = np.isfinite(p).all(1)
    if not keep.any():
        raise ValueError("register_scans: scan %d has no row of three finite coordinates" % k)
    colors = None if colors is None else np.asarray(colors).reshape(-1, 3)[keep]
    normals = None if normals is None else np.asarray(normals, np.float32).reshape(-1, 3)[keep]
    for a, what in ((colors, "colours"), (normals, "normals")):
        if a is not None and len(a) != int(keep.sum()):
            raise ValueError("register_scans: scan %d has %d points and %d %s" % (k, len(p), len(a), what))
    return p[keep], colors, normals


def register_scans(scans, bits=None, voxel_size=None, metric="plane", max_dist=DEFAULT_MAX_DIST, iters=50, tol=1e-3, init=None,
                   estimate_normals=False, clean=None, names=None):
    """scans: list of (points float64 [n,3] in the scanner's units, colors uint8 [n,3] | None, normals [n,3] | None).  Scan 0
    defines the coordinates; scan k >= 1 is registered against the union of scan 0 and the aligned scans before it, on the
    grid of the ingest.Frame fitted to that union with bits / voxel_size.  init: per scan None or (R, t) in scan units;
    names: what to call the scans in an error.
    -> dict: merged = ingest.voxelize_scan(union, ..., clean=clean) as it returns it, poses = per scan the icp result with
    R, t in scan units and "pose" the 4x4 matrix (scan 0: the identity), aligned = the union's (points, colors, normals)."""
    from . import ingest
    if len(scans) < 1:
        raise ValueError("register_scans: no scans")
    # the targets are the scans before the last: every one of them needs normals for the plane metric
    check_arguments(metric, all((tuple(s) + (None, None))[2] is not None for s in scans[:-1]), estimate_normals, iters, tol)
    if (bits is None) == (voxel_size is None):
        raise ValueError("register_scans: give bits or voxel_size, one of them")
    gates = _schedule(max_dist)
    scans = [_finite_scan(k, s) for k, s in enumerate(scans)]
    pts, cols, nrms = [scans[0][0]], [scans[0][1]], [scans[0][2]]
    poses = [{"R": np.eye(3), "t": np.zeros(3), "pose": np.eye(4), "iterations": [], "converged": True, "n_used": len(pts[0]),
              "fitness": 1.0, "rmse": 0.0, "plane_rmse": None}]
    for k in range(1, len(scans)):
        p, col, nrm = scans[k]
        target = np.concatenate(pts)
        frame = ingest.fit_frame(target, bits=bits, voxel_size=voxel_size)
        tn = None
        if metric == "plane":
            tn = np.concatenate(nrms) if all(n is not None for n in nrms) else estimated_target_normals(target, frame)
        start = None if init is None or init[k] is None else pose_from_scan_units(init[k][0], init[k][1], frame)
        try:
            r = icp(to_grid(p, frame), to_grid(target, frame), tn, metric, gates, iters, tol, start)
        except ValueError as e:
            raise ValueError("%s: %s" % (names[k] if names else "scan %d" % k, e))
        r["R"], r["t"] = pose_to_scan_units(r["R"], r["t"], frame)
        r["pose"] = pose_matrix(r["R"], r["t"])
        poses.append(r)
        pts.append(p @ r["R"].T + r["t"])
        cols.append(col)
        nrms.append(None if nrm is None else (nrm.astype(np.float64) @ r["R"].T).astype(np.float32))
    union = (np.concatenate(pts), np.concatenate(cols) if all(c is not None for c in cols) else None,
             np.concatenate(nrms) if all(n is not None for n in nrms) else None)
    merged = ingest.voxelize_scan(union[0], union[1], union[2], bits=bits, voxel_size=voxel_size, clean=clean)
    return {"merged": merged, "poses": poses, "aligned": union}


# ---------------------------------------------------------------------------- <name>.poses.json
def poses_path(ply_or_stem):
    """merged_vox10.ply -> merged_vox10.poses.json"""
    return (ply_or_stem[:-4] if ply_or_stem.lower().endswith(".ply") else ply_or_stem) + ".poses.json"


def write_poses(filename, names, poses):
    entries = [{"file": name, "pose": [[float(v) for v in row] for row in np.asarray(r["pose"], np.float64)],
                "iterations": [int(i) for i in r["iterations"]], "converged": bool(r["converged"]), "fitness": float(r["fitness"]),
                "rmse": float(r["rmse"]), "plane_rmse": None if r["plane_rmse"] is None else float(r["plane_rmse"])}
               for name, r in zip(names, poses)]
    with open(filename, "w") as f:
        json.dump(entries, f, indent=1)


def read_poses(filename):
    """-> the entries as written, each "pose" a float64 4x4 array (repr round-trips a float64 exactly)"""
    with open(filename) as f:
        entries = json.load(f)
    if not isinstance(entries, list):
        raise ValueError("%s: a poses file is a list with one entry per scan" % filename)
    for k, e in enumerate(entries):
        pose = np.asarray(e.get("pose") if isinstance(e, dict) else None, np.float64)
        if pose.shape != (4, 4) or not np.isfinite(pose).all() or pose[3].tolist() != [0.0, 0.0, 0.0, 1.0]:
            raise ValueError("%s: entry %d has no finite 4x4 pose with a last row of 0 0 0 1" % (filename, k))
        e["pose"] = pose
    return entries


# ---------------------------------------------------------------------------- command line
def summary_line(name, r):
    return "register: {}: {} steps {}, {}, fitness {:.4f}, rmse {:.4f}{}".format(
        name, sum(r["iterations"]), r["iterations"], "converged" if r["converged"] else "NOT converged", r["fitness"], r["rmse"],
        "" if r["plane_rmse"] is None else ", plane rmse {:.4f}".format(r["plane_rmse"]))


def parse_args(argv=None):
    from . import ingest
    ap = argparse.ArgumentParser(description="register overlapping scans against the first one and merge them onto the codec's grid")
    ap.add_argument("--input", required=True, nargs="+", help="the scans (ASCII or binary ply); the first defines the coordinates")
    ap.add_argument("--output", required=True, help="the voxelised ply; <output without .ply>.frame and .poses.json are written next to it")
    ap.add_argument("--bits", type=int, default=None, help="fit the union into a grid of 2^bits cells per axis (1..12)")
    ap.add_argument("--voxel_size", type=float, default=None, help="voxel edge in the scans' units; the grid grows to hold the union")
    ap.add_argument("--metric", choices=("plane", "point"), default="plane")
    ap.add_argument("--max_dist", default="4,2,1", help="the gates of the stages in voxels, coarse to fine")
    ap.add_argument("--iters", type=int, default=50, help="most steps per stage")
    ap.add_argument("--tol", type=float, default=1e-3, help="a stage ends when a step moves the target's box by less (voxels)")
    ap.add_argument("--estimate_normals", action="store_true",
                    help="--metric=plane with scans that have no normals: estimate the target's on its voxels (radius 10, 20 neighbours)")
    ap.add_argument("--init", default=None, help="a poses.json with the start pose of every scan, scan units")
    ap.add_argument("--min_fitness", type=float, default=0.3, help="fail when less of a scan lies within the last gate")
    ap.add_argument("--attributes", choices=("colors", "normals"), default="colors",
                    help="which attribute the ply carries when the union has both")
    from .clean import add_clean_argument, check_clean_argument
    add_clean_argument(ap)
    args = ap.parse_args(argv)
    check_clean_argument(ap, args)
    if (args.bits is None) == (args.voxel_size is None):
        ap.error("give --bits or --voxel_size, one of them")
    if args.bits is not None and not 1 <= args.bits <= ingest.MAX_BITS:
        ap.error("--bits=%d outside 1..%d" % (args.bits, ingest.MAX_BITS))
    if args.voxel_size is not None and not (np.isfinite(args.voxel_size) and args.voxel_size > 0):
        ap.error("--voxel_size must be positive (got %r)" % args.voxel_size)
    try:
        args.max_dist = _schedule([float(v) for v in args.max_dist.split(",")])
    except ValueError:
        ap.error("--max_dist is a comma-separated list of positive distances in voxels (got %r)" % (args.max_dist,))
    if args.iters < 1 or not (np.isfinite(args.tol) and args.tol > 0):
        ap.error("--iters must be at least 1 and --tol positive")
    if len(args.input) < 2:
        ap.error("--input takes two scans or more: one has nothing to be registered against")
    if args.metric == "plane" and not args.estimate_normals:
        # with the other argument errors, before anything is loaded: the plane metric measures against the target's normals
        from .test import _ply_has_normals
        for name in args.input[:-1]:
            if not _ply_has_normals(name):
                ap.error("--metric=plane needs normals: %s has no nx ny nz properties (or cannot be read); pass --estimate_normals "
                         "to estimate them, or --metric=point" % name)
    if args.init is not None:
        try:
            args.init_poses = read_poses(args.init)
        except (OSError, ValueError) as e:
            ap.error("--init: %s" % e)
        if len(args.init_poses) != len(args.input):
            ap.error("--init: %s holds %d poses for %d scans" % (args.init, len(args.init_poses), len(args.input)))
    return args


def main(argv=None):
    from . import ingest
    from .dataprocess.inout_points import load_ply_scan, write_ply_colors, write_ply_data, write_ply_normals
    args = parse_args(argv)
    scans = []
    for name in args.input:
        scan = load_ply_scan(name)
        if not len(scan[0]):
            raise SystemExit("register: %s holds no points" % name)
        scans.append(scan)
    init = None
    if args.init is not None:
        init = [(e["pose"][:3, :3], e["pose"][:3, 3]) for e in args.init_poses]
    try:
        out = register_scans(scans, args.bits, args.voxel_size, args.metric, args.max_dist, args.iters, args.tol, init,
                             args.estimate_normals, args.clean, names=args.input)
    except ValueError as e:
        raise SystemExit("register: %s" % e)
    failed = []
    for name, r in list(zip(args.input, out["poses"]))[1:]:
        print(summary_line(name, r))
        if not r["converged"]:
            failed.append("%s did not converge within %d steps per stage (steps %s)" % (name, args.iters, r["iterations"]))
        elif r["fitness"] < args.min_fitness:
            failed.append("%s: fitness %.4f is below --min_fitness=%g" % (name, r["fitness"], args.min_fitness))
    if failed:
        raise SystemExit("register: " + "; ".join(failed))
    merged = out["merged"]
    points, colors, normals, counts, frame, n_dropped = merged[:6]
    if colors is not None and (normals is None or args.attributes == "colors"):
        write_ply_colors(args.output, points, colors)
    elif normals is not None:
        write_ply_normals(args.output, points, normals)
    else:
        write_ply_data(args.output, points)
    ingest.write_frame(ingest.frame_path(args.output), frame)
    write_poses(poses_path(args.output), [os.path.basename(n) for n in args.input], out["poses"])
    print(ingest.summary_line(len(out["aligned"][0]), n_dropped, counts, frame))
    print("wrote {}, {} and {}".format(args.output, ingest.frame_path(args.output), poses_path(args.output)))


if __name__ == "__main__":
    main()
