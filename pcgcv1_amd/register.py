"""Overlapping scans into one cloud: rigid registration (ICP, point-to-plane and point-to-point) on the GPU, then the merge
of pcgcv1_amd/ingest.py.

    python -m pcgcv1_amd.register --input a.ply b.ply c.ply --output merged_vox10.ply --bits 10     # or --voxel_size S
                                  [--metric plane|point|color [--color_weight 0.9] [--color_radius 3] [--color_kmin 6]]
                                  [--max_dist 4,2,1] [--iters 50] [--tol 1e-3] [--estimate_normals]
                                  [--init poses.json] [--smooth SPEC] [--clean SPEC] [--min_fitness 0.3]
                                  [--global_init [--feature_voxel 1] [--feature_radius 8] [--corr_dist 2] [--draws 100000] [--seed 0]]

writes the voxelised ply and merged_vox10.frame as pcgcv1_amd.ingest would for the union of the aligned scans, and
merged_vox10.poses.json: per input the 4x4 pose in the scan's own units and what the loop reports.

The rule (include/pcgc.h, pcgc_register_*; tests/_register_ref.py restates it in numpy).  ICP runs in grid
units, neighbouring surface points about 1 apart.  One step (csrc/offgrid.hip) moves the source by the trial pose, finds
every tied nearest neighbour in the target with the off-grid search, keeps the points within max_dist and reduces them to 45
float64 sums in a fixed order.  The solve is numpy float64 on the host: Kabsch for point-to-point, the 6x6 normal equations
with an exact Rodrigues rotation for point-to-plane.  metric="color" (tests/_color_icp_ref.py) adds a photometric
term to the point-to-plane one: the target's intensity gradients are fitted once (csrc/color_icp.hip), a step gives 59 sums,
and the solve mixes the two systems by color_weight.  max_dist is a coarse-to-fine schedule: with one wide gate the points
beyond the overlap pair with the target's rim and pull the pose.  A start further off than the first gate bridges comes from
init, or from the global alignment below (global_init / --global_init).

Global alignment (include/pcgc.h, pcgc_feature_* and pcgc_ransac_score; tests/_global_ref.py restates it in
numpy; csrc/global.hip).  Each cloud is reduced to one keypoint per cell of feature_voxel with a unit normal; every keypoint
gets a sign-invariant integer descriptor of 33 bytes from the keypoints within `radius`; every source keypoint is paired with
the target keypoint of the nearest descriptor.  On the host, seeded triples of those pairs whose triangles agree in size are
solved by Kabsch (numpy float64), the device counts per pose the pairs it brings within corr_dist, and the pose with the most,
solved again over its inliers, is the start ICP refines.  Every device stage gives integers that equal numpy's.
"""
import argparse
import json
import math
import os

import numpy as np

from . import _lib
from .cells import cell_keys, cell_order, cells_from_bounds, feature_cells              # noqa: F401  (re-exported: tests, tools)

N_SUMS = 45
N_COLOR_SUMS = 59            # pcgc_register_color_step: the plane block [2..29], the valid weight [30], the photometric block [31..58]
MIN_PAIRS = {"point": 3, "plane": 6, "color": 6}
COND_LIMIT = 1e12
DEFAULT_MAX_DIST = (4.0, 2.0, 1.0)
# the colour metric: the photometric share of the joint objective, and the ball the target's intensity gradients
# are fitted in (voxels; at least kmin points, the point itself included).  Of the weights 0.5 and 0.9, 0.9 left the flat and
# the spherical fixtures closest to the truth
DEFAULT_COLOR_WEIGHT, DEFAULT_COLOR_RADIUS, DEFAULT_COLOR_KMIN = 0.9, 3.0, 6
COLOR_MAX_RADIUS, COLOR_MIN_KMIN, COLOR_MAX_KMIN = 16.0, 3, 1 << 20
INTENSITY_SCALE = 2550000    # 255 * (2126 + 7152 + 722)
GRADIENT_BAD_INPUT, GRADIENT_TOO_DENSE = 255, 254              # what pcgc_color_gradient leaves in `valid` when its flag is raised
# global alignment, grid units (neighbouring surface points about 1 apart): keypoints are the voxels ICP sees; a radius of 8
# holds about 200 of them on a surface, enough for an 11-bin histogram and small enough to be local; a pair counts as an
# inlier within 2, so the pose it votes for lands inside ICP's first gate of 4; triangles with a side under 6 fix a rotation
# badly at that tolerance; 20 inliers are far more than the three a triple explains by itself
DEFAULT_FEATURE_VOXEL, DEFAULT_FEATURE_RADIUS, DEFAULT_CORR_DIST, DEFAULT_MIN_EDGE, DEFAULT_MIN_INLIERS = 1.0, 8.0, 2.0, 6.0, 20
DEFAULT_DRAWS = 100000
DRAW_BATCH = 16384           # triples per call of the generator: part of the rule, the stream of draws depends on it
EDGE_RATIO = 0.9
FEATURE_BINS, FEATURE_ROW = 33, 36


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
                         "motions, as a plane, a sphere or too few pairs do not; use metric='color' when the scans carry texture, metric='point', or scans "
                         "with more shape" % cond)
    x = np.linalg.solve(A, g)
    return rodrigues(x[:3]), x[3:]


def color_system(S, weight):
    """the joint system of the colour metric from the 59 sums -> (A symmetric 6x6, g): (1 - weight) times the point-to-plane
    normal equations plus weight times the photometric ones"""
    S = np.asarray(S, np.float64)
    lam = float(weight)
    if not 0.0 < lam < 1.0:
        raise ValueError("icp: color_weight must lie strictly between 0 and 1 (got %r): 0 is metric='plane', and colour alone "
                         "does not see the motion along the normals" % (weight,))
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = (1.0 - lam) * S[2:23] + lam * S[31:52]
    return A + np.triu(A, 1).T, -((1.0 - lam) * S[23:29] + lam * S[52:58])


def solve_color(S, weight):
    """the joint normal equations A x = g of the colour metric -> (dR = the exact rotation of x[:3], dt = x[3:]).  Distances
    are in voxels and intensities in [0, 1]: the weight balances those units."""
    A, g = color_system(S, weight)
    cond = np.linalg.cond(A) if np.isfinite(A).all() else float("inf")
    if not cond <= COND_LIMIT:
        raise ValueError("icp: the joint point-to-plane and colour system is singular (condition %.3g): neither the matched surface "
                         "nor its texture fixes all six motions, as a plane of one colour or too few pairs do not; %d of the pairs "
                         "have an intensity gradient" % (cond, int(round(S[30]))))
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
    n_sums, workspace_bytes, step_symbol = N_SUMS, "pcgc_register_workspace_bytes", "pcgc_register_step"

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
        self.ws = torch.empty(int(getattr(lib, self.workspace_bytes)(self.cells.res, self.m)), dtype=torch.uint8, device=dev)
        self.out = torch.empty(self.n_sums, dtype=torch.float64, device=dev)
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
        order = torch.sort(cell_keys(moved, self.cells.grid(), clamp=True), stable=True)[1]         # a point outside: the nearest cell
        self.source_d = self.source_d[order].contiguous()
        self.order = order if self.order is None else self.order[order]
        return order

    @property
    def centre(self):
        return np.rint((self.lo + self.hi) / 2.0)

    @property
    def radius(self):
        return float(np.linalg.norm(self.hi - self.lo)) / 2.0

    def _clouds(self, with_normals):
        """the arguments of `step_symbol` in front of the cells: the two clouds and what travels with their points"""
        return (_lib.dptr(self.source_d), self.n, _lib.dptr(self.cells.points), self.m, _lib.dptr(self.normals_d if with_normals else None))

    def step(self, R, t, c, max_dist, with_normals=True, per_point=False):
        """-> S float64 [n_sums]; per_point=True: (S, best float64 [n], ties int32 [n]).  RuntimeError when a moved coordinate
        is a NaN or out of every cell's reach."""
        import torch
        R9 = np.ascontiguousarray(np.asarray(R, np.float64).reshape(9))
        t3 = np.ascontiguousarray(np.asarray(t, np.float64).reshape(3))
        c3 = np.ascontiguousarray(np.asarray(c, np.float64).reshape(3))
        dev = self.source_d.device
        best = torch.empty(self.n, dtype=torch.float64, device=dev) if per_point else None
        ties = torch.empty(self.n, dtype=torch.int32, device=dev) if per_point else None
        _lib.check(getattr(_lib.hip(), self.step_symbol)(
            *self._clouds(with_normals), *self.cells.grid(), _lib.nptr(R9), _lib.nptr(t3), _lib.nptr(c3), float(max_dist),
            _lib.dptr(self.out), _lib.dptr(best), _lib.dptr(ties), _lib.dptr(self.ws), self.ws.numel(), _lib.stream()), self.step_symbol)
        S = self.out.cpu().numpy().copy()
        if np.isnan(S).any():
            raise RuntimeError("%s: a moved source coordinate is not finite or leaves every cell's reach, or the target breaks the "
                               "cell rule (include/pcgc.h)" % self.step_symbol)
        if per_point:
            if self.order is not None:
                best, ties = torch.empty_like(best).index_copy_(0, self.order, best), torch.empty_like(ties).index_copy_(0, self.order, ties)
            return S, best.cpu().numpy(), ties.cpu().numpy()
        return S


# ---------------------------------------------------------------------------- the colour metric on the device
def intensity(colors, n, what):
    """colours [n,3] with whole values in 0..255 -> Y int32 [n] = 2126 R + 7152 G + 722 B (BT.709 in integers, 0 .. 2 550 000)"""
    c = np.asarray(colors)
    if c.size != 3 * n:
        raise ValueError("icp: %d %s colours for %d points" % (c.size // 3 if c.size % 3 == 0 else -1, what, n))
    c = c.reshape(n, 3)
    with np.errstate(invalid="ignore"):
        whole = c.dtype.kind in "ui" or bool(np.all(np.isfinite(c)) and np.all(c == np.rint(c)))
    if c.dtype.kind not in "uif" or not whole or (c.size and (c.min() < 0 or c.max() > 255)):
        raise ValueError("icp: the %s colours must be whole numbers in 0..255 (uint8 red, green, blue)" % what)
    c = c.astype(np.int32)
    return np.ascontiguousarray(2126 * c[:, 0] + 7152 * c[:, 1] + 722 * c[:, 2], np.int32)


def check_color_options(color_weight, color_radius, color_kmin):
    if not (np.isfinite(color_weight) and 0.0 < color_weight < 1.0):
        raise ValueError("icp: color_weight must lie strictly between 0 and 1 (got %r)" % (color_weight,))
    if not (np.isfinite(color_radius) and 0.0 < color_radius <= COLOR_MAX_RADIUS):
        raise ValueError("icp: color_radius must be positive and at most %g voxels (got %r)" % (COLOR_MAX_RADIUS, color_radius))
    if not COLOR_MIN_KMIN <= int(color_kmin) <= COLOR_MAX_KMIN:
        raise ValueError("icp: color_kmin outside %d..%d (got %r)" % (COLOR_MIN_KMIN, COLOR_MAX_KMIN, color_kmin))


def color_gradient_step(points_d, normals_d, Y_d, cells, radius, kmin, debug=False):
    """pcgc_color_gradient on device tensors sorted by the key of `cells` (cells_from_bounds, cell_order): points float32
    [n,3], unit normals float32 [n,3], Y int32 [n] -> (g float64 [n,3], valid uint8 [n]) device tensors, with debug also K int32
    [n], Q int64 [n,6], B int64 [n,3].  RuntimeError when the call raised its flag."""
    import torch
    n, dev = int(points_d.shape[0]), points_d.device
    lib = _lib.hip()
    ws = torch.empty(max(1, int(lib.pcgc_color_gradient_workspace_bytes(cells[4], n))), dtype=torch.uint8, device=dev)
    g = torch.empty((n, 3), dtype=torch.float64, device=dev)
    valid = torch.empty(n, dtype=torch.uint8, device=dev)
    K = torch.empty(n, dtype=torch.int32, device=dev) if debug else None
    Q = torch.empty((n, 6), dtype=torch.int64, device=dev) if debug else None
    B = torch.empty((n, 3), dtype=torch.int64, device=dev) if debug else None
    _lib.check(lib.pcgc_color_gradient(_lib.dptr(points_d), _lib.dptr(normals_d), _lib.dptr(Y_d), n, *cells, float(radius), int(kmin),
                                       _lib.dptr(g), _lib.dptr(valid), _lib.dptr(K), _lib.dptr(Q), _lib.dptr(B), _lib.dptr(ws), ws.numel(),
                                       _lib.stream()), "pcgc_color_gradient")
    worst = int(valid.max().item())
    if worst == GRADIENT_TOO_DENSE:
        raise RuntimeError("pcgc_color_gradient: a point has more than %d neighbours within %g voxels: the radius is too large for "
                           "this density; use a smaller color_radius or a coarser grid" % (COLOR_MAX_KMIN, radius))
    if worst == GRADIENT_BAD_INPUT:
        raise RuntimeError("pcgc_color_gradient: a coordinate is not finite or leaves the cells, an intensity lies outside 0..%d, or "
                           "the points are not sorted by cell (include/pcgc.h)" % INTENSITY_SCALE)
    return (g, valid, K, Q, B) if debug else (g, valid)


def color_gradient(points, normals, Y, radius=DEFAULT_COLOR_RADIUS, kmin=DEFAULT_COLOR_KMIN, debug=False):
    """The intensity gradients of a cloud (float32 [n,3] grid units, normals [n,3], Y int32 [n]) in the caller's order ->
    (g float64 [n,3], valid bool [n]) device tensors; debug: also K, Q, B.  The points are sorted by cell for the kernel."""
    import torch
    dev = _lib.require_gpu()
    p = _float32_cloud(points, "target")
    if not np.isfinite(p).all():
        raise ValueError("icp: metric='color' takes a target with finite coordinates")
    p64 = p.astype(np.float64)
    try:
        cells = cells_from_bounds(p64.min(0), p64.max(0), float(radius), "icp")
    except ValueError as e:
        raise ValueError(str(e).replace("keypoints", "a target"))
    p_d = torch.from_numpy(p).to(dev)
    order = cell_order(p_d, cells)
    n_d = torch.from_numpy(_unit_normals(normals, len(p))).to(dev)
    Y_d = torch.from_numpy(np.ascontiguousarray(Y, np.int32).reshape(len(p))).to(dev)
    got = color_gradient_step(p_d[order].contiguous(), n_d[order].contiguous(), Y_d[order].contiguous(), cells, radius, kmin, debug)
    back = [torch.empty_like(a).index_copy_(0, order, a) for a in got]
    back[1] = back[1] != 0
    return tuple(back)


class ColorMatcher(Matcher):
    """Matcher for metric="color": the source's and the target's intensities travel with the points, and the target's
    intensity gradients are fitted once (pcgc_color_gradient) and kept in the matcher's cell order.  colours: whole numbers
    in 0..255, [n,3] / [m,3]; the target's normals are required."""
    n_sums, workspace_bytes, step_symbol = N_COLOR_SUMS, "pcgc_register_color_workspace_bytes", "pcgc_register_color_step"

    def __init__(self, source, target, target_normals, source_colors, target_colors, color_radius=DEFAULT_COLOR_RADIUS,
                 color_kmin=DEFAULT_COLOR_KMIN):
        import torch
        if target_normals is None or source_colors is None or target_colors is None:
            raise ValueError("icp: metric='color' needs the target's normals and the colours of both clouds")
        Yp = intensity(source_colors, len(_float32_cloud(source, "source")), "source")
        Yq = intensity(target_colors, len(_float32_cloud(target, "target")), "target")
        Matcher.__init__(self, source, target, target_normals)
        dev = self.source_d.device
        grad, valid = color_gradient(target, target_normals, Yq, color_radius, color_kmin)
        self.Yp_d = torch.from_numpy(Yp).to(dev)
        self.Yq_d = torch.from_numpy(Yq).to(dev)[self.cells.order].contiguous()
        self.grad_d = grad[self.cells.order].contiguous()
        self.valid_d = valid.to(torch.uint8)[self.cells.order].contiguous()
        self.n_valid = int(valid.sum().item())

    def sort_source(self, R, t):
        order = Matcher.sort_source(self, R, t)
        self.Yp_d = self.Yp_d[order].contiguous()
        return order

    def _clouds(self, with_normals):
        return (_lib.dptr(self.source_d), _lib.dptr(self.Yp_d), self.n, _lib.dptr(self.cells.points), _lib.dptr(self.normals_d),
                _lib.dptr(self.Yq_d), _lib.dptr(self.grad_d), _lib.dptr(self.valid_d), self.m)


# ---------------------------------------------------------------------------- the loop
def _schedule(max_dist):
    gates = [float(g) for g in (max_dist if isinstance(max_dist, (tuple, list, np.ndarray)) else (max_dist,))]
    if not gates or not all(np.isfinite(g) and g > 0 for g in gates):
        raise ValueError("icp: max_dist must be positive distances in grid units (got %r)" % (max_dist,))
    return gates


def check_arguments(metric, have_normals, estimate_normals=False, iters=50, tol=1e-3):
    """the argument errors of icp / register_scans, before any work"""
    if metric not in MIN_PAIRS:
        raise ValueError("icp: metric must be 'plane', 'point' or 'color' (got %r)" % (metric,))
    if metric in ("plane", "color") and not have_normals and not estimate_normals:
        raise ValueError("icp: metric='%s' needs the target's normals: give them, estimate them (estimate_normals / "
                         "--estimate_normals), or use metric='point'" % metric)
    if int(iters) < 1 or not (np.isfinite(tol) and tol > 0):
        raise ValueError("icp: iters must be at least 1 and tol positive (got %r, %r)" % (iters, tol))


def _rows(a):
    a = np.asarray(a)
    return a.size // 3 if a.size % 3 == 0 else -1


def check_color_arguments(n_source, n_target, source_colors, target_colors, color_weight, color_radius, color_kmin):
    """the argument errors of metric='color', before any work"""
    check_color_options(color_weight, color_radius, color_kmin)
    if source_colors is None or target_colors is None:
        raise ValueError("icp: metric='color' needs source_colors and target_colors (%s missing): scans without colours register "
                         "with metric='plane' or 'point'" % ("both are" if source_colors is None and target_colors is None else
                                                               "source_colors is" if source_colors is None else "target_colors is"))
    for a, n, what in ((source_colors, n_source, "source"), (target_colors, n_target, "target")):
        if _rows(a) != n:
            raise ValueError("icp: %d %s colours for %d %s points" % (_rows(a), what, n, what))


def icp(source, target, target_normals=None, metric="plane", max_dist=DEFAULT_MAX_DIST, iters=50, tol=1e-3, init=None,
        source_colors=None, target_colors=None, color_weight=DEFAULT_COLOR_WEIGHT, color_radius=DEFAULT_COLOR_RADIUS,
        color_kmin=DEFAULT_COLOR_KMIN):
    """Align `source` to `target` (float32 [n,3] / [m,3], grid units) from the pose init = (R, t), identity when None ->
    dict: R, t (target ~ R source + t), iterations (per stage), converged, n_used, fitness = n_used / n, rmse =
    sqrt(sum of best / n_used), plane_rmse (plane and colour mode, else None).  Each entry of max_dist is a stage of at most
    `iters` steps that ends when the last step moved no point of the target's bounding box by `tol`; one more step at the
    final pose gives the figures.  ValueError: nothing within max_dist, or a singular system.
    metric="color": source_colors and target_colors ([n,3] / [m,3], whole numbers in 0..255) are required with the target's
    normals; color_weight in (0, 1) is the photometric share of the joint objective; the target's intensity gradients are
    fitted over the points within color_radius voxels, at least color_kmin of them.  The result gains color_rmse =
    sqrt(sum of w rc^2 / sum of w) over the pairs whose target point has a gradient, in intensity units of [0, 1], and
    color_fitness = that sum of w / n_used."""
    check_arguments(metric, target_normals is not None, False, iters, tol)
    gates = _schedule(max_dist)
    plane, color = metric == "plane", metric == "color"
    if color:
        check_color_arguments(_rows(source), _rows(target), source_colors, target_colors, color_weight, color_radius, color_kmin)
        m = ColorMatcher(source, target, target_normals, source_colors, target_colors, color_radius, color_kmin)
    else:
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
            dR, dt = solve_color(S, color_weight) if color else solve_plane(S) if plane else solve_point(S)
            R, t = compose(R, t, c, dR, dt)
            k += 1
            done = rotation_angle(dR) * rho + float(np.linalg.norm(dt)) < tol
        iterations.append(k)
        converged = converged and done
    S = m.step(R, t, c, gates[-1], plane)
    n_used = int(S[0])
    out = {"R": R, "t": t, "iterations": iterations, "converged": converged, "n_used": n_used, "fitness": n_used / m.n,
           "rmse": math.sqrt(S[1] / n_used) if n_used else float("nan"),
           "plane_rmse": (math.sqrt(S[29 if color else 44] / n_used) if n_used else float("nan")) if plane or color else None}
    if color:
        out["color_rmse"] = math.sqrt(S[58] / S[30]) if S[30] > 0 else float("nan")
        out["color_fitness"] = S[30] / n_used if n_used else float("nan")
    return out


# ---------------------------------------------------------------------------- global alignment: the device stages
def keypoints(points, normals, feature_voxel):
    """points float32 [n,3] in grid units, normals [n,3] or None -> (keypoints float32 [m,3], unit normals float32 [m,3]):
    one keypoint per occupied cell of edge feature_voxel (ingest's frame, quantise and merge), at the cell's position, rows
    in ascending cell key; its normal is the merged normal, or without normals metrics.estimate_normals of those cells"""
    from . import ingest, metrics
    p = _float32_cloud(points, "global_align").astype(np.float64)
    if not (np.isfinite(feature_voxel) and feature_voxel > 0):
        raise ValueError("global_align: feature_voxel must be positive (got %r)" % (feature_voxel,))
    try:
        frame = ingest.fit_frame(p, voxel_size=float(feature_voxel))
    except ValueError as e:
        raise ValueError("global_align: %s" % e)
    _, keys = ingest.quantize(p, frame)
    vox, _, _, nrm = ingest.merge(keys, frame.bits, None, None if normals is None else np.asarray(normals, np.float32).reshape(-1, 3))
    if normals is None:
        nrm = metrics.estimate_normals(vox)
    return ingest.apply_frame(vox, frame).astype(np.float32), _unit_normals(nrm, len(vox))


class _FeatureCloud(object):
    """keypoints and normals on the device, sorted by the cell key pcgc_feature_* want; rows come back in the caller's order"""

    def __init__(self, kp, normals, radius, cells=None):
        import torch
        self.dev = _lib.require_gpu()
        kp = _float32_cloud(kp, "keypoint")
        nrm = np.ascontiguousarray(np.asarray(normals), np.float32).reshape(-1, 3)
        if len(nrm) != len(kp):
            raise ValueError("global_align: %d normals for %d keypoints" % (len(nrm), len(kp)))
        self.n, self.radius = len(kp), float(radius)
        self.cells = feature_cells(kp, radius) if cells is None else cells
        res = self.cells[4]
        self.order = cell_order(torch.from_numpy(kp), self.cells).numpy()
        self.kp = torch.from_numpy(kp[self.order]).to(self.dev)
        self.normals = torch.from_numpy(nrm[self.order]).to(self.dev)
        self.ws = torch.empty(max(1, int(_lib.hip().pcgc_feature_workspace_bytes(res, self.n))), dtype=torch.uint8, device=self.dev)

    def back(self, t):
        out = np.empty_like(t.cpu().numpy())
        out[self.order] = t.cpu().numpy()
        return out

    def pairs(self):
        import torch
        S = torch.empty((self.n, FEATURE_BINS), dtype=torch.int32, device=self.dev)          # uint32 on the device
        k = torch.empty(self.n, dtype=torch.int32, device=self.dev)
        _lib.check(_lib.hip().pcgc_feature_pairs(_lib.dptr(self.kp), _lib.dptr(self.normals), self.n, *self.cells, self.radius, _lib.dptr(S),
                                                 _lib.dptr(k), _lib.dptr(self.ws), self.ws.numel(), _lib.stream()), "pcgc_feature_pairs")
        if int(k.min().item()) < 0:
            raise RuntimeError("pcgc_feature_pairs: a keypoint coordinate is not finite or leaves the cells, or the keypoints are not "
                               "sorted by cell (include/pcgc.h)")
        return S, k

    def combine(self, S, k):
        import torch
        feat = torch.empty((self.n, FEATURE_ROW), dtype=torch.uint8, device=self.dev)
        valid = torch.empty(self.n, dtype=torch.uint8, device=self.dev)
        _lib.check(_lib.hip().pcgc_feature_combine(_lib.dptr(self.kp), _lib.dptr(self.normals), self.n, *self.cells, self.radius, _lib.dptr(S),
                                                   _lib.dptr(k), _lib.dptr(feat), _lib.dptr(valid), _lib.dptr(self.ws), self.ws.numel(),
                                                   _lib.stream()), "pcgc_feature_combine")
        if int(valid.max().item()) > 1:
            raise RuntimeError("pcgc_feature_combine: a keypoint coordinate is not finite or leaves the cells, or the keypoints are "
                               "not sorted by cell (include/pcgc.h)")
        return feat, valid


def feature_pairs(kp, normals, radius, cells=None):
    """stage 1 (pcgc_feature_pairs) -> (S uint32 [n,33], k int32 [n]) in the caller's order.  RuntimeError for a NaN keypoint."""
    c = _FeatureCloud(kp, normals, radius, cells)
    S, k = c.pairs()
    return c.back(S).view(np.uint32), c.back(k)


def feature_combine(kp, normals, radius, S, k, cells=None):
    """stage 2 (pcgc_feature_combine) from S uint32 [n,33] and k int32 [n] -> (feat uint8 [n,36], valid bool [n])"""
    import torch
    c = _FeatureCloud(kp, normals, radius, cells)
    S = np.ascontiguousarray(np.asarray(S, np.uint32).reshape(c.n, FEATURE_BINS)[c.order]).view(np.int32)
    k = np.ascontiguousarray(np.asarray(k, np.int32).reshape(c.n)[c.order])
    feat, valid = c.combine(torch.from_numpy(S).to(c.dev), torch.from_numpy(k).to(c.dev))
    return c.back(feat), c.back(valid).astype(bool)


def features(kp, normals, radius):
    """keypoints float32 [n,3] and their unit normals -> (descriptors uint8 [n,36], valid bool [n]): stages 1 and 2"""
    c = _FeatureCloud(kp, normals, radius)
    feat, valid = c.combine(*c.pairs())
    return c.back(feat), c.back(valid).astype(bool)


def match_features(fs, vs, ft, vt):
    """stage 3 (pcgc_feature_match): per valid source row the valid target row of the nearest descriptor -> (j int32 [n],
    dist uint32 [n]); -1 and 0xFFFFFFFF for an invalid source row"""
    import torch
    dev = _lib.require_gpu()
    rows = [np.ascontiguousarray(np.asarray(f), np.uint8).reshape(-1, FEATURE_ROW) for f in (fs, ft)]
    valid = [np.ascontiguousarray(np.asarray(v).astype(bool), np.uint8).reshape(-1) for v in (vs, vt)]
    if not len(rows[0]) or not len(rows[1]) or len(valid[0]) != len(rows[0]) or len(valid[1]) != len(rows[1]):
        raise ValueError("match_features: needs source and target rows, each with its valid flags")
    fs_d, ft_d, vs_d, vt_d = (torch.from_numpy(a).to(dev) for a in (rows[0], rows[1], valid[0], valid[1]))
    n, m = len(rows[0]), len(rows[1])
    lib = _lib.hip()
    ws = torch.empty(int(lib.pcgc_feature_match_workspace_bytes(n)), dtype=torch.uint8, device=dev)
    j = torch.empty(n, dtype=torch.int32, device=dev)
    dist = torch.empty(n, dtype=torch.int32, device=dev)
    _lib.check(lib.pcgc_feature_match(_lib.dptr(fs_d), _lib.dptr(vs_d), n, _lib.dptr(ft_d), _lib.dptr(vt_d), m, _lib.dptr(j), _lib.dptr(dist),
                                      _lib.dptr(ws), ws.numel(), _lib.stream()), "pcgc_feature_match")
    return j.cpu().numpy(), dist.cpu().numpy().view(np.uint32)


class Scorer(object):
    """stage 4 (pcgc_ransac_score): correspondences P -> Q (float32 [C,3]) on the device, and the inlier counts of poses"""

    def __init__(self, P, Q, dist):
        import torch
        self.dev = _lib.require_gpu()
        P, Q = _float32_cloud(P, "correspondence"), _float32_cloud(Q, "correspondence")
        if len(P) != len(Q):
            raise ValueError("global_align: %d source and %d target correspondences" % (len(P), len(Q)))
        self.P, self.Q, self.C, self.dist = torch.from_numpy(P).to(self.dev), torch.from_numpy(Q).to(self.dev), len(P), float(dist)

    def __call__(self, poses):
        """poses float64 [K,12], R row-major then t -> int32 [K]"""
        import torch
        poses = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 12))
        poses_d = torch.from_numpy(poses).to(self.dev)
        counts = torch.empty(len(poses), dtype=torch.int32, device=self.dev)
        _lib.check(_lib.hip().pcgc_ransac_score(_lib.dptr(poses_d), len(poses), _lib.dptr(self.P), _lib.dptr(self.Q), self.C, self.dist,
                                                _lib.dptr(counts), _lib.stream()), "pcgc_ransac_score")
        return counts.cpu().numpy()


def score_poses(poses, P, Q, dist):
    return Scorer(P, Q, dist)(poses)


# ---------------------------------------------------------------------------- global alignment: the draws and their solve (host, float64)
def _edges(x, tri):
    """float64 [K,3]: the lengths of the edges 0-1, 1-2, 2-0 of the triangles tri [K,3] of the points x (float64 [C,3])"""
    a = x[tri]
    d = a - a[:, (1, 2, 0), :]
    return np.sqrt((d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2])


def keep_triples(tri, P, Q, min_edge):
    """bool [K]: distinct indices, every source edge at least min_edge, every source edge and its target edge within a factor
    of 0.9 of each other.  P, Q float64 [C,3]."""
    distinct = (tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 2] != tri[:, 0])
    es, et = _edges(P, tri), _edges(Q, tri)
    return distinct & (es >= float(min_edge)).all(1) & (et >= EDGE_RATIO * es).all(1) & (es >= EDGE_RATIO * et).all(1)


def kabsch(a, b):
    """a, b float64 [K,M,3] -> (R [K,3,3], t [K,3]) with b ~ R a + t: solve_point's rule (the determinant fix included), batched"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    m = float(a.shape[1])
    mu_a, mu_b = a.sum(1) / m, b.sum(1) / m
    H = np.einsum("kmi,kmj->kij", a - mu_a[:, None, :], b - mu_b[:, None, :])
    U, _, Vt = np.linalg.svd(H)
    V, Ut = np.swapaxes(Vt, 1, 2), np.swapaxes(U, 1, 2)
    D = np.zeros_like(H)
    D[:, 0, 0] = D[:, 1, 1] = 1.0
    D[:, 2, 2] = np.sign(np.linalg.det(V @ Ut))
    R = V @ D @ Ut
    return R, mu_b - np.einsum("kij,kj->ki", R, mu_a)


def draw_hypotheses(P, Q, min_edge, draws, seed):
    """The seeded triples of correspondence indices, DRAW_BATCH per call of np.random.default_rng(seed).integers, and the
    poses of the kept ones -> (poses float64 [K,12], draw index int64 [K]) in draw order; a pose that is not finite is dropped"""
    rng = np.random.default_rng(seed)
    P64, Q64 = np.asarray(P, np.float32).astype(np.float64), np.asarray(Q, np.float32).astype(np.float64)
    poses, index = [], []
    for d0 in range(0, int(draws), DRAW_BATCH):
        tri = rng.integers(0, len(P64), size=(min(DRAW_BATCH, int(draws) - d0), 3))
        kept = np.nonzero(keep_triples(tri, P64, Q64, min_edge))[0]
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


def inlier_mask(pose, P, Q, dist):
    """pcgc_ransac_score's rule for one pose on the host -> bool [C]"""
    pose = np.asarray(pose, np.float64).reshape(12)
    p = np.asarray(P, np.float32).astype(np.float64)
    q = np.asarray(Q, np.float32).astype(np.float64)
    d = []
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(3):
            moved = (((pose[3 * r] * p[:, 0] + pose[3 * r + 1] * p[:, 1]) + pose[3 * r + 2] * p[:, 2]) + pose[9 + r]).astype(np.float32)
            d.append(moved.astype(np.float64) - q[:, r])
        return ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) <= float(dist) * float(dist)


def ransac(P, Q, corr_dist=DEFAULT_CORR_DIST, min_edge=DEFAULT_MIN_EDGE, draws=DEFAULT_DRAWS, seed=0, min_inliers=DEFAULT_MIN_INLIERS,
           scorer=None):
    """correspondences P -> Q (float32 [C,3]) -> dict R, t (Q ~ R P + t), inliers, correspondences, hypotheses, draw, draws.
    The pose with the most inliers among the kept draws (the lowest draw among equals), solved once more over its inliers.
    scorer: poses [K,12] -> counts, in place of the device's Scorer (the tests of the host rule run without a device)."""
    if not (np.isfinite(corr_dist) and corr_dist > 0 and np.isfinite(min_edge) and min_edge >= 0 and int(draws) >= 1):
        raise ValueError("global_align: corr_dist must be positive, min_edge not negative, draws at least 1 (got %r, %r, %r)"
                         % (corr_dist, min_edge, draws))
    if len(P) < 3:
        raise ValueError("global_align: fewer than 3 valid correspondences (%d): the clouds have too few keypoints with neighbours within "
                         "the feature radius; use a smaller feature_voxel or a larger radius" % len(P))
    poses, draw = draw_hypotheses(P, Q, min_edge, draws, seed)
    if not len(poses):
        raise ValueError("global_align: no triple kept: none of %d draws among %d correspondences has three distinct pairs with source "
                         "edges of at least %g that match their target edges within a factor of %g; lower min_edge or draw more"
                         % (int(draws), len(P), min_edge, EDGE_RATIO))
    scorer = Scorer(P, Q, corr_dist) if scorer is None else scorer
    counts = np.asarray(scorer(poses))
    w = int(np.argmax(counts))                                 # the first of equals: the lowest draw
    inl = inlier_mask(poses[w], P, Q, corr_dist)
    P64, Q64 = np.asarray(P, np.float32).astype(np.float64), np.asarray(Q, np.float32).astype(np.float64)
    R, t = kabsch(P64[inl][None], Q64[inl][None])
    refined = np.concatenate([R.reshape(9), t.reshape(3)])
    n_in = int(scorer(refined[None])[0]) if np.isfinite(refined).all() else 0
    if n_in < min_inliers:
        raise ValueError("global_align: the best of %d poses has %d inliers of %d correspondences, below min_inliers = %d: the scans may "
                         "not overlap, or their shape gives the descriptors nothing to hold on to"
                         % (len(poses), n_in, len(P), min_inliers))
    return {"R": R[0], "t": t[0], "inliers": n_in, "correspondences": len(P), "hypotheses": len(poses), "draw": int(draw[w]),
            "draws": int(draws), "raw_inliers": int(counts[w])}


def correspondences(source_kp, fs, vs, target_kp, ft, vt):
    """-> (P float32 [C,3], Q float32 [C,3], source rows, target rows): every valid source keypoint and its match"""
    j, _ = match_features(fs, vs, ft, vt)
    rows = np.nonzero(j >= 0)[0]
    return np.asarray(source_kp, np.float32)[rows], np.asarray(target_kp, np.float32)[j[rows]], rows, j[rows].astype(np.int64)


def global_align(source, target, source_normals=None, target_normals=None, feature_voxel=DEFAULT_FEATURE_VOXEL,
                 radius=DEFAULT_FEATURE_RADIUS, corr_dist=DEFAULT_CORR_DIST, min_edge=DEFAULT_MIN_EDGE, draws=DEFAULT_DRAWS, seed=0,
                 min_inliers=DEFAULT_MIN_INLIERS):
    """A start for icp from any relative pose.  source, target float32 [n,3] / [m,3] in grid units, their normals (of either
    sign) or None: estimated on the keypoint cells -> dict: R, t (target ~ R source + t), inliers, correspondences, hypotheses
    (kept draws), draw (the winner's index) and draws.  The pose is coarse: within about corr_dist, which icp's first gate must
    bridge.  ValueError: fewer than 3 valid correspondences, no triple kept, a winner below min_inliers."""
    ks, ns = keypoints(source, source_normals, feature_voxel)
    kt, nt = keypoints(target, target_normals, feature_voxel)
    fs, vs = features(ks, ns, radius)
    ft, vt = features(kt, nt, radius)
    P, Q, _, _ = correspondences(ks, fs, vs, kt, ft, vt) if vt.any() and vs.any() else (ks[:0], kt[:0], None, None)
    return ransac(P, Q, corr_dist, min_edge, draws, seed, min_inliers)


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
                   estimate_normals=False, clean=None, names=None, global_init=False, global_options=None, smooth=None,
                   color_weight=DEFAULT_COLOR_WEIGHT, color_radius=DEFAULT_COLOR_RADIUS, color_kmin=DEFAULT_COLOR_KMIN):
    """scans: list of (points float64 [n,3] in the scanner's units, colors uint8 [n,3] | None, normals [n,3] | None).  Scan 0
    defines the coordinates; scan k >= 1 is registered against the union of scan 0 and the aligned scans before it, on the
    grid of the ingest.Frame fitted to that union with bits / voxel_size.  init: per scan None or (R, t) in scan units;
    names: what to call the scans in an error.  global_init: a scan k >= 1 without an init starts from global_align against
    the union before it (global_options: its keyword arguments), normals a scan lacks estimated on its voxels; icp then runs
    unchanged, and the scan's pose entry gains "global": inliers, correspondences, hypotheses, draw.
    smooth (a --smooth spec, pcgcv1_amd/smooth.py): the aligned union's positions are smoothed just before the merge, which is
    where the sheets of the same surface lie on top of each other; the result gains "smooth", the line the command prints.
    metric="color": every scan needs colours (the union's travel along as the target's); the target's normals follow the rule
    of "plane"; color_weight, color_radius and color_kmin are icp's.
    -> dict: merged = ingest.voxelize_scan(union, ..., clean=clean) as it returns it, poses = per scan the icp result with
    R, t in scan units and "pose" the 4x4 matrix (scan 0: the identity), aligned = the union's (points, colors, normals), as
    registered: not smoothed."""
    from . import ingest
    if len(scans) < 1:
        raise ValueError("register_scans: no scans")
    # the targets are the scans before the last: every one of them needs normals for the plane metric
    check_arguments(metric, all((tuple(s) + (None, None))[2] is not None for s in scans[:-1]), estimate_normals, iters, tol)
    if metric == "color":
        check_color_options(color_weight, color_radius, color_kmin)
        for k, scan in enumerate(scans):
            if (tuple(scan) + (None,))[1] is None:
                raise ValueError("register_scans: metric='color' needs the colours of every scan, and %s has none: use metric='plane' "
                                 "or 'point'" % (names[k] if names else "scan %d" % k))
    if (bits is None) == (voxel_size is None):
        raise ValueError("register_scans: give bits or voxel_size, one of them")
    gates = _schedule(max_dist)
    if smooth:
        from .smooth import parse_spec
        smooth = parse_spec(smooth)
    scans = [_finite_scan(k, s) for k, s in enumerate(scans)]
    pts, cols, nrms = [scans[0][0]], [scans[0][1]], [scans[0][2]]
    poses = [{"R": np.eye(3), "t": np.zeros(3), "pose": np.eye(4), "iterations": [], "converged": True, "n_used": len(pts[0]),
              "fitness": 1.0, "rmse": 0.0, "plane_rmse": None}]
    for k in range(1, len(scans)):
        p, col, nrm = scans[k]
        target = np.concatenate(pts)
        frame = ingest.fit_frame(target, bits=bits, voxel_size=voxel_size)
        tn = None
        if metric in ("plane", "color"):
            tn = np.concatenate(nrms) if all(n is not None for n in nrms) else estimated_target_normals(target, frame)
        start = None if init is None or init[k] is None else pose_from_scan_units(init[k][0], init[k][1], frame)
        coarse = None
        try:
            if global_init and start is None:
                # normals for the descriptors: the scans' own, else estimated on the voxels of the registration grid, as the
                # plane metric's are (the keypoint cells may be finer than the points lie, and estimate nothing there)
                given = tn if tn is not None else (np.concatenate(nrms) if all(n is not None for n in nrms) else
                                                   estimated_target_normals(target, frame))
                own = nrm if nrm is not None else estimated_target_normals(p, ingest.fit_frame(p, voxel_size=frame.step))
                coarse = global_align(to_grid(p, frame), to_grid(target, frame), own, given, **(global_options or {}))
                start = (coarse["R"], coarse["t"])
            if metric == "color":
                r = icp(to_grid(p, frame), to_grid(target, frame), tn, metric, gates, iters, tol, start, source_colors=col,
                        target_colors=np.concatenate(cols), color_weight=color_weight, color_radius=color_radius, color_kmin=color_kmin)
            else:
                r = icp(to_grid(p, frame), to_grid(target, frame), tn, metric, gates, iters, tol, start)
        except ValueError as e:
            raise ValueError("%s: %s" % (names[k] if names else "scan %d" % k, e))
        if coarse is not None:
            r["global"] = {key: coarse[key] for key in ("inliers", "correspondences", "hypotheses", "draw")}
        r["R"], r["t"] = pose_to_scan_units(r["R"], r["t"], frame)
        r["pose"] = pose_matrix(r["R"], r["t"])
        poses.append(r)
        pts.append(p @ r["R"].T + r["t"])
        cols.append(col)
        nrms.append(None if nrm is None else (nrm.astype(np.float64) @ r["R"].T).astype(np.float32))
    union = (np.concatenate(pts), np.concatenate(cols) if all(c is not None for c in cols) else None,
             np.concatenate(nrms) if all(n is not None for n in nrms) else None)
    if not smooth:
        merged = ingest.voxelize_scan(union[0], union[1], union[2], bits=bits, voxel_size=voxel_size, clean=clean)
        return {"merged": merged, "poses": poses, "aligned": union}
    smoothed, moved = ingest.smooth_points(union[0], None, bits, voxel_size, smooth)
    merged = ingest.voxelize_scan(smoothed, union[1], union[2], bits=bits, voxel_size=voxel_size, clean=clean)
    return {"merged": merged, "poses": poses, "aligned": union, "smooth": ingest.smooth_line(union[0], smoothed, moved, bits, voxel_size)}


# ---------------------------------------------------------------------------- <name>.poses.json
def poses_path(ply_or_stem):
    """merged_vox10.ply -> merged_vox10.poses.json"""
    return (ply_or_stem[:-4] if ply_or_stem.lower().endswith(".ply") else ply_or_stem) + ".poses.json"


def write_poses(filename, names, poses):
    entries = [{"file": name, "pose": [[float(v) for v in row] for row in np.asarray(r["pose"], np.float64)],
                "iterations": [int(i) for i in r["iterations"]], "converged": bool(r["converged"]), "fitness": float(r["fitness"]),
                "rmse": float(r["rmse"]), "plane_rmse": None if r["plane_rmse"] is None else float(r["plane_rmse"])}
               for name, r in zip(names, poses)]
    for e, r in zip(entries, poses):
        for key in ("color_rmse", "color_fitness"):            # metric="color" only
            if key in r:
                e[key] = float(r[key])
        if "global" in r:                                      # the coarse start the scan's icp began from (--global_init)
            e["global"] = {key: int(v) for key, v in r["global"].items()}
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
def _ply_has_colors(filename):
    """whether the ply's header declares one of the colour triples load_ply_scan reads (False for a file that is missing or
    has no header)"""
    from .dataprocess.inout_points import _COLOR_NAMES
    try:
        with open(filename, "rb") as f:
            head = f.read(1 << 16)
    except (OSError, TypeError):
        return False
    end = head.find(b"end_header")
    if end < 0:
        return False
    props = {ln.split()[-1].decode("ascii", "replace") for ln in head[:end].split(b"\n") if ln.strip().startswith(b"property")}
    return any(set(names) <= props for names in _COLOR_NAMES)


def summary_line(name, r):
    return "register: {}: {} steps {}, {}, fitness {:.4f}, rmse {:.4f}{}{}".format(
        name, sum(r["iterations"]), r["iterations"], "converged" if r["converged"] else "NOT converged", r["fitness"], r["rmse"],
        "" if r["plane_rmse"] is None else ", plane rmse {:.4f}".format(r["plane_rmse"]),
        "" if "color_rmse" not in r else ", colour rmse {:.4f}, colour fitness {:.4f}".format(r["color_rmse"], r["color_fitness"]))


def parse_args(argv=None):
    from . import ingest
    ap = argparse.ArgumentParser(description="register overlapping scans against the first one and merge them onto the codec's grid")
    ap.add_argument("--input", required=True, nargs="+", help="the scans (ASCII or binary ply); the first defines the coordinates")
    ap.add_argument("--output", required=True, help="the voxelised ply; <output without .ply>.frame and .poses.json are written next to it")
    ap.add_argument("--bits", type=int, default=None, help="fit the union into a grid of 2^bits cells per axis (1..12)")
    ap.add_argument("--voxel_size", type=float, default=None, help="voxel edge in the scans' units; the grid grows to hold the union")
    ap.add_argument("--metric", choices=("plane", "point", "color"), default="plane",
                    help="color: point-to-plane plus a photometric term, for scans whose shape leaves a motion free (a wall, a vase, a "
                         "sphere) and whose texture does not; every scan needs red, green and blue")
    ap.add_argument("--color_weight", type=float, default=DEFAULT_COLOR_WEIGHT,
                    help="--metric=color: the photometric share of the joint objective, strictly between 0 and 1 (default %(default)g)")
    ap.add_argument("--color_radius", type=float, default=DEFAULT_COLOR_RADIUS,
                    help="--metric=color: the target's intensity gradients are fitted over the points within this many voxels "
                         "(default %(default)g, at most 16)")
    ap.add_argument("--color_kmin", type=int, default=DEFAULT_COLOR_KMIN,
                    help="--metric=color: a target point with fewer such points, itself included, has no gradient (default %(default)d)")
    ap.add_argument("--max_dist", default="4,2,1", help="the gates of the stages in voxels, coarse to fine")
    ap.add_argument("--iters", type=int, default=50, help="most steps per stage")
    ap.add_argument("--tol", type=float, default=1e-3, help="a stage ends when a step moves the target's box by less (voxels)")
    ap.add_argument("--estimate_normals", action="store_true",
                    help="--metric=plane with scans that have no normals: estimate the target's on its voxels (radius 10, 20 neighbours)")
    ap.add_argument("--init", default=None, help="a poses.json with the start pose of every scan, scan units")
    ap.add_argument("--min_fitness", type=float, default=0.3, help="fail when less of a scan lies within the last gate")
    ap.add_argument("--global_init", action="store_true",
                    help="start every scan from a global alignment against the scans before it (descriptor matching and RANSAC), so "
                         "that any relative pose will do; not with --init.  A scan without normals gets them estimated on its "
                         "voxels.  The pose it finds is coarse, within about --corr_dist: the first gate of --max_dist must "
                         "bridge that, as the default 4 does for the default 2")
    ap.add_argument("--feature_voxel", type=float, default=DEFAULT_FEATURE_VOXEL,
                    help="--global_init: edge of the cells that give one keypoint each, in voxels (default %(default)g: the voxels "
                         "the registration itself sees)")
    ap.add_argument("--feature_radius", type=float, default=DEFAULT_FEATURE_RADIUS,
                    help="--global_init: the neighbourhood a descriptor describes, in voxels (default %(default)g: about 200 "
                         "keypoints of a surface, enough to fill the histograms and still local)")
    ap.add_argument("--corr_dist", type=float, default=DEFAULT_CORR_DIST,
                    help="--global_init: a matched pair counts for a pose that brings it within this many voxels (default "
                         "%(default)g: half the first gate, so the winner lands inside it)")
    ap.add_argument("--draws", type=int, default=DEFAULT_DRAWS,
                    help="--global_init: triples of matched pairs drawn (default %(default)d: about one in 70 passes the edge "
                         "checks, and of those about one in 100 is near the truth)")
    ap.add_argument("--seed", type=int, default=0, help="--global_init: seed of the draws (default %(default)d); the same seed, the same pose")
    ap.add_argument("--attributes", choices=("colors", "normals"), default="colors",
                    help="which attribute the ply carries when the union has both")
    from .clean import add_clean_argument, check_clean_argument
    add_clean_argument(ap)
    from .smooth import add_smooth_argument, check_smooth_argument
    add_smooth_argument(ap)
    args = ap.parse_args(argv)
    check_clean_argument(ap, args)
    check_smooth_argument(ap, args)
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
    if args.metric == "color":
        try:
            check_color_options(args.color_weight, args.color_radius, args.color_kmin)
        except ValueError as e:
            ap.error(str(e).replace("icp: color_", "--color_"))
        for name in args.input:                               # the headers only: no scan is parsed yet
            if not _ply_has_colors(name):
                ap.error("--metric=color needs colours: %s has no red green blue properties (or cannot be read); use --metric=plane "
                         "or --metric=point" % name)
    if args.metric in ("plane", "color") and not args.estimate_normals:
        # with the other argument errors, before anything is loaded: the plane metric measures against the target's normals
        from .test import _ply_has_normals
        for name in args.input[:-1]:
            if not _ply_has_normals(name):
                ap.error("--metric=%s needs normals: %s has no nx ny nz properties (or cannot be read); pass --estimate_normals "
                         "to estimate them, or --metric=point" % (args.metric, name))
    if args.global_init and args.init is not None:
        ap.error("--global_init finds the start itself: not together with --init")
    for name in ("feature_voxel", "feature_radius", "corr_dist"):
        if not (np.isfinite(getattr(args, name)) and getattr(args, name) > 0):
            ap.error("--%s must be positive (got %r)" % (name, getattr(args, name)))
    if args.draws < 1 or args.seed < 0:
        ap.error("--draws must be at least 1 and --seed not negative")
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
        options = {"feature_voxel": args.feature_voxel, "radius": args.feature_radius, "corr_dist": args.corr_dist, "draws": args.draws,
                   "seed": args.seed}
        out = register_scans(scans, args.bits, args.voxel_size, args.metric, args.max_dist, args.iters, args.tol, init,
                             args.estimate_normals, args.clean, names=args.input, global_init=args.global_init,
                             global_options=options, smooth=args.smooth, color_weight=args.color_weight,
                             color_radius=args.color_radius, color_kmin=args.color_kmin)
    except ValueError as e:
        raise SystemExit("register: %s" % e)
    failed = []
    for name, r in list(zip(args.input, out["poses"]))[1:]:
        if "global" in r:
            print("register: {}: global start from draw {} of {} kept, {} inliers of {} matches".format(
                name, r["global"]["draw"], r["global"]["hypotheses"], r["global"]["inliers"], r["global"]["correspondences"]))
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
    if "smooth" in out:
        print(out["smooth"])
    print("wrote {}, {} and {}".format(args.output, ingest.frame_path(args.output), poses_path(args.output)))


if __name__ == "__main__":
    main()
