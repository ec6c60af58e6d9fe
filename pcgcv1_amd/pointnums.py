"""Encoder-side choice of the per-cube point counts (`test.py compress --pointnums d1`).

The decoder turns each cube's logits into points with one rule: keep the voxels whose logit is >= the k-th largest, ties
included, with k = int(rho * pointnums[b]) (select_voxels / get_adaptive_thres, dataprocess/inout_points.py:147-179).  The
encoder writes `.pointnums`, so it may pick every cube's k such that the unchanged decoder at rho = 1 gives the smallest D1.

Per cube b (x_b the voxelised input, P_b its occupied voxels, N_b = |P_b|, l_b the decoded logits the decoder's synthesis
produces, n_b the stored count; coordinates are voxel indices inside the cube, distances squared integers):

    S_b(k) = { v : l_b[v] >= the k-th largest of l_b }      (-0.0 == +0.0), m_b(k) = |S_b(k)|
    A_b(k) = sum_{p in P_b} min_{v in S_b(k)} |p - v|^2      (the cube's mse1 numerator)
    B_b(k) = sum_{v in S_b(k)} min_{p in P_b} |v - p|^2      (the cube's mse2 numerator)

for k = 1 .. K_b, K_b = min(65535, 3 n_b) (the top of eval's RHOS_D1 ladder; the uint16 limit), at least 1 and at most
the cube's voxel count (a larger k selects every voxel, like the decoder's clamp).  The candidate assignments are the
sweep k_b(j) = argmin_k j A_b(k) + (J - j) B_b(k), j = 0 .. J (int64, ties to the smallest k), and the uniform ladder
k_b = clamp(int(rho n_b), 1, K_b) for rho in RHOS_D1 (rho = 1 is what `--pointnums count` writes).  The one chosen
minimises the cube-local cloud D1  F = max(sum A / sum N, sum B / sum m), compared exactly in integers; ties go to rho = 1,
then the ladder in order, then the sweep in ascending j.  So F(chosen) <= F(true counts) and <= F(any ladder rho).

F is cube-local: a voxel's nearest neighbour is searched inside its own cube only (a neighbour across a cube face is not
seen), and with --scale != 1 it is measured on the coded grid.  pc_error's whole-cloud D1 (metrics.d1_psnr) can
therefore rank two assignments differently; DESIGN.md §"Encoder-side point counts" has the measured table.

The curves and the sweep run on the device (csrc/pointnums.hip); the selection is a handful of Python integers.

metric="d2" (`--pointnums d2`) does the same for the point-to-plane error.  Every occupied voxel carries the normal of the
lowest-index input point that maps to it (the mapping of preprocess / pcgc_voxelize_points), quantised to
n_q = rint(1024 n / |n|) (float64, half to even, int32 components; a zero or non-finite normal gives (0, 0, 0)), so all that
follows is integer arithmetic again.  With v*(p, k) the voxel of S_b(k) nearest to p (ties: the lowest rank under logit
descending, voxel index ascending) and p*(v) the occupied voxel nearest to v (ties: the smallest voxel index),

    A2_b(k) = sum_{p in P_b} ((v*(p, k) - p) . n_q(p))^2          B2_b(k) = sum_{v in S_b(k)} ((p*(v) - v) . n_q(p*(v)))^2

replace A and B: F2 = max(sum A2 / sum N, sum B2 / sum m), the sweep argmin_k j A2 + (J - j) B2, the ladder eval.RHOS_D2
(which holds 1.0), the same tie rules, hence F2(chosen) <= F2(true counts) and <= F2(any ladder rho).  F2 carries the factor
1024^2 of the quantised normals; the report divides it out.  Like F, F2 is cube-local (a nearest neighbour or a plane across
a cube face is not seen) and is measured on the coded grid; pc_error's whole-cloud D2 (metrics.d2_metrics) also averages the
normals of all points that chose a decoded point, which F2 does not, so the two can rank assignments differently.  One term
is at most 3 (cs - 1)^2 1026^2: chunks are cut so that (points + segment voxels) times that stays below 2^62, and the
cross-chunk totals are Python integers.
"""
from fractions import Fraction

import numpy as np

from . import _lib

RHOS_D1 = [0.8, 0.9, 1.0, 1.02, 1.05, 1.10, 1.15, 1.2, 1.25, 1.30, 1.40, 1.50, 1.75, 2.0, 2.5, 3.0]   # eval.RHOS_D1
RHOS_D2 = [1.0, 0.98, 0.95, 0.92, 0.90, 0.88, 0.85, 0.82, 0.80, 0.75, 0.70, 0.65, 0.50, 0.40, 0.30]          # eval.RHOS_D2
NORMAL_ONE = 1024             # length of a quantised normal
K_CAP = 65535
_CHUNK_SEG = 1 << 23          # segment voxels per pcgc_pointnums_curves call (32 bytes each): bounds the workspace
_TILE = 256                   # elements per workgroup of the per-element kernels (csrc/pointnums.hip kTile)


def candidate_counts(points_numbers, vox):
    """K_b = min(65535, 3 n_b), clamped to 1 .. vox."""
    n = np.asarray(points_numbers).reshape(-1).astype(np.int64)
    return np.clip(np.minimum(3 * n, K_CAP), 1, max(1, min(K_CAP, int(vox)))).astype(np.int64)


def ladder_counts(points_numbers, k_max, rhos):
    """[len(rhos), B] int64: clamp(int(rho * n_b), 1, K_b) — int() of the product as select_voxels forms it."""
    n = np.asarray(points_numbers).reshape(-1)
    out = np.empty((len(rhos), len(n)), np.int64)
    for i, rho in enumerate(rhos):
        out[i] = [int(rho * np.array(v)) for v in n]
    return np.clip(out, 1, np.asarray(k_max, np.int64)[None, :])


def cloud_f(sum_a, sum_n, sum_b, sum_m):
    """F = max(sum A / sum N, sum B / sum m) as an exact fraction (a side with an empty denominator counts as 0)."""
    fa = Fraction(int(sum_a), int(sum_n)) if int(sum_n) > 0 else Fraction(0)
    fb = Fraction(int(sum_b), int(sum_m)) if int(sum_m) > 0 else Fraction(0)
    return max(fa, fb)


def local_psnr(f, resolution=1023):
    """10 log10(3 peak^2 / F), pc_error's form (inf for F = 0)."""
    f = float(f)
    return float("inf") if f == 0 else 10.0 * np.log10(3.0 * float(resolution) ** 2 / f)


def select_assignment(sweep_sums, ladder_sums, rhos, sum_n):
    """sweep_sums[j], ladder_sums[i]: (sum A, sum B, sum m) of sweep point j / ladder entry rhos[i].  -> (kind, index, F)
    with kind "ladder" or "sweep": the smallest F; ties to rho = 1, then the ladder in order, then ascending j."""
    order = []
    if 1.0 in rhos:
        order.append(("ladder", list(rhos).index(1.0)))
    order += [("ladder", i) for i in range(len(rhos)) if ("ladder", i) not in order]
    order += [("sweep", j) for j in range(len(sweep_sums))]
    best = None
    for kind, i in order:
        a, b, m = (ladder_sums if kind == "ladder" else sweep_sums)[i]
        f = cloud_f(a, sum_n, b, m)
        if best is None or f < best[2]:
            best = (kind, i, f)
    return best


def _flat(t, dev):
    import torch
    x = t if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t, np.float32))
    x = x.to(dev, torch.float32)
    B = int(x.shape[0])
    return x.reshape(B, -1).contiguous(), B


def _blocks(counts):
    """(cube, first element) pairs cutting every cube's `counts` elements into _TILE pieces, int32 flat."""
    counts = np.asarray(counts, np.int64)
    nb = (counts + _TILE - 1) // _TILE
    cube = np.repeat(np.arange(len(counts)), nb)
    first = np.arange(int(nb.sum())) - np.repeat(np.cumsum(nb) - nb, nb)
    return np.ascontiguousarray(np.stack([cube, first * _TILE], 1).astype(np.int32).reshape(-1))


def _offsets(counts):
    return np.concatenate([[0], np.cumsum(np.asarray(counts, np.int64))]).astype(np.int64)


def plane_term_bound(cube_size):
    """Upper bound of one plane-error term: |d|^2 |n_q|^2 <= 3 (cs - 1)^2 1026^2 (|n_q| <= 1024 + sqrt(3) / 2)."""
    return 3 * (int(cube_size) - 1) ** 2 * 1026 ** 2


def chunk_plan(n_seg, n_pts=None, chunk_seg=None, term_bound=None, limit=1 << 62):
    """[(lo, hi)]: greedy runs of cubes whose segment voxels fit chunk_seg (one cube at least).  With term_bound (the d2
    curves): a run also keeps (points + segment voxels) * term_bound below `limit`, so no int64 sum of a chunk can wrap."""
    chunk_seg = _CHUNK_SEG if chunk_seg is None else chunk_seg
    B = len(n_seg)
    elems = [int(n_seg[b]) + (int(n_pts[b]) if term_bound else 0) for b in range(B)]
    cap = (limit - 1) // term_bound if term_bound else None          # elements a chunk may hold
    chunks, lo = [], 0
    while lo < B:
        hi, tot, el = lo + 1, int(n_seg[lo]), elems[lo]
        while hi < B and tot + int(n_seg[hi]) <= chunk_seg and (cap is None or el + elems[hi] <= cap):
            tot += int(n_seg[hi])
            el += elems[hi]
            hi += 1
        chunks.append((lo, hi))
        lo = hi
    return chunks


class _Prepared(object):
    """Thresholds, counts and the chunk plan of one cube batch."""

    def __init__(self, cubes, logits, points_numbers, vox_normals=None):
        import torch
        self.dev = _lib.require_gpu()
        self.x, B = _flat(cubes, self.dev)
        self.l, B2 = _flat(logits, self.dev)
        if B != B2 or self.x.shape != self.l.shape:
            raise ValueError("cubes %s and logits %s differ in shape" % (tuple(self.x.shape), tuple(self.l.shape)))
        vox = int(self.x.shape[1])
        cs = int(round(vox ** (1.0 / 3)))
        if cs ** 3 != vox or cs > 256:
            raise ValueError("cubes of %d voxels are not cubes of edge <= 256" % vox)
        self.B, self.cs, self.vox = B, cs, vox
        nums = np.asarray(points_numbers).reshape(-1)
        if len(nums) != B:
            raise ValueError("%d point counts for %d cubes" % (len(nums), B))
        self.nums = nums
        self.k_max = candidate_counts(nums, vox)
        self.k_max_d = torch.from_numpy(self.k_max.astype(np.int32)).to(self.dev)
        self.thr = torch.empty(B, dtype=torch.float32, device=self.dev)
        n_pts = torch.empty(B, dtype=torch.int32, device=self.dev)
        n_seg = torch.empty(B, dtype=torch.int32, device=self.dev)
        if B:
            _lib.check(_lib.hip().pcgc_pointnums_count(_lib.dptr(self.x), _lib.dptr(self.l), _lib.dptr(self.k_max_d), B, cs,
                                                       _lib.dptr(self.thr), _lib.dptr(n_pts), _lib.dptr(n_seg), _lib.stream()),
                       "pcgc_pointnums_count")
        self.n_pts = n_pts.cpu().numpy().astype(np.int64)
        self.n_seg = n_seg.cpu().numpy().astype(np.int64)
        self.curve_off = _offsets(self.k_max)
        self.vn = None
        if vox_normals is not None:                   # the d2 curves: int16 [sum N_b, 4] in P's order (voxel_normals)
            vn = vox_normals if torch.is_tensor(vox_normals) else torch.from_numpy(np.ascontiguousarray(vox_normals, np.int16))
            vn = vn.to(self.dev, torch.int16).contiguous()
            if vn.dim() != 2 or vn.shape[1] != 4 or int(vn.shape[0]) != int(self.n_pts.sum()):
                raise ValueError("voxel normals %s for %d occupied voxels (expected int16 [%d, 4], pointnums.voxel_normals)"
                                 % (tuple(vn.shape), int(self.n_pts.sum()), int(self.n_pts.sum())))
            self.vn = vn
            self.pts_off = _offsets(self.n_pts)
        # greedy: cubes while the chunk's segment fits (one cube at least)
        self.chunks = chunk_plan(self.n_seg, self.n_pts, _CHUNK_SEG, plane_term_bound(cs) if self.vn is not None else None)

    def curves(self, lo, hi, m, A, Bc):
        """curves of cubes lo..hi into m / A / Bc (device views of the chunk's curve entries)"""
        import torch
        dev = self.dev
        pts_off, seg_off = _offsets(self.n_pts[lo:hi]), _offsets(self.n_seg[lo:hi])
        curve_off = _offsets(self.k_max[lo:hi])
        sb, pb = _blocks(self.n_seg[lo:hi]), _blocks(self.n_pts[lo:hi])
        d = {k: torch.from_numpy(v).to(dev) for k, v in (("p", pts_off), ("s", seg_off), ("c", curve_off), ("sb", sb), ("pb", pb))}
        lib = _lib.hip()
        ws = torch.empty(int(lib.pcgc_pointnums_curves_workspace_bytes(int(seg_off[-1]), int(pts_off[-1]))), dtype=torch.uint8,
                         device=dev)
        if self.vn is not None:
            vn = self.vn[int(self.pts_off[lo]):int(self.pts_off[hi])]
            _lib.check(lib.pcgc_pointnums_curves_d2(_lib.dptr(self.x[lo:hi]), _lib.dptr(self.l[lo:hi]), _lib.dptr(self.thr[lo:hi]),
                                                    _lib.dptr(vn) if vn.numel() else None, hi - lo, self.cs, _lib.dptr(d["p"]),
                                                    _lib.dptr(d["s"]), _lib.dptr(d["c"]), int(seg_off[-1]), int(pts_off[-1]),
                                                    _lib.dptr(d["sb"]), len(sb) // 2, _lib.dptr(d["pb"]), len(pb) // 2,
                                                    _lib.dptr(m), _lib.dptr(A), _lib.dptr(Bc), _lib.dptr(ws), ws.numel(),
                                                    _lib.stream()), "pcgc_pointnums_curves_d2")
            return d["c"]
        _lib.check(lib.pcgc_pointnums_curves(_lib.dptr(self.x[lo:hi]), _lib.dptr(self.l[lo:hi]), _lib.dptr(self.thr[lo:hi]),
                                             hi - lo, self.cs, _lib.dptr(d["p"]), _lib.dptr(d["s"]), _lib.dptr(d["c"]),
                                             int(seg_off[-1]), int(pts_off[-1]), _lib.dptr(d["sb"]), len(sb) // 2,
                                             _lib.dptr(d["pb"]), len(pb) // 2, _lib.dptr(m), _lib.dptr(A), _lib.dptr(Bc),
                                             _lib.dptr(ws), ws.numel(), _lib.stream()), "pcgc_pointnums_curves")
        return d["c"]


def distortion_curves(cubes, logits, points_numbers):
    """-> (m int32, A int64, B int64, offsets int64 [B+1]): the curves of every cube, flat; cube b's k = 1 .. K_b are the
    entries offsets[b] .. offsets[b+1]-1.  m / A / B are device tensors, offsets a numpy array."""
    return _all_curves(_Prepared(cubes, logits, points_numbers))


def _all_curves(p):
    import torch
    tot = int(p.curve_off[-1])
    m = torch.empty(tot, dtype=torch.int32, device=p.dev)
    A = torch.empty(tot, dtype=torch.int64, device=p.dev)
    Bc = torch.empty(tot, dtype=torch.int64, device=p.dev)
    for lo, hi in p.chunks:
        a, b = int(p.curve_off[lo]), int(p.curve_off[hi])
        p.curves(lo, hi, m[a:b], A[a:b], Bc[a:b])
    return m, A, Bc, p.curve_off


def point_keys(points, cube_positions, scale, cube_size):
    """int64 [n]: cube * cs^3 + voxel index of every input point, cubes in stored order (ordered_positions), or -1 for a point
    of a cube that was dropped — the mapping of process.preprocess_points (round(float32(p) * scale) when scale != 1, floor
    division by the cube size, row-major voxel index) for the points as given, duplicates included."""
    from .dataprocess.inout_points import ordered_positions
    points = np.asarray(points)
    if scale != 1:
        points = np.round(points.astype("float32") * scale)
    c = np.ascontiguousarray(points, np.int32).reshape(-1, 3).astype(np.int64)
    cs = int(cube_size)
    cube = np.floor_divide(c, cs)
    loc = c - cube * cs
    spos = np.asarray(ordered_positions(cube_positions), np.int64).reshape(-1, 3)
    if len(c) == 0 or len(spos) == 0:
        return np.full(len(c), -1, np.int64)
    lo = np.minimum(cube.min(0), spos.min(0))
    ext = np.maximum(cube.max(0), spos.max(0)) - lo + 1

    def flat(v):
        v = v - lo
        return (v[:, 0] * ext[1] + v[:, 1]) * ext[2] + v[:, 2]
    ck, pk = flat(spos), flat(cube)
    order = np.argsort(ck, kind="stable")
    at = np.minimum(np.searchsorted(ck[order], pk), len(ck) - 1)
    b = order[at]
    found = ck[b] == pk
    key = b.astype(np.int64) * cs ** 3 + (loc[:, 0] * cs + loc[:, 1]) * cs + loc[:, 2]
    return np.where(found, key, -1)


def voxel_normals(points, normals, cube_positions, scale, cube_size):
    """The quantised normal of every occupied voxel of the cubes preprocess makes of `points` -> int16 device tensor
    [sum N_b, 4] = (nx, ny, nz, 0), cubes in stored order, a cube's voxels in ascending voxel index (the P order of the
    curves).  A voxel takes the normal of the lowest-index input point that maps to it (point_keys), as
    rint(1024 n / |n|); a zero or non-finite normal gives (0, 0, 0).  No dense volume is built: the distinct keys are
    sorted, every point finds its voxel by bisection and leaves its index by an atomic min, a gather quantises."""
    import torch
    dev = _lib.require_gpu()
    keys = point_keys(points, cube_positions, scale, cube_size)
    nrm = np.ascontiguousarray(np.asarray(normals), np.float32).reshape(-1, 3)
    if len(nrm) != len(keys):
        raise ValueError("%d normals for %d points" % (len(nrm), len(keys)))
    keys_d = torch.from_numpy(keys).to(dev)
    nrm_d = torch.from_numpy(nrm).to(dev)
    vox_key = torch.unique(keys_d[keys_d >= 0], sorted=True).contiguous()
    n_vox = int(vox_key.numel())
    out = torch.zeros((n_vox, 4), dtype=torch.int16, device=dev)
    if n_vox:
        lib = _lib.hip()
        ws = torch.empty(int(lib.pcgc_pointnums_normals_workspace_bytes(n_vox)), dtype=torch.uint8, device=dev)
        _lib.check(lib.pcgc_pointnums_normals(_lib.dptr(keys_d), _lib.dptr(nrm_d), len(keys), _lib.dptr(vox_key), n_vox,
                                              _lib.dptr(out), _lib.dptr(ws), ws.numel(), _lib.stream()), "pcgc_pointnums_normals")
    return out


def distortion_curves_d2(cubes, logits, points_numbers, voxel_normals):
    """-> (m int32, A2 int64, B2 int64, offsets int64 [B+1]) in distortion_curves' layout: the point-to-plane curves, with
    voxel_normals the int16 [sum N_b, 4] tensor pointnums.voxel_normals returns for these cubes."""
    if voxel_normals is None:
        raise ValueError("distortion_curves_d2 needs the voxel normals (pointnums.voxel_normals)")
    return _all_curves(_Prepared(cubes, logits, points_numbers, voxel_normals))


def sweep_curves(m, A, Bc, offsets, sweep=64, fixed_k=None):
    """The device sweep over curves (distortion_curves' layout): -> (k [n_assign, B] int64, sums [n_assign, 3] int64) with
    n_assign = sweep + 1 + len(fixed_k); fixed_k [L, B]: given assignments (clamped to 1 .. K_b)."""
    import torch
    dev = m.device
    offsets = np.asarray(offsets, np.int64)
    B = len(offsets) - 1
    fk = np.zeros((0, B), np.int32) if fixed_k is None else np.ascontiguousarray(np.asarray(fixed_k).reshape(-1, B), np.int32)
    L = fk.shape[0]
    n_assign = sweep + 1 + L
    k_out = torch.empty((n_assign, B), dtype=torch.int32, device=dev)
    sums = torch.zeros((n_assign, 3), dtype=torch.int64, device=dev)
    if B == 0:
        return k_out.cpu().numpy().astype(np.int64), sums.cpu().numpy()
    lib = _lib.hip()
    ws = torch.empty(int(lib.pcgc_pointnums_sweep_workspace_bytes(B, n_assign)), dtype=torch.uint8, device=dev)
    off_d = torch.from_numpy(offsets).to(dev)
    fk_d = torch.from_numpy(fk).to(dev) if L else None
    _lib.check(lib.pcgc_pointnums_sweep(_lib.dptr(m), _lib.dptr(A), _lib.dptr(Bc), _lib.dptr(off_d), B, int(sweep),
                                        _lib.dptr(fk_d), L, _lib.dptr(k_out), _lib.dptr(sums), _lib.dptr(ws), ws.numel(),
                                        _lib.stream()), "pcgc_pointnums_sweep")
    return k_out.cpu().numpy().astype(np.int64), sums.cpu().numpy()


def optimize_points_numbers(cubes, logits, points_numbers, sweep=64, rhos=None, resolution=1023, metric="d1", normals=None):
    """-> (counts uint16 [B], report).  metric="d1" (rhos: RHOS_D1 unless given) minimises F; metric="d2" (rhos: RHOS_D2)
    minimises F2 over the point-to-plane curves and needs normals = pointnums.voxel_normals(...) of these cubes; its report
    has the same keys with F2 / 1024^2 (voxel units) as F and the sums of A2, B2 (with the 1024^2 factor) and m.
      Chunk by chunk: curves, then the sweep and the ladder on the device; the per-
    assignment sums are added up as Python integers and the selection (select_assignment) runs on the host.  report:
    {"choice": ("ladder", rho) or ("sweep", j), "F_count", "F_chosen" (floats), "psnr_count", "psnr_chosen" (local PSNR
    at `resolution`), "sum_n", "sums": {assignment: (sum A, sum B, sum m)}, "ks": every assignment's counts [n_assign, B]}."""
    import torch
    if metric not in ("d1", "d2"):
        raise ValueError("optimize_points_numbers: metric must be 'd1' or 'd2' (got %r)" % (metric,))
    if metric == "d2" and normals is None:
        raise ValueError("optimize_points_numbers: metric='d2' needs normals=pointnums.voxel_normals(...)")
    if metric == "d1" and normals is not None:
        raise ValueError("optimize_points_numbers: normals belong to metric='d2'")
    rhos = list((RHOS_D1 if metric == "d1" else RHOS_D2) if rhos is None else rhos)
    p = _Prepared(cubes, logits, points_numbers, normals)
    unit = 1 if metric == "d1" else NORMAL_ONE ** 2
    ladder = ladder_counts(p.nums, p.k_max, rhos)
    n_assign = sweep + 1 + len(rhos)
    totals = [[0, 0, 0] for _ in range(n_assign)]
    ks = np.zeros((n_assign, p.B), np.int64)
    for lo, hi in p.chunks:
        a, b = int(p.curve_off[lo]), int(p.curve_off[hi])
        m = torch.empty(b - a, dtype=torch.int32, device=p.dev)
        A = torch.empty(b - a, dtype=torch.int64, device=p.dev)
        Bc = torch.empty(b - a, dtype=torch.int64, device=p.dev)
        p.curves(lo, hi, m, A, Bc)
        k, s = sweep_curves(m, A, Bc, p.curve_off[lo:hi + 1] - a, sweep, ladder[:, lo:hi])
        ks[:, lo:hi] = k
        for i in range(n_assign):
            for q in range(3):
                totals[i][q] += int(s[i, q])
    sum_n = int(p.n_pts.sum())
    sweep_sums, ladder_sums = totals[:sweep + 1], totals[sweep + 1:]
    kind, idx, f = select_assignment(sweep_sums, ladder_sums, rhos, sum_n)
    row = idx if kind == "sweep" else sweep + 1 + idx
    counts = ks[row].astype(np.uint16)
    i1 = rhos.index(1.0) if 1.0 in rhos else None
    f_count = cloud_f(ladder_sums[i1][0], sum_n, ladder_sums[i1][1], ladder_sums[i1][2]) if i1 is not None else None
    sums = {("sweep", j): tuple(sweep_sums[j]) for j in range(sweep + 1)}
    sums.update({("ladder", rhos[i]): tuple(ladder_sums[i]) for i in range(len(rhos))})
    f, f_count = f / unit, None if f_count is None else f_count / unit
    report = {"choice": (kind, idx if kind == "sweep" else rhos[idx]), "F_chosen": float(f), "psnr_chosen": local_psnr(f, resolution),
              "F_count": None if f_count is None else float(f_count),
              "psnr_count": None if f_count is None else local_psnr(f_count, resolution), "sum_n": sum_n, "sums": sums,
              "ks": ks}
    return counts, report
