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
"""
from fractions import Fraction

import numpy as np

from . import _lib

RHOS_D1 = [0.8, 0.9, 1.0, 1.02, 1.05, 1.10, 1.15, 1.2, 1.25, 1.30, 1.40, 1.50, 1.75, 2.0, 2.5, 3.0]   # eval.RHOS_D1
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


class _Prepared(object):
    """Thresholds, counts and the chunk plan of one cube batch."""

    def __init__(self, cubes, logits, points_numbers):
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
        self.chunks, lo = [], 0
        while lo < B:                                 # greedy: cubes while the chunk's segment fits (one cube at least)
            hi, tot = lo + 1, int(self.n_seg[lo])
            while hi < B and tot + int(self.n_seg[hi]) <= _CHUNK_SEG:
                tot += int(self.n_seg[hi])
                hi += 1
            self.chunks.append((lo, hi))
            lo = hi

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
        _lib.check(lib.pcgc_pointnums_curves(_lib.dptr(self.x[lo:hi]), _lib.dptr(self.l[lo:hi]), _lib.dptr(self.thr[lo:hi]),
                                             hi - lo, self.cs, _lib.dptr(d["p"]), _lib.dptr(d["s"]), _lib.dptr(d["c"]),
                                             int(seg_off[-1]), int(pts_off[-1]), _lib.dptr(d["sb"]), len(sb) // 2,
                                             _lib.dptr(d["pb"]), len(pb) // 2, _lib.dptr(m), _lib.dptr(A), _lib.dptr(Bc),
                                             _lib.dptr(ws), ws.numel(), _lib.stream()), "pcgc_pointnums_curves")
        return d["c"]


def distortion_curves(cubes, logits, points_numbers):
    """-> (m int32, A int64, B int64, offsets int64 [B+1]): the curves of every cube, flat; cube b's k = 1 .. K_b are the
    entries offsets[b] .. offsets[b+1]-1.  m / A / B are device tensors, offsets a numpy array."""
    import torch
    p = _Prepared(cubes, logits, points_numbers)
    tot = int(p.curve_off[-1])
    m = torch.empty(tot, dtype=torch.int32, device=p.dev)
    A = torch.empty(tot, dtype=torch.int64, device=p.dev)
    Bc = torch.empty(tot, dtype=torch.int64, device=p.dev)
    for lo, hi in p.chunks:
        a, b = int(p.curve_off[lo]), int(p.curve_off[hi])
        p.curves(lo, hi, m[a:b], A[a:b], Bc[a:b])
    return m, A, Bc, p.curve_off


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


def optimize_points_numbers(cubes, logits, points_numbers, sweep=64, rhos=RHOS_D1, resolution=1023):
    """-> (counts uint16 [B], report).  Chunk by chunk: curves, then the sweep and the ladder on the device; the per-
    assignment sums are added up as Python integers and the selection (select_assignment) runs on the host.  report:
    {"choice": ("ladder", rho) or ("sweep", j), "F_count", "F_chosen" (floats), "psnr_count", "psnr_chosen" (local PSNR
    at `resolution`), "sum_n", "sums": {assignment: (sum A, sum B, sum m)}, "ks": every assignment's counts [n_assign, B]}."""
    import torch
    rhos = list(rhos)
    p = _Prepared(cubes, logits, points_numbers)
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
    report = {"choice": (kind, idx if kind == "sweep" else rhos[idx]), "F_chosen": float(f), "psnr_chosen": local_psnr(f, resolution),
              "F_count": None if f_count is None else float(f_count),
              "psnr_count": None if f_count is None else local_psnr(f_count, resolution), "sum_n": sum_n, "sums": sums,
              "ks": ks}
    return counts, report
