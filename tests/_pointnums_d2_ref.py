"""The definition, in numpy, of the point-to-plane (D2) curves behind `--pointnums d2` (pcgcv1_amd/pointnums.py,
csrc/pointnums.hip).  Everything after quantise_normals is integer arithmetic, so results are exact and order-free.

Per cube b, exactly as for D1 (tests/_pointnums_ref.py): P_b the occupied voxels, the voxels ranked by (logit descending,
voxel index ascending, -0.0 == +0.0), S_b(k) = { v : l_b[v] >= the k-th largest }, m_b(k) = |S_b(k)|, k = 1 .. K_b,
K_b = min(65535, 3 n_b) clamped to 1 .. voxels.  New:

  normal of an occupied voxel   input point i maps to (cube, voxel) as preprocess / pcgc_voxelize_points map it; a voxel
                                takes the normal of the lowest-index point that maps to it (voxel_normals_ref), quantised to
                                n_q = rint(1024 n / |n|), float64, half to even, int32 components; a zero or non-finite
                                normal gives (0, 0, 0)
  A side                        v*(p, k) = the voxel of S_b(k) at the smallest squared distance from p, ties to the lowest
                                rank (the running nearest changes only on a strict drop);
                                A2_b(k) = sum_p ((v* - p) . n_q(p))^2
  B side                        p*(v) = the occupied voxel nearest to v, ties to the smallest voxel index;
                                B2_b(k) = sum_{v in S_b(k)} ((p* - v) . n_q(p*))^2   (0 for an empty P_b)
  objective                     F2 = max(sum A2 / sum N, sum B2 / sum m), compared exactly as fractions (pointnums.cloud_f)
  candidates                    the sweep argmin_k j A2 + (64 - j) B2, j = 0 .. 64, ties to the smallest k
                                (_pointnums_ref.sweep_ref serves as it is), and the ladder eval.RHOS_D2 (it holds 1.0)
  ties in the choice            rho = 1, then the ladder in order, then ascending j (pointnums.select_assignment), hence
                                F2(chosen) <= F2(true counts) and <= F2 of every ladder entry
  overflow                      one term is at most 3 (cs - 1)^2 1026^2 (pointnums.plane_term_bound); the host cuts chunks so
                                that (points + segment voxels) times that stays below 2^62 (pointnums.chunk_plan); totals
                                across chunks are Python integers

F2 is cube-local, like F: the nearest voxel and its plane are searched inside the cube only, and with --scale != 1 the
measure is taken on the coded grid.  An exact half never arises in exact arithmetic (1024 n_x / |n| = j + 1/2 would need
(2 j + 1)^2 + b^2 + c^2 = 2048^2 up to scale, impossible modulo 8), but float64 can land on one; rint then goes to even.

curves_d2_ref is the fast form (one ranking, a signed difference array for A2, a prefix sum for B2); curves_d2_direct builds each mask as
the decoder does, `vol >= sorted(values)[-k]`, and measures both directions from scratch.
"""
import numpy as np

from pcgcv1_amd.pointnums import candidate_counts

from _pointnums_ref import _coords, _d2


def quantise_normals(normals):
    """float [n,3] -> int32 [n,3]: rint(1024 n / |n|) in float64 (half to even); zero / non-finite -> (0, 0, 0)"""
    n = np.asarray(normals, np.float32).reshape(-1, 3).astype(np.float64)
    with np.errstate(all="ignore"):
        ln = np.sqrt(n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2])
        ok = np.isfinite(n).all(1) & (ln > 0)
        q = np.rint(1024.0 * n / np.where(ok, ln, 1.0)[:, None])
    return np.where(ok[:, None], q, 0.0).astype(np.int32)


def voxel_normals_ref(keys, normals):
    """keys int64 [n] (cube * vox + voxel, < 0: dropped; pointnums.point_keys), normals [n,3] -> (distinct keys ascending,
    int32 [n_vox,3] quantised normal of each key's lowest-index point)"""
    keys = np.asarray(keys, np.int64)
    idx = np.flatnonzero(keys >= 0)
    uniq, first = np.unique(keys[idx], return_index=True)          # index of the first occurrence = the lowest input index
    return uniq, quantise_normals(np.asarray(normals).reshape(-1, 3)[idx[first]])


def _plane(d, n):
    """d [..., 3] int64 offsets, n [..., 3] int64 normals -> (d . n)^2"""
    return (d * n).sum(-1) ** 2


def _rank(logits, n):
    lf = np.asarray(logits, np.float32).reshape(-1).copy()
    vox = lf.size
    K = int(candidate_counts([n], vox)[0])
    lf[lf == 0] = 0.0                                              # -0.0 -> +0.0
    order = np.lexsort((np.arange(vox), -lf.astype(np.float64)))
    M = int((lf >= lf[order[K - 1]]).sum())
    ranked = order[:M]
    vals = lf[ranked]
    gend = np.searchsorted(-vals, -vals, side="right")            # #(l >= vals[r])
    return K, ranked, gend


def curves_d2_ref(x, logits, n, nq, rows=512):
    """one cube: x, logits [cs,cs,cs(,1)], n the stored count, nq int [N,3] the quantised normals of the occupied voxels in
    ascending voxel index -> (m int64 [K], A2 int64 [K], B2 int64 [K])"""
    vox = np.asarray(logits).size
    cs = int(round(vox ** (1.0 / 3)))
    K, ranked, gend = _rank(logits, n)
    M = len(ranked)
    P = _coords(np.flatnonzero(np.asarray(x).reshape(-1) > 0), cs)
    nq = np.asarray(nq, np.int64).reshape(-1, 3)
    assert len(nq) == len(P)
    V = _coords(ranked, cs)
    diff = np.zeros(M, np.int64)                                   # signed changes of A2 by rank
    best = np.full(M, np.iinfo(np.int64).max, np.int64)
    e_b = np.zeros(M, np.int64)
    for lo in range(0, len(P), rows):
        Pc, Nc = P[lo:lo + rows], nq[lo:lo + rows]
        D = _d2(Pc, V)                                                           # [p, rank]
        run = np.minimum.accumulate(D, axis=1)
        # the running nearest moves at rank 0 and wherever the running minimum drops strictly (a tie does not move it)
        drop = np.concatenate([np.ones((len(Pc), 1), bool), run[:, 1:] < run[:, :-1]], 1)
        pi, ri = np.nonzero(drop)                                                # row-major: per p, ranks ascending
        e = _plane(V[ri] - Pc[pi], Nc[pi])
        prev = np.where(ri == 0, 0, np.concatenate([[0], e[:-1]]))               # the same p's previous plane error
        np.add.at(diff, ri, e - prev)
        # B side: P is in ascending voxel index, argmin takes the first minimum; a later chunk wins only if strictly nearer
        j = D.argmin(0)
        d = D[j, np.arange(M)]
        better = d < best
        best = np.where(better, d, best)
        e_b = np.where(better, _plane(Pc[j] - V, Nc[j]), e_b)
    a_full = np.cumsum(diff)
    b_full = np.cumsum(e_b)
    m = gend[:K].astype(np.int64)
    return m, a_full[m - 1], b_full[m - 1]


def curves_d2_direct(x, logits, ks, nq):
    """[(m, A2, B2)] for the given k, each from the decoder's own mask, every nearest voxel searched anew.  The A side's tie
    rule needs the rank of the mask's voxels: (logit descending, index ascending) among the selected ones."""
    l = np.asarray(logits, np.float32).reshape(-1)
    vox = l.size
    cs = int(round(vox ** (1.0 / 3)))
    pidx = np.flatnonzero(np.asarray(x).reshape(-1) > 0)
    P = _coords(pidx, cs)
    nq = np.asarray(nq, np.int64).reshape(-1, 3)
    srt = np.sort(l)
    out = []
    for k in ks:
        mask = l >= srt[-int(k)]
        sel = np.flatnonzero(mask)
        key = l[sel].astype(np.float64) + 0.0                                    # -0.0 + 0.0 = +0.0
        sel = sel[np.lexsort((sel, -key))]                                       # rank order
        V = _coords(sel, cs)
        A = B = 0
        for i in range(len(P)):                                                  # v*: smallest distance, then lowest rank
            d = ((V - P[i]) ** 2).sum(-1)
            j = int(np.argmin(d))
            A += int(_plane(V[j] - P[i], nq[i]))
        if len(P):
            for v in V:                                                          # p*: smallest distance, then smallest index
                d = ((P - v) ** 2).sum(-1)
                j = int(np.argmin(d))
                B += int(_plane(P[j] - v, nq[j]))
        out.append((int(mask.sum()), A, B))
    return out
