"""numpy restatement of pcgcv1_amd/pointnums.py's curves and sweep (csrc/pointnums.hip).

curves_ref ranks the voxels by (logit descending, index ascending), takes m(k) as the end of the tie group that holds
rank k-1, B from a prefix sum of per-voxel nearest distances and A from the running minimum of every occupied voxel's
distance over the ranked list.  curves_direct builds each mask the way the reference's decoder does,
`vol >= sorted(values)[-k]`, and measures it from scratch: the slow definition the fast forms are checked against.
"""
import numpy as np

from pcgcv1_amd.pointnums import candidate_counts


def _coords(idx, cs):
    return np.stack(np.unravel_index(np.asarray(idx, np.int64), (cs, cs, cs)), -1).astype(np.int64)


def _d2(p, v):
    return ((p[:, None, :] - v[None, :, :]) ** 2).sum(-1)


def curves_ref(x, logits, n, rows=512):
    """one cube: x, logits [cs,cs,cs(,1)], n the stored count -> (m int64 [K], A int64 [K], B int64 [K])"""
    lf = np.asarray(logits, np.float32).reshape(-1).copy()
    vox = lf.size
    cs = int(round(vox ** (1.0 / 3)))
    K = int(candidate_counts([n], vox)[0])
    lf[lf == 0] = 0.0                                             # -0.0 -> +0.0
    order = np.lexsort((np.arange(vox), -lf.astype(np.float64)))
    t = lf[order[K - 1]]
    M = int((lf >= t).sum())
    ranked = order[:M]
    vals = lf[ranked]
    gend = np.searchsorted(-vals, -vals, side="right")           # #(l >= vals[r])
    P = _coords(np.flatnonzero(np.asarray(x).reshape(-1) > 0), cs)
    V = _coords(ranked, cs)
    a_full = np.zeros(M, np.int64)
    d_b = np.full(M, np.iinfo(np.int64).max, np.int64) if len(P) else np.zeros(M, np.int64)
    for lo in range(0, len(P), rows):
        D = _d2(P[lo:lo + rows], V)
        a_full += np.minimum.accumulate(D, axis=1).sum(0)
        d_b = np.minimum(d_b, D.min(0))
    b_full = np.cumsum(d_b)
    m = gend[:K].astype(np.int64)
    return m, a_full[m - 1], b_full[m - 1]


def curves_direct(x, logits, ks):
    """the same quantities for the given k, each from the decoder's own mask"""
    l = np.asarray(logits, np.float32).reshape(-1)
    vox = l.size
    cs = int(round(vox ** (1.0 / 3)))
    P = _coords(np.flatnonzero(np.asarray(x).reshape(-1) > 0), cs)
    srt = np.sort(l)
    out = []
    for k in ks:
        mask = l >= srt[-int(k)]
        V = _coords(np.flatnonzero(mask), cs)
        A = B = 0
        for lo in range(0, len(P), 256):
            D = _d2(P[lo:lo + 256], V)
            A += int(D.min(1).sum())
        for lo in range(0, len(V), 256):
            D = _d2(V[lo:lo + 256], P) if len(P) else np.zeros((len(V[lo:lo + 256]), 1), np.int64)
            B += int(D.min(1).sum())
        out.append((int(mask.sum()), A, B))
    return out


def sweep_ref(curves, J=64, fixed=None):
    """curves: [(m, A, B)] per cube -> (k [n_assign, B], sums [n_assign, 3]) like pcgc_pointnums_sweep; fixed [L, B]
    are clamped to 1 .. K_b"""
    nb = len(curves)
    fixed = np.zeros((0, nb), np.int64) if fixed is None else np.asarray(fixed, np.int64).reshape(-1, nb)
    ks = np.zeros((J + 1 + len(fixed), nb), np.int64)
    for b, (m, A, B) in enumerate(curves):
        for j in range(J + 1):
            ks[j, b] = int(np.argmin(j * A.astype(np.int64) + (J - j) * B.astype(np.int64))) + 1
        for i in range(len(fixed)):
            ks[J + 1 + i, b] = min(max(int(fixed[i, b]), 1), len(m))
    sums = np.zeros((len(ks), 3), np.int64)
    for a in range(len(ks)):
        for b, (m, A, B) in enumerate(curves):
            k = ks[a, b] - 1
            sums[a] += (A[k], B[k], m[k])
    return ks, sums
