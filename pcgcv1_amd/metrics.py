"""Rate / distortion figures of the reference's eval path (eval.py:102-111 bpp, 194-207 D1 via myutils/pc_error_d).

`d1_psnr(a, b, resolution)` reproduces what MPEG pc_error 0.13.4 prints as "mseF,PSNR (p2point)" for two
voxelised clouds: mse1 = mean_{p in A} min_{q in B} |p-q|^2, mse2 the same B->A, mseF = max, PSNR =
10 log10(3 peak^2 / mseF).  The nearest-neighbour search runs on the device (pcgc_d1_mse); the prebuilt
pc_error_d binary cannot ship, its answers on seeded clouds are pinned in tests/golden/pc_error_d1.npz.
`d2_metrics` adds the point-to-plane figures ("mseF,PSNR (p2plane)", eval.py's D2) with pc_error's tie handling
and normal transfer (csrc/tail.hip), pinned in tests/golden/pc_error_d2.npz.
`color_metrics` is the tool's `--color=1` table (csrc/color.hip), pinned in tests/golden/pc_error_color.npz.
`mesh_error` measures a cloud against a triangle mesh: the exact distance from every point to the nearest triangle
(csrc/meshdist.hip), held to tests/_mesh_error_ref.py bit for bit.
"""
import numpy as np
import torch

from . import _lib
from .cells import cell_keys


GRID_MAX_RES = 4096               # cells per axis of the largest voxel grid pcgc_d1_mse, pcgc_d2_*, pcgc_color_mse and pcgc_recolor take


def check_grid_range(what, *clouds):
    """ValueError unless every coordinate of every cloud lies within [0, GRID_MAX_RES): beyond it the library has only its
    "bad arguments" to say.  Host arithmetic on the caller's arrays, before anything touches the device."""
    lo = min(int(np.min(c)) for c in clouds)
    hi = max(int(np.max(c)) for c in clouds)
    if lo < 0 or hi >= GRID_MAX_RES:
        raise ValueError("%s: coordinates must lie within [0, %d) (got %d .. %d)" % (what, GRID_MAX_RES, lo, hi))


def _d1_one_way(a_d, b_d, res, ws):
    out = torch.empty(2, dtype=torch.float64, device=a_d.device)
    _lib.check(_lib.hip().pcgc_d1_mse(_lib.dptr(a_d), a_d.shape[0], _lib.dptr(b_d), b_d.shape[0], res, _lib.dptr(out),
                                      _lib.dptr(ws), ws.numel(), _lib.stream()), "pcgc_d1_mse")
    mse, h2 = (float(v) for v in out.cpu().numpy())
    return mse, h2


def d1_metrics(points_a, points_b, resolution):
    """resolution = peak value (pc_error -r), e.g. 1023 for a 10-bit cloud.  Returns a dict with the pc_error keys."""
    check_grid_range("d1_metrics", points_a, points_b)
    dev = _lib.require_gpu()
    res = int(max(int(np.max(points_a)), int(np.max(points_b))) + 1)
    a_d = torch.from_numpy(np.ascontiguousarray(points_a, np.int32)).to(dev)
    b_d = torch.from_numpy(np.ascontiguousarray(points_b, np.int32)).to(dev)
    ws = torch.empty(int(_lib.hip().pcgc_d1_workspace_bytes(res)), dtype=torch.uint8, device=dev)
    mse1, h1 = _d1_one_way(a_d, b_d, res, ws)
    mse2, h2 = _d1_one_way(b_d, a_d, res, ws)
    mse_f = max(mse1, mse2)
    peak = float(resolution)

    def psnr(m):
        return float("inf") if m == 0 else 10.0 * np.log10(3.0 * peak * peak / m)
    return {"mse1      (p2point)": mse1, "mse2      (p2point)": mse2, "mseF      (p2point)": mse_f,
            "mse1,PSNR (p2point)": psnr(mse1), "mse2,PSNR (p2point)": psnr(mse2), "mseF,PSNR (p2point)": psnr(mse_f),
            "h.       1(p2point)": h1, "h.       2(p2point)": h2, "h.        (p2point)": max(h1, h2)}


def d1_psnr(points_a, points_b, resolution):
    return d1_metrics(points_a, points_b, resolution)["mseF,PSNR (p2point)"]


def _sorted_keys(points_d, res):
    p = points_d.to(torch.int64)
    keys = (p[:, 0] * res + p[:, 1]) * res + p[:, 2]
    keys, order = torch.sort(keys)
    if keys.numel() > 1 and bool((keys[1:] == keys[:-1]).any()):
        raise ValueError("point cloud holds duplicate points (pc_error drops them first; pass unique voxels)")
    return keys.contiguous(), order


def d2_metrics(points_a, normals_a, points_b, resolution):
    """Point-to-plane (D2) figures of `pc_error -a A -b B -n A` (myutils/pc_error_wrapper.py:46-51): A carries
    normals, B (the decoded cloud) receives them from A.  Returns the p2plane keys of the wrapper's table."""
    check_grid_range("d2_metrics", points_a, points_b)
    dev = _lib.require_gpu()
    lib = _lib.hip()
    res = int(max(int(np.max(points_a)), int(np.max(points_b))) + 1)
    a_d = torch.from_numpy(np.ascontiguousarray(points_a, np.int32)).to(dev)
    b_d = torch.from_numpy(np.ascontiguousarray(points_b, np.int32)).to(dev)
    na_d = torch.from_numpy(np.ascontiguousarray(normals_a, np.float32)).to(dev)
    ka, oa = _sorted_keys(a_d, res)
    kb, ob = _sorted_keys(b_d, res)
    a_s, na_s, b_s = a_d[oa].contiguous(), na_d[oa].contiguous(), b_d[ob].contiguous()
    ws = torch.empty(int(lib.pcgc_d2_workspace_bytes(res, max(len(ka), len(kb)))), dtype=torch.uint8, device=dev)
    nb_s = torch.empty((len(kb), 3), dtype=torch.float32, device=dev)
    _lib.check(lib.pcgc_d2_transfer_normals(_lib.dptr(a_s), len(ka), _lib.dptr(na_s), _lib.dptr(kb), len(kb), res, _lib.dptr(nb_s),
                                            _lib.dptr(ws), ws.numel(), _lib.stream()), "pcgc_d2_transfer_normals")
    out = torch.empty(4, dtype=torch.float64, device=dev)
    _lib.check(lib.pcgc_d2_mse(_lib.dptr(a_s), len(ka), _lib.dptr(kb), len(kb), _lib.dptr(nb_s), res, _lib.dptr(out),
                               _lib.dptr(ws), ws.numel(), _lib.stream()), "pcgc_d2_mse A->B")
    _lib.check(lib.pcgc_d2_mse(_lib.dptr(b_s), len(kb), _lib.dptr(ka), len(ka), _lib.dptr(na_s), res, _lib.dptr(out[2:]),
                               _lib.dptr(ws), ws.numel(), _lib.stream()), "pcgc_d2_mse B->A")
    mse1, h1, mse2, h2 = (float(v) for v in out.cpu().numpy())
    mse_f, peak = max(mse1, mse2), float(resolution)

    def psnr(m):
        return float("inf") if m == 0 else 10.0 * np.log10(3.0 * peak * peak / m)
    return {"mse1      (p2plane)": mse1, "mse2      (p2plane)": mse2, "mseF      (p2plane)": mse_f,
            "mse1,PSNR (p2plane)": psnr(mse1), "mse2,PSNR (p2plane)": psnr(mse2), "mseF,PSNR (p2plane)": psnr(mse_f),
            "h.       1(p2plane)": h1, "h.       2(p2plane)": h2, "h.        (p2plane)": max(h1, h2)}


def _colored_cloud(points, colors, res, what):
    """device copies of a voxelised coloured cloud, checked for what the kernels assume: coordinates within [0, res), no
    point twice (pc_error drops duplicates first; which colour it keeps is not part of the stated rule)"""
    pts = np.ascontiguousarray(points, np.int32).reshape(-1, 3)
    col = np.ascontiguousarray(colors, np.uint8).reshape(-1, 3)
    if len(pts) == 0 or len(pts) != len(col):
        raise ValueError("%s: %d points, %d colours" % (what, len(pts), len(col)))
    if int(pts.min()) < 0 or int(pts.max()) >= res:
        raise ValueError("%s: coordinates outside [0, %d)" % (what, res))
    dev = _lib.require_gpu()
    p_d = torch.from_numpy(pts).to(dev)
    _sorted_keys(p_d, res)                                    # raises on duplicate points
    return p_d, torch.from_numpy(col).to(dev)


def color_metrics(points_a, colors_a, points_b, colors_b):
    """The colour figures `pc_error --color=1` (0.13.4) prints for two voxelised clouds with uint8 rgb per point, under its
    own keys: "c[i],    1" = mean over A of (yuv_a[i] - yuv_m[i])^2 with m the rounded-half-up integer mean colour of ALL
    nearest points of B and yuv = BT.709 of rgb / 255, "c[i],PSNR1" = -10 log10 of it, the 2 forms with A and B swapped,
    the F forms the larger mse (smaller PSNR) per channel (include/pcgc.h, pcgc_color_mse; pinned against the pc_error
    binary in tests/golden/pc_error_color.npz).  The tool's h.c[i] lines are not produced."""
    check_grid_range("color_metrics", points_a, points_b)
    lib = _lib.hip()
    res = int(max(int(np.max(points_a)), int(np.max(points_b))) + 1)
    pa, ca = _colored_cloud(points_a, colors_a, res, "color_metrics: cloud A")
    pb, cb = _colored_cloud(points_b, colors_b, res, "color_metrics: cloud B")
    out = torch.empty(6, dtype=torch.float64, device=pa.device)
    ws = torch.empty(int(lib.pcgc_color_mse_workspace_bytes(res, max(len(pa), len(pb)))), dtype=torch.uint8, device=pa.device)
    _lib.check(lib.pcgc_color_mse(_lib.dptr(pa), _lib.dptr(ca), len(pa), _lib.dptr(pb), _lib.dptr(cb), len(pb), res, _lib.dptr(out),
                                  _lib.dptr(ws), ws.numel(), _lib.stream()), "pcgc_color_mse A->B")
    _lib.check(lib.pcgc_color_mse(_lib.dptr(pb), _lib.dptr(cb), len(pb), _lib.dptr(pa), _lib.dptr(ca), len(pa), res, _lib.dptr(out[3:]),
                                  _lib.dptr(ws), ws.numel(), _lib.stream()), "pcgc_color_mse B->A")
    m = out.cpu().numpy()
    res_ = {}
    for d, mse in (("1", m[:3]), ("2", m[3:]), ("F", np.maximum(m[:3], m[3:]))):
        for i in range(3):
            res_["c[%d],    %s" % (i, d)] = float(mse[i])
            res_["c[%d],PSNR%s" % (i, d)] = float("inf") if mse[i] == 0 else float(-10.0 * np.log10(mse[i]))
    return res_


def estimate_normals(points, radius=10, max_nn=20, return_cov=False):
    """Normals of a voxelised cloud, as mesh2pc_open3d.py:75-78 writes them with
    estimate_normals(KDTreeSearchParamHybrid(radius=10, max_nn=20)): the first max_nn occupied cells of the offsets
    within `radius` sorted by (|d|^2, dx, dy, dz), the smallest eigenvector of their integer covariance, first
    significant component positive (include/pcgc.h, pcgc_estimate_normals).  points: int [N,3] >= 0 (numpy, or an int32
    device tensor); -> float32 [N,3] numpy in input order.  return_cov=True also returns the covariance matrices
    K sum d d^T - (sum d)(sum d)^T as int64 [N,6] (c00 c01 c02 c11 c12 c22) and the neighbour counts K int32 [N]."""
    dev = _lib.require_gpu()
    lib = _lib.hip()
    p_d = points if torch.is_tensor(points) else torch.from_numpy(np.ascontiguousarray(points, np.int32).reshape(-1, 3))
    p_d = p_d.to(device=dev, dtype=torch.int32).reshape(-1, 3).contiguous()
    n = int(p_d.shape[0])
    if not (0.0 <= float(radius) <= 16.0) or not (1 <= int(max_nn) <= 64):
        raise ValueError("estimate_normals: radius must be within [0, 16] and max_nn within [1, 64]")
    if n == 0:
        empty = np.zeros((0, 3), np.float32)
        return (empty, np.zeros((0, 6), np.int64), np.zeros(0, np.int32)) if return_cov else empty
    lo, hi = (int(v) for v in torch.stack([p_d.min(), p_d.max()]).cpu())
    if lo < 0 or hi >= 4096:
        raise ValueError("estimate_normals: coordinates must lie within [0, 4096) (got %d .. %d)" % (lo, hi))
    res = hi + 1
    ws = torch.empty(int(lib.pcgc_normals_workspace_bytes(res, n, float(radius))), dtype=torch.uint8, device=dev)
    nrm = torch.empty((n, 3), dtype=torch.float32, device=dev)
    cov = torch.empty((n, 6), dtype=torch.int64, device=dev) if return_cov else None
    k = torch.empty(n, dtype=torch.int32, device=dev) if return_cov else None
    _lib.check(lib.pcgc_estimate_normals(_lib.dptr(p_d), n, res, float(radius), int(max_nn), _lib.dptr(nrm), _lib.dptr(cov),
                                         _lib.dptr(k), _lib.dptr(ws), ws.numel(), _lib.stream()), "pcgc_estimate_normals")
    if return_cov:
        return nrm.cpu().numpy(), cov.cpu().numpy(), k.cpu().numpy()
    return nrm.cpu().numpy()

def _off_grid(points):
    p = np.asarray(points)
    return np.issubdtype(p.dtype, np.floating) and bool((p != np.rint(p)).any())


def pc_error_off_grid(points_a, points_b, normals_a=None, resolution=1023):
    """The same figures when the decoded cloud B is NOT on the integer grid: a rate point with scale != 1 (R1 = 5/8) is
    scaled back by 1 / scale as float32 and written as text (process.py:76-77), and pc_error measures those coordinates —
    rounding them first moves D1 by a whole dB.  The kernels of d1_metrics / d2_metrics search a voxel bitmap and cannot
    hold such a cloud; this path is a k-d tree on the host (scipy, float64 like pc_error, at most 8 ties per point), and
    pc_error_float is the same rule on the device.  Same definitions as d1_metrics / d2_metrics: T(p) = every target point at the minimal distance,
    B's normals transferred from A as the plain mean over the points that chose it.  Pinned against the prebuilt pc_error_d
    on the config-3 frame's R1 section (tests/golden/oracle_a0.75b3_cloud2000_s0.625.npz)."""
    from scipy.spatial import cKDTree
    a = np.asarray(points_a, np.float64)
    b = np.unique(np.asarray(points_b, np.float32), axis=0).astype(np.float64)          # pc_error drops duplicate points
    peak = float(resolution)

    def psnr(m):
        return float("inf") if m == 0 else 10.0 * np.log10(3.0 * peak * peak / m)

    def tied(src, tree, k=8):
        """-> (squared NN distance per source point, list of (source index, target index) pairs of every tied nearest neighbour)"""
        d, idx = tree.query(src, k=k)
        d2 = d * d
        # pc_error's tie rule, pinned on the goldens: squared distances within 1e-8 (absolute, float64) of the minimum
        # (scale 3/4: |2 - 1.3333334| and |2.6666667 - 2| differ by 1e-7 and are NOT tied; 5.3333335 / 6.6666665 around 6 are)
        tie = np.abs(d2 - d2[:, :1]) < 1e-8                   # the first column is the minimum
        tie &= np.isfinite(d2)
        rows = np.nonzero(tie)
        return d2[:, 0], rows[0], idx[rows]
    tree_a, tree_b = cKDTree(a), cKDTree(b)
    d2_ab, ia, jb = tied(a, tree_b)
    d2_ba, ib, ja = tied(b, tree_a)
    mse1, mse2 = float(d2_ab.mean()), float(d2_ba.mean())
    out = {"mse1      (p2point)": mse1, "mse2      (p2point)": mse2, "mseF      (p2point)": max(mse1, mse2),
           "mse1,PSNR (p2point)": psnr(mse1), "mse2,PSNR (p2point)": psnr(mse2), "mseF,PSNR (p2point)": psnr(max(mse1, mse2)),
           "h.       1(p2point)": float(d2_ab.max()), "h.       2(p2point)": float(d2_ba.max()),
           "h.        (p2point)": float(max(d2_ab.max(), d2_ba.max()))}
    if normals_a is not None:
        na = np.asarray(normals_a, np.float64)
        nb = np.zeros((len(b), 3))
        cnt = np.zeros(len(b))
        np.add.at(nb, jb, na[ia])
        np.add.at(cnt, jb, 1.0)
        nb[cnt > 0] /= cnt[cnt > 0, None]

        def plane(src, dst, n_dst, i_src, j_dst):
            e = ((src[i_src] - dst[j_dst]) * n_dst[j_dst]).sum(1) ** 2
            tot, c = np.zeros(len(src)), np.zeros(len(src))
            np.add.at(tot, i_src, e)
            np.add.at(c, i_src, 1.0)
            return tot / c
        p1, p2 = plane(a, b, nb, ia, jb), plane(b, a, na, ib, ja)
        m1, m2 = float(p1.mean()), float(p2.mean())
        out.update({"mse1      (p2plane)": m1, "mse2      (p2plane)": m2, "mseF      (p2plane)": max(m1, m2),
                    "mse1,PSNR (p2plane)": psnr(m1), "mse2,PSNR (p2plane)": psnr(m2), "mseF,PSNR (p2plane)": psnr(max(m1, m2)),
                    "h.       1(p2plane)": float(p1.max()), "h.       2(p2plane)": float(p2.max()),
                    "h.        (p2plane)": float(max(p1.max(), p2.max()))})
    return out


OFFGRID_MAX_CELLS = 1024          # cells per axis of the device search's grid (csrc/offgrid.hip)
OFFGRID_MAX_EDGE = 2.0 ** 20      # its largest cell edge
OFFGRID_MAX_CELL = 2 ** 28        # |floor(x / edge)| of every coordinate of either cloud stays below this (|cell - origin| < 2^29)


def _offgrid_cells(target, source):
    """-> (h, origin [3], res) of the grid pcgc_offgrid_* searches `target` (float32 [N,3]) in: the smallest power of two
    h >= 1 with at most OFFGRID_MAX_CELLS cells of edge h per axis between the target's extremes; sized from the data."""
    ends = [np.stack([x.min(0), x.max(0)]).astype(np.float64) for x in (target, source)]       # a NaN anywhere shows in them
    if not all(np.isfinite(e).all() for e in ends):
        raise ValueError("pc_error_float: coordinates must be finite")
    lo, hi = ends[0]
    h = 1.0
    while int((np.floor(hi / h) - np.floor(lo / h)).max()) + 1 > OFFGRID_MAX_CELLS:
        h *= 2.0
        if h > OFFGRID_MAX_EDGE:
            raise ValueError("pc_error_float: a cloud of extent %g needs cells wider than 2^20 to fit %d cells per axis; the "
                             "device search supports a cell edge of at most 2^20" % (float((hi - lo).max()), OFFGRID_MAX_CELLS))
    origin = np.floor(lo / h)
    far = max(float(np.abs(np.floor(e / h)).max()) for e in ends)          # floor is monotone: the extremes bound every cell
    if far >= OFFGRID_MAX_CELL:
        raise ValueError("pc_error_float: coordinate / cell edge reaches %g; the device search supports less than 2^28 cells "
                         "from zero (cell edge %g)" % (far, h))
    return h, origin.astype(np.int64), int((np.floor(hi / h) - origin).max()) + 1


class _OffgridTarget:
    """a cloud as pcgc_offgrid_* searches it: its cell rule against one source cloud, and its points sorted by cell key"""

    def __init__(self, target, source, dev):
        self.h, origin, self.res = _offgrid_cells(target, source)
        self.origin = [int(v) for v in origin]
        q = torch.from_numpy(target).to(dev)
        # every row is finite and lies inside (the cells come from the target's extremes), so no treatment of outside rows
        # applies; clamp=True is the one with fewer device operations
        self.order = torch.sort(cell_keys(q, self.grid(), clamp=True), stable=True)[1]
        self.points = q[self.order].contiguous()

    def grid(self):
        return (self.h, self.origin[0], self.origin[1], self.origin[2], self.res)


def _offgrid_mse(p_d, target, normals_t, ws, per_point=False):
    """pcgc_offgrid_mse of the device cloud p_d against an _OffgridTarget (normals_t: float64 device tensor in the target's
    sorted order, or None) -> the four figures; per_point=True: also (best, plane, n_ties) numpy arrays per point of p_d"""
    dev, n = p_d.device, p_d.shape[0]
    out = torch.empty(4, dtype=torch.float64, device=dev)
    best = torch.empty(n, dtype=torch.float64, device=dev) if per_point else None
    plane = torch.empty(n, dtype=torch.float64, device=dev) if per_point else None
    ties = torch.empty(n, dtype=torch.int32, device=dev) if per_point else None
    _lib.check(_lib.hip().pcgc_offgrid_mse(_lib.dptr(p_d), n, _lib.dptr(target.points), target.points.shape[0], _lib.dptr(normals_t),
                                           *target.grid(), _lib.dptr(out), _lib.dptr(best), _lib.dptr(plane), _lib.dptr(ties),
                                           _lib.dptr(ws), ws.numel(), _lib.stream()), "pcgc_offgrid_mse")
    figures = [float(v) for v in out.cpu().numpy()]
    if any(np.isnan(figures)):
        raise RuntimeError("pcgc_offgrid_mse: the clouds break the cell rule (include/pcgc.h)")
    if per_point:
        return figures, (best.cpu().numpy(), plane.cpu().numpy(), ties.cpu().numpy())
    return figures


def _offgrid_transfer(p_d, normals_p, target, ws):
    """pcgc_offgrid_transfer_normals: float64 device tensor [n_target, 3] in the target's sorted order"""
    out = torch.empty((target.points.shape[0], 3), dtype=torch.float64, device=p_d.device)
    _lib.check(_lib.hip().pcgc_offgrid_transfer_normals(_lib.dptr(p_d), p_d.shape[0], _lib.dptr(normals_p), _lib.dptr(target.points),
                                                        target.points.shape[0], *target.grid(), _lib.dptr(out), _lib.dptr(ws),
                                                        ws.numel(), _lib.stream()), "pcgc_offgrid_transfer_normals")
    return out


def _float32_cloud(points, what):
    p = np.asarray(points)
    p32 = np.ascontiguousarray(p, np.float32).reshape(-1, 3)
    if len(p32) == 0 or not np.array_equal(p32.astype(np.float64), np.asarray(p, np.float64).reshape(-1, 3)):
        raise ValueError("pc_error_float: %s must be a non-empty cloud of float32-representable coordinates" % what)
    return p32


def pc_error_float(points_a, points_b, normals_a=None, resolution=1023, per_point=False):
    """pc_error_off_grid on the device (csrc/offgrid.hip; include/pcgc.h, pcgc_offgrid_*): the same keys and the same rule
    for two clouds of any float32-representable coordinates, integral or not, neither of them voxelised.  B loses its
    duplicate points (np.unique of the float32 rows, as the host path does), A is taken as it is.  Every tied nearest
    neighbour counts (squared distances within 1e-8 of the minimum), however many there are; no scipy.
    Raises ValueError when a cloud's extent / 1024 needs a cell edge above 2^20, the widest the search supports.
    per_point=True: -> (dict, {"1": (best, plane, n_ties) per point of A, "2": the same per point of the deduplicated B in
    np.unique's order, "normals_b": the normals B received, float64, in that order})."""
    dev = _lib.require_gpu()
    a = _float32_cloud(points_a, "cloud A")
    b = np.unique(_float32_cloud(points_b, "cloud B"), axis=0)
    tb, ta = _OffgridTarget(b, a, dev), _OffgridTarget(a, b, dev)
    lib = _lib.hip()
    ws = torch.empty(int(max(lib.pcgc_offgrid_workspace_bytes(tb.res, len(b)), lib.pcgc_offgrid_workspace_bytes(ta.res, len(a)))),
                     dtype=torch.uint8, device=dev)
    a_d, b_d = ta.points, tb.points                           # either order of a source cloud gives the same sums: use the sorted
    nb_d = na_d = None
    if normals_a is not None:
        na = np.ascontiguousarray(normals_a, np.float32).reshape(-1, 3)
        if len(na) != len(a):
            raise ValueError("pc_error_float: %d normals for %d points" % (len(na), len(a)))
        na32 = torch.from_numpy(na).to(dev)[ta.order].contiguous()
        nb_d, na_d = _offgrid_transfer(a_d, na32, tb, ws), na32.to(torch.float64)
    peak = float(resolution)

    def psnr(m):
        return float("inf") if m == 0 else 10.0 * np.log10(3.0 * peak * peak / m)
    r1 = _offgrid_mse(a_d, tb, nb_d, ws, per_point)
    r2 = _offgrid_mse(b_d, ta, na_d, ws, per_point)
    (mse1, h1, m1, p1), (mse2, h2, m2, p2) = (r1[0], r2[0]) if per_point else (r1, r2)
    out = {"mse1      (p2point)": mse1, "mse2      (p2point)": mse2, "mseF      (p2point)": max(mse1, mse2),
           "mse1,PSNR (p2point)": psnr(mse1), "mse2,PSNR (p2point)": psnr(mse2), "mseF,PSNR (p2point)": psnr(max(mse1, mse2)),
           "h.       1(p2point)": h1, "h.       2(p2point)": h2, "h.        (p2point)": max(h1, h2)}
    if normals_a is not None:
        out.update({"mse1      (p2plane)": m1, "mse2      (p2plane)": m2, "mseF      (p2plane)": max(m1, m2),
                    "mse1,PSNR (p2plane)": psnr(m1), "mse2,PSNR (p2plane)": psnr(m2), "mseF,PSNR (p2plane)": psnr(max(m1, m2)),
                    "h.       1(p2plane)": p1, "h.       2(p2plane)": p2, "h.        (p2plane)": max(p1, p2)})
    if not per_point:
        return out

    def unsort(values, order):                                # per-point arrays back from the sorted order to the caller's
        back = np.empty_like(values)
        back[order.cpu().numpy()] = values
        return back
    detail = {"1": tuple(unsort(v, ta.order) for v in r1[1]), "2": tuple(unsort(v, tb.order) for v in r2[1])}
    if normals_a is not None:
        detail["normals_b"] = unsort(nb_d.cpu().numpy(), tb.order)
    return out, detail


def pc_error(points_a, points_b, normals_a=None, resolution=1023, colors_a=None, colors_b=None, off_grid="host"):
    """All figures of myutils/pc_error_wrapper.pc_error (26-75) as one dict: D1 always, D2 when normals are given.
    points_b with fractional coordinates (a rate point with scale != 1): pc_error_off_grid (off_grid="host", a k-d tree in
    scipy, at most 8 ties per point) or pc_error_float (off_grid="device", the HIP kernels, every tie).
    colors_a and colors_b (uint8 [N,3], both): the colour keys of `--color=1` as well (color_metrics; voxelised clouds only)."""
    if off_grid not in ("host", "device"):
        raise ValueError("pc_error: off_grid must be 'host' or 'device' (got %r)" % (off_grid,))
    if (colors_a is None) != (colors_b is None):
        raise ValueError("pc_error: colours of both clouds are needed for the colour figures")
    if _off_grid(points_b):
        if colors_a is not None:
            raise ValueError("pc_error: the colour figures need a cloud on the integer grid")
        if off_grid == "device":
            return pc_error_float(points_a, points_b, normals_a, resolution)
        return pc_error_off_grid(points_a, points_b, normals_a, resolution)
    out = d1_metrics(points_a, points_b, resolution)
    if normals_a is not None:
        out.update(d2_metrics(points_a, normals_a, points_b, resolution))
    if colors_a is not None:
        out.update(color_metrics(points_a, colors_a, points_b, colors_b))
    return out


# ---------------------------------------------------------------------------- a mesh against its cloud
MESH_MAX_COORD = 2.0 ** 20        # every coordinate of the cloud and the mesh lies strictly inside (include/pcgc.h, pcgc_meshdist_*)
MESH_PAIRS_PER_TRIANGLE = 32      # the cell edge doubles while the triangles are listed in more cells than this, on average


def mesh_cells(lo, hi, h):
    """-> (h, ox, oy, oz, res): the cells of edge h that cover the box lo .. hi (float64 [3])"""
    lo, hi = np.asarray(lo, np.float64).reshape(3), np.asarray(hi, np.float64).reshape(3)
    origin = np.floor(lo / h)
    return (float(h), int(origin[0]), int(origin[1]), int(origin[2]), int((np.floor(hi / h) - origin).max()) + 1)


def mesh_first_edge(lo, hi):
    """the smallest power of two h >= 1 whose cells cover the box with at most OFFGRID_MAX_CELLS per axis"""
    h = 1.0
    while mesh_cells(lo, hi, h)[4] > OFFGRID_MAX_CELLS:
        h *= 2.0
    return h


def choose_mesh_cells(lo, hi, n_triangles, count_pairs, edge=None):
    """-> (cells, pairs).  The cells the triangles of a mesh with the bounding box lo .. hi are listed in: the edge starts at
    mesh_first_edge and doubles while count_pairs(cells), the number of (cell, triangle) pairs, exceeds 32 per triangle.  It
    ends: once the edge reaches the widest bounding box, a triangle overlaps at most 8 cells.  edge: that edge and no other."""
    first = mesh_first_edge(lo, hi)
    if edge is not None:
        h = float(edge)
        if not (h >= first and h <= OFFGRID_MAX_EDGE and np.frexp(h)[0] == 0.5):
            raise ValueError("mesh_error: the cell edge %r must be a power of two within %g .. 2^20" % (edge, first))
        cells = mesh_cells(lo, hi, h)
        return cells, int(count_pairs(cells))
    h = first
    while True:
        cells = mesh_cells(lo, hi, h)
        pairs = int(count_pairs(cells))
        if pairs <= MESH_PAIRS_PER_TRIANGLE * n_triangles or h >= OFFGRID_MAX_EDGE:
            return cells, pairs
        h *= 2.0


def check_max_dist(max_dist):
    if max_dist is None:
        return float("inf")
    if isinstance(max_dist, bool) or not (np.isfinite(max_dist) and max_dist > 0):
        raise ValueError("mesh_error: max_dist = %r must be finite and positive (None: no gate)" % (max_dist,))
    return float(max_dist)


def _mesh_error_input(points, vertices, triangles):
    """float64 [N,3], float64 [V,3], int32 [T,3] on the device and the bounding box of the triangles' corners; a ValueError
    names the first bad row (one read-back)"""
    dev = _lib.require_gpu()

    def tensor(x, dtype, np_dtype):
        x = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(np.asarray(x).reshape(-1, 3).astype(np_dtype)))
        x = x.to(dev).reshape(-1, 3)
        return (x if dtype is None else x.to(dtype)).contiguous()
    p, v = tensor(points, torch.float64, np.float64), tensor(vertices, torch.float64, np.float64)
    t = tensor(triangles, None, np.int64)                                 # in its own integer type until the indices are checked
    if t.dtype not in (torch.int32, torch.int64):
        t = t.to(torch.int64)
    N, V, T = int(p.shape[0]), int(v.shape[0]), int(t.shape[0])
    if N == 0:
        raise ValueError("mesh_error: the cloud has no points")
    if T == 0 or V == 0:
        raise ValueError("mesh_error: the mesh has no triangles")
    if N >= 2 ** 31 or V >= 2 ** 31 or 3 * T >= 2 ** 31:
        raise ValueError("mesh_error: %d points, %d vertices and %d triangles are too many (N, V and 3 T below 2^31)" % (N, V, T))
    bad_p = ~(p.abs() < MESH_MAX_COORD).all(1)                            # a NaN is not below
    bad_v = ~(v.abs() < MESH_MAX_COORD).all(1)
    bad_t = ((t < 0) | (t >= V)).any(1)
    inside = t.clamp(0, V - 1)                                            # what this clamps is refused below
    used = torch.zeros(V, dtype=torch.bool, device=dev).index_fill_(0, inside.reshape(-1).long(), True)[:, None]
    lo, hi = torch.where(used, v, float("inf")).min(0)[0], torch.where(used, v, float("-inf")).max(0)[0]       # of the corners alone
    got = torch.cat([torch.stack([bad_p.any(), bad_v.any(), bad_t.any()]).double(), lo, hi]).tolist()
    if got[0]:
        row = int(bad_p.nonzero()[0])
        raise ValueError("mesh_error: point row %d, %s, is not finite or reaches 2^20" % (row, p[row].tolist()))
    if got[1]:
        row = int(bad_v.nonzero()[0])
        raise ValueError("mesh_error: vertex row %d, %s, is not finite or reaches 2^20" % (row, v[row].tolist()))
    if got[2]:
        row = int(bad_t.nonzero()[0])
        raise ValueError("mesh_error: triangle row %d, %s, names a vertex outside 0..%d" % (row, t[row].tolist(), V - 1))
    return p, v, inside.to(torch.int32).contiguous(), np.array(got[3:6]), np.array(got[6:9])


class _MeshSearch(object):
    """the triangles of a mesh in their cells, one method per part (tools/surface_bench.py times them one by one)"""

    def __init__(self, v, t, lo, hi):
        self.lib, self.v, self.t, self.lo, self.hi, self.dev = _lib.hip(), v, t, lo, hi, v.device
        self.V, self.T = int(v.shape[0]), int(t.shape[0])
        self.flag = torch.zeros(1, dtype=torch.int32, device=self.dev)

    def count(self, cells):
        self.counts = torch.empty(self.T, dtype=torch.int64, device=self.dev)
        _lib.check(self.lib.pcgc_meshdist_count(_lib.dptr(self.v), self.V, _lib.dptr(self.t), self.T, *cells, _lib.dptr(self.counts),
                                                _lib.dptr(self.flag), _lib.stream()), "pcgc_meshdist_count")
        return int(self.counts.sum().item())                             # the one read-back per edge tried

    def choose(self, edge=None):
        self.cells, self.pairs = choose_mesh_cells(self.lo, self.hi, self.T, self.count, edge)
        if not 1 <= self.pairs < 2 ** 31 - 1:
            raise ValueError("mesh_error: %d pairs of cell and triangle (1 .. 2^31 - 2 are searched)" % self.pairs)
        return self.cells, self.pairs

    def emit(self):
        """the pairs of the chosen cells (self.counts are theirs: the last edge counted), sorted"""
        offsets = (torch.cumsum(self.counts, 0) - self.counts).contiguous()
        words = torch.full((self.pairs,), -1, dtype=torch.int64, device=self.dev)
        _lib.check(self.lib.pcgc_meshdist_emit(_lib.dptr(self.v), self.V, _lib.dptr(self.t), self.T, *self.cells, _lib.dptr(offsets),
                                               self.pairs, _lib.dptr(words), _lib.dptr(self.flag), _lib.stream()), "pcgc_meshdist_emit")
        self.words = torch.sort(words)[0]

    def prepare(self, n_points):
        self.n_points = int(n_points)
        self.ws = torch.empty(int(self.lib.pcgc_meshdist_workspace_bytes(self.cells[4], self.pairs, self.n_points)), dtype=torch.uint8,
                              device=self.dev)
        self.packed = torch.empty((self.T, 9), dtype=torch.float64, device=self.dev)
        _lib.check(self.lib.pcgc_meshdist_prepare(_lib.dptr(self.v), self.V, _lib.dptr(self.t), self.T, _lib.dptr(self.words), self.pairs,
                                                  self.cells[4], self.n_points, _lib.dptr(self.packed), _lib.dptr(self.flag),
                                                  _lib.dptr(self.ws), self.ws.numel(), _lib.stream()), "pcgc_meshdist_prepare")

    def order(self, p):
        """the points by the key of their cell (the nearest cell for a point outside), so that a wave's lanes walk the same cells"""
        return torch.sort(cell_keys(p, self.cells, clamp=True), stable=True)[1].to(torch.int32).contiguous()

    def query(self, p, order, max_dist):
        """-> (out4 float64 [4], best float64 [N], nearest int32 [N]), device tensors"""
        n = int(p.shape[0])
        out = torch.empty(4, dtype=torch.float64, device=self.dev)
        best = torch.empty(n, dtype=torch.float64, device=self.dev)
        nearest = torch.empty(n, dtype=torch.int32, device=self.dev)
        _lib.check(self.lib.pcgc_meshdist_query(_lib.dptr(p), n, _lib.dptr(order), _lib.dptr(self.packed), self.T, self.pairs, *self.cells,
                                                max_dist, _lib.dptr(out), _lib.dptr(best), _lib.dptr(nearest), _lib.dptr(self.flag),
                                                _lib.dptr(self.ws), self.ws.numel(), _lib.stream()), "pcgc_meshdist_query")
        return out, best, nearest


def _mesh_error_device(p, v, t, lo, hi, max_dist=float("inf"), edge=None, sort_points=True):
    """the search on validated device tensors -> (figures dict, best, nearest, candidates evaluated)"""
    s = _MeshSearch(v, t, lo, hi)
    cells, pairs = s.choose(edge)
    s.emit()
    s.prepare(p.shape[0])
    out, best, nearest = s.query(p, s.order(p) if sort_points else None, max_dist)
    mse, top, far, evaluated = out.tolist()
    if np.isnan(far):
        raise RuntimeError("pcgc_meshdist_*: the mesh or the cloud breaks the rule's contract (include/pcgc.h)")
    n = int(p.shape[0])
    figures = {"points": n, "far": int(far), "mse (p2mesh)": mse, "rms (p2mesh)": float(np.sqrt(mse)), "h. (p2mesh)": top,
               "edge": int(cells[0]), "pairs": pairs}
    return figures, best, nearest, int(evaluated)


def mesh_error(points, vertices, triangles, max_dist=None, samples=0, seed=0, per_point=False, _edge=None, _sort_points=True):
    """How far a cloud lies from a triangle mesh (csrc/meshdist.hip; include/pcgc.h, pcgc_meshdist_*; tests/_mesh_error_ref.py is
    the rule in numpy): for every point the exact squared distance to the nearest triangle, faces, edges and corners alike, in
    float64.  points [N,3] integer voxels or floats, vertices float64 [V,3], triangles int [T,3], numpy arrays or device
    tensors, all in the same units (voxel units: surface.reconstruct's before a frame is applied), |coordinate| < 2^20.
    max_dist: a point farther than it from the mesh is far and counts in no mean (None: no gate); it also bounds the walk of a
    point that lies many cells from every triangle, which without a gate looks at every cell on its way.  -> a dict:
      points, far                          how many points, and how many of them far
      mse (p2mesh), rms (p2mesh)           the mean of the squared distance over the points that are not far, and its root
      h. (p2mesh)                          the largest SQUARED distance among them (as pc_error's h. keys); NaN, like the means,
                                           where every point is far
      edge, pairs                          the edge of the search's cells and the (cell, triangle) pairs listed in them
    The figures depend on the cloud and the triangle list alone, not on the cells.  per_point=True: -> (dict, (best float64
    [N] = the squared distances, +inf for a far point; nearest int32 [N] = the smallest index of a triangle at that distance,
    -1 for a far point)), in the caller's order.
    samples > 0 adds the opposite direction: `samples` area-weighted points of the mesh (mesh2pc_open3d.sample_points_uniformly
    with `seed`), rounded to float32, against the cloud by one direction of pc_error_float's search: mse (mesh2p), h. (mesh2p)
    and h. (sym) = the larger of the two h.  That direction finds sheets the mesh invented where there are no points; a mesh
    lying exactly on the surface still measures about half the point spacing there, since the samples fall between the points.
    _edge, _sort_points: the tests' (a forced cell edge; the points taken as they come)."""
    gate = check_max_dist(max_dist)
    if isinstance(samples, bool) or int(samples) != samples or samples < 0:
        raise ValueError("mesh_error: samples = %r must be a count" % (samples,))
    p, v, t, lo, hi = _mesh_error_input(points, vertices, triangles)
    figures, best, nearest, _ = _mesh_error_device(p, v, t, lo, hi, gate, _edge, _sort_points)
    if samples:
        figures.update(_mesh_to_cloud(p, v, t, int(samples), seed))
        figures["h. (sym)"] = max(figures["h. (p2mesh)"], figures["h. (mesh2p)"])
    if per_point:
        return figures, (best.cpu().numpy(), nearest.cpu().numpy())
    return figures


def _mesh_to_cloud(p, v, t, samples, seed):
    """samples of the mesh against the cloud: pieces that exist (the sampler, the off-grid target and its search)"""
    from .dataprocess.mesh2pc_open3d import sample_points_uniformly
    s = sample_points_uniformly(v.cpu().numpy(), t.cpu().numpy(), samples, seed, device=True).to(torch.float32).contiguous()
    cloud = p.to(torch.float32).cpu().numpy()
    target = _OffgridTarget(cloud, s.cpu().numpy(), p.device)
    ws = torch.empty(int(_lib.hip().pcgc_offgrid_workspace_bytes(target.res, len(cloud))), dtype=torch.uint8, device=p.device)
    mse, top, _, _ = _offgrid_mse(s, target, None, ws)
    return {"mse (mesh2p)": mse, "h. (mesh2p)": top}


def bpp(total_bytes, n_input_points):
    """eval.py:102-111: 8 * bytes of all files / points of the ORIGINAL cloud."""
    return 8.0 * float(total_bytes) / float(n_input_points)
