"""The cells a float32 cloud is searched in on the device (csrc/offgrid_cells.h), as the Python side sizes and sorts by them:
cells = (h, ox, oy, oz, res), cubic cells of edge h (a power of two), the cell of a coordinate v being floor(v / h) - origin
inside a grid of res^3 cells, and the key of a cell (x * res + y) * res + z.  The kernels want their cloud sorted by that key."""
import numpy as np

MAX_CELLS, MAX_EDGE = 1024, 2.0 ** 20


def cells_from_bounds(lo, hi, radius, who="global_align"):
    """-> (h, ox, oy, oz, res): the cells a search within `radius` walks between the extremes lo and hi (float64 [3]) of a cloud:
    the smallest power of two h >= max(1, radius) with at most 1024 cells per axis"""
    lo, hi = np.asarray(lo, np.float64).reshape(3), np.asarray(hi, np.float64).reshape(3)
    h = 1.0
    while h < radius or int((np.floor(hi / h) - np.floor(lo / h)).max()) + 1 > MAX_CELLS:
        h *= 2.0
        if h > MAX_EDGE:
            raise ValueError("%s: keypoints of extent %g with radius %g need cells wider than 2^20" % (who, float((hi - lo).max()), radius))
    origin = np.floor(lo / h)
    if float(np.abs(np.stack([origin, np.floor(hi / h)])).max()) >= 2.0 ** 28:
        raise ValueError("%s: coordinate / cell edge reaches 2^28 (cell edge %g)" % (who, h))
    return (h, int(origin[0]), int(origin[1]), int(origin[2]), int((np.floor(hi / h) - origin).max()) + 1)


def feature_cells(kp, radius):
    """-> (h, ox, oy, oz, res): the cells pcgc_feature_* search keypoints in: the smallest power of two h >= max(1, radius)
    with at most 1024 cells per axis between the extremes of the finite rows"""
    p = np.asarray(kp, np.float64).reshape(-1, 3)
    p = p[np.isfinite(p).all(1)]
    if not len(p) or not (np.isfinite(radius) and radius > 0):
        raise ValueError("global_align: the keypoints need a finite row and radius must be positive (got %r)" % (radius,))
    return cells_from_bounds(p.min(0), p.max(0), radius)


def cell_keys(points, cells, clamp=False):
    """points: a float [n,3] tensor, on the host or the device -> int64 [n], the key of each row's cell under `cells`.  A row
    outside the cells or with a coordinate that is not finite gets key -1; with clamp=True it gets the key of the nearest cell
    instead, a NaN counting as the coordinate 0."""
    import torch
    h, ox, oy, oz, res = cells
    p = points.to(torch.float64)
    origin = torch.tensor([ox, oy, oz], dtype=torch.float64, device=p.device)

    def key(cell):
        c = cell.to(torch.int64)
        return (c[:, 0] * res + c[:, 1]) * res + c[:, 2]

    if clamp:
        return key((torch.floor(torch.nan_to_num(p, nan=0.0) / h) - origin).clamp_(0, res - 1))
    cell = torch.floor(p / h) - origin
    inside = torch.isfinite(cell).all(1) & (cell >= 0).all(1) & (cell < res).all(1)
    keys = key(torch.where(inside[:, None], cell, torch.zeros_like(cell)))
    return torch.where(inside, keys, torch.full_like(keys, -1))


def cell_order(points, cells):
    """points: a float32 [n,3] tensor, on the host or the device -> the stable order (int64 tensor, where the points lie) that
    sorts them by the key of `cells`, which is how pcgc_feature_*, pcgc_smooth_step and the off-grid search want them; a row
    outside the cells or with a coordinate that is not finite sorts first (key -1), and the kernels refuse it"""
    import torch
    return torch.sort(cell_keys(points, cells), stable=True)[1]
