"""Thin a noisy scan before it is voxelised: every point is projected onto the plane fitted to the points around it.

    --smooth R[:ITERS[:KMIN]]       on python -m pcgcv1_amd.ingest, pcgcv1_amd.register and pcgcv1_amd.test compress --voxelize

A scanner's range noise is a good part of a voxel, and registered scans lie on top of each other off by their residual pose
error: after voxelize_scan that is a shell two or three voxels thick where the codec expects one.  None of the filters of
pcgcv1_amd/clean.py touches it: those points are dense, connected and on the object.

The rule (include/pcgc.h, pcgc_smooth_step; tests/_smooth_ref.py restates it in numpy; csrc/smooth.hip), in grid
units g = float32((p - origin) / step) of the frame fitted to the raw scan (register.to_grid):

  N(i) = the points within R of point i, itself included; a point with fewer than KMIN of them is not moved
  S, Q = the sums of the offsets to them and of their products, exact integers in 2^-16 of a grid unit
  n    = the eigenvector of the smallest eigenvalue of the covariance Q / K - m m^T, m = S / K (float64, cyclic Jacobi)
  g'   = float32(g + (m . n) n)

The weights are uniform inside the ball on purpose: every sum is then an integer, and the device and numpy agree bit for bit.
ITERS passes (default 2, 1..8) are chained, each on the output of the one before, the points sorted by cell again in
between on the device.  KMIN defaults to 6.  Back in scan units p' = origin + double(g') * step (ingest.apply_frame) for
the rows a pass moved; the others, and rows with a coordinate that is not finite, keep their own bits.  Only positions move:
colours and normals stay with their rows.
"""
import numpy as np

from . import _lib
from .cells import cell_order, cells_from_bounds

MAX_RADIUS, MIN_ITERS, MAX_ITERS, MIN_KMIN, MAX_KMIN = 16.0, 1, 8, 3, 1 << 22
DEFAULT_ITERS, DEFAULT_KMIN = 2, 6
BAD_INPUT, TOO_DENSE = 255, 254                      # what pcgc_smooth_step leaves in `moved` when its flag is raised


class Spec(object):
    """radius in voxels, the number of passes, the fewest neighbours that move a point; text = R:ITERS:KMIN"""

    def __init__(self, radius, iters, kmin):
        self.radius, self.iters, self.kmin = float(radius), int(iters), int(kmin)
        self.text = "%g:%d:%d" % (self.radius, self.iters, self.kmin)

    def __repr__(self):
        return "Spec(%s)" % self.text


def _int_field(text, name, value, lo, hi):
    try:
        v = int(value)
    except ValueError:
        raise ValueError("smooth: %s of %r must be a whole number (got %r)" % (name, text, value))
    if not lo <= v <= hi:
        raise ValueError("smooth: %s of %r outside %d..%d" % (name, text, lo, hi))
    return v


def parse_spec(spec):
    """"R[:ITERS[:KMIN]]" (or a Spec) -> Spec.  ValueError names what is wrong."""
    if isinstance(spec, Spec):
        return spec
    text = str(spec)
    fields = text.split(":")
    if not 1 <= len(fields) <= 3 or any(f.strip() == "" for f in fields):
        raise ValueError("smooth: a spec is R[:ITERS[:KMIN]], for example 3:2:6 (got %r)" % (text,))
    try:
        radius = float(fields[0])
    except ValueError:
        raise ValueError("smooth: the radius of %r must be a number of voxels (got %r)" % (text, fields[0]))
    if not (np.isfinite(radius) and 0 < radius <= MAX_RADIUS):
        raise ValueError("smooth: the radius of %r must be positive and at most %g voxels" % (text, MAX_RADIUS))
    iters = _int_field(text, "ITERS", fields[1], MIN_ITERS, MAX_ITERS) if len(fields) > 1 else DEFAULT_ITERS
    kmin = _int_field(text, "KMIN", fields[2], MIN_KMIN, MAX_KMIN) if len(fields) > 2 else DEFAULT_KMIN
    return Spec(radius, iters, kmin)


# ---------------------------------------------------------------------------- the device loop
def smooth_step(points_d, cells, radius, kmin, debug=False):
    """One pass (pcgc_smooth_step) over a device tensor float32 [n,3] that is sorted by the key of `cells` (h, ox, oy, oz,
    res: cells.cells_from_bounds, cells.cell_order) -> (out float32 [n,3], moved uint8 [n]) device tensors, with debug
    also K int32 [n], S int64 [n,3], Q int64 [n,6].  RuntimeError when the step raised its flag."""
    import torch
    n, dev = int(points_d.shape[0]), points_d.device
    lib = _lib.hip()
    ws = torch.empty(max(1, int(lib.pcgc_smooth_workspace_bytes(cells[4], n))), dtype=torch.uint8, device=dev)
    out = torch.empty((n, 3), dtype=torch.float32, device=dev)
    moved = torch.empty(n, dtype=torch.uint8, device=dev)
    K = torch.empty(n, dtype=torch.int32, device=dev) if debug else None
    S = torch.empty((n, 3), dtype=torch.int64, device=dev) if debug else None
    Q = torch.empty((n, 6), dtype=torch.int64, device=dev) if debug else None
    _lib.check(lib.pcgc_smooth_step(_lib.dptr(points_d), n, *cells, float(radius), int(kmin), _lib.dptr(out), _lib.dptr(moved), _lib.dptr(K),
                                    _lib.dptr(S), _lib.dptr(Q), _lib.dptr(ws), ws.numel(), _lib.stream()), "pcgc_smooth_step")
    worst = int(moved.max().item())
    if worst == TOO_DENSE:
        raise RuntimeError("pcgc_smooth_step: a point has more than %d neighbours within %g voxels: the radius is too large for this "
                           "density; use a smaller radius or a coarser grid" % (MAX_KMIN, radius))
    if worst == BAD_INPUT:
        raise RuntimeError("pcgc_smooth_step: a coordinate is not finite or leaves the cells, or the points are not sorted by cell "
                           "(include/pcgc.h)")
    return (out, moved, K, S, Q) if debug else (out, moved)


def smooth_grid_device(g_d, spec):
    """smooth_grid on a device tensor float32 [n,3], n > 0, every coordinate finite -> (g' float32 [n,3], moved bool [n]) device
    tensors, rows in the caller's order"""
    import torch
    from .ingest import bounds
    cur = g_d
    rows = torch.arange(len(cur), device=cur.device)           # cur[k] is the caller's row rows[k]
    moved_any = torch.zeros(len(cur), dtype=torch.bool, device=cur.device)
    for _ in range(spec.iters):
        lo, hi, _ = bounds(cur.to(torch.float64))             # one small kernel; torch's amin / amax over rows take 1.4 ms each at 4 M
        cells = cells_from_bounds(lo, hi, spec.radius, "smooth")
        order = cell_order(cur, cells)
        cur, rows, moved_any = cur[order].contiguous(), rows[order], moved_any[order]
        cur, moved = smooth_step(cur, cells, spec.radius, spec.kmin)
        moved_any |= moved != 0
    out, any_out = torch.empty_like(cur), torch.empty_like(moved_any)
    out[rows], any_out[rows] = cur, moved_any
    return out, any_out


def smooth_grid(g, radius, iters=DEFAULT_ITERS, kmin=DEFAULT_KMIN):
    """g float32 [n,3] in grid units, every coordinate finite -> (g' float32 [n,3], moved bool [n]: some pass moved the row),
    rows in the caller's order.  The passes run on the device, the points sorted by cell again between them there."""
    import torch
    g = np.ascontiguousarray(np.asarray(g), np.float32).reshape(-1, 3)
    spec = parse_spec("%r:%d:%d" % (float(radius), int(iters), int(kmin)))
    if not len(g):
        return g.copy(), np.zeros(0, bool)
    if not np.isfinite(g).all():
        raise ValueError("smooth: smooth_grid takes finite coordinates (smooth_scan passes the other rows through)")
    out, moved = smooth_grid_device(torch.from_numpy(g).to(_lib.require_gpu()), spec)
    return out.cpu().numpy(), moved.cpu().numpy()


def smooth_scan_device(points, frame, spec):
    """smooth_scan with the result left on the device -> (p' float64 [n,3] device tensor, report): what voxelize_scan goes on
    with.  points: numpy or a tensor.  The two conversions are float64 arithmetic, one operation per step, as register.to_grid
    and ingest.apply_frame have it; the divisor and the factor are device tensors, so the division stays a division."""
    import torch
    from .ingest import _device_points
    spec = parse_spec(spec)
    p_d = _device_points(points)
    dev = p_d.device
    finite = torch.isfinite(p_d).all(1)
    report = {"spec": spec.text, "points": int(finite.sum().item()), "moved": 0, "rms_move": 0.0}
    if not report["points"]:
        return p_d.clone(), report
    origin, step = torch.from_numpy(frame.origin.copy()).to(dev), torch.tensor(frame.step, dtype=torch.float64, device=dev)
    g = ((p_d[finite] - origin) / step).to(torch.float32)
    if not bool(torch.isfinite(g).all().item()):
        raise ValueError("smooth: a coordinate does not fit float32 in grid units (step %r)" % frame.step)
    g2, moved = smooth_grid_device(g, spec)
    out = p_d.clone()
    report["moved"] = int(moved.sum().item())
    if report["moved"]:
        landed = g2[moved].to(torch.float64)
        out[torch.nonzero(finite)[:, 0][moved]] = origin + landed * step
        d = landed - g[moved].to(torch.float64)
        report["rms_move"] = float(torch.sqrt(((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).mean()).item())
    return out, report


def smooth_scan(points, frame, spec):
    """points float64 [n,3] in the scan's units, frame: the ingest.Frame whose voxels are the unit of the radius (the one
    fitted to the raw scan) -> (p' float64 [n,3], report).  A row that a pass moved becomes origin + double(g') * step; every
    other row, the rows with a coordinate that is not finite among them, keeps its bits: those are never neighbours, and
    ingest drops and counts them as before.  report: spec (text), points (finite rows), moved, rms_move (voxels, over the
    moved rows)."""
    out, report = smooth_scan_device(np.asarray(points, np.float64).reshape(-1, 3), frame, spec)
    return out.cpu().numpy(), report


def summary_line(report, voxels_before, voxels_after):
    """smooth: 3:2:6 moved 119874 of 120000 points, rms move 0.4312 voxels; voxels 69936 -> 47141"""
    return "smooth: {} moved {} of {} points, rms move {:.4f} voxels; voxels {} -> {}".format(
        report["spec"], report["moved"], report["points"], report["rms_move"], voxels_before, voxels_after)


# ---------------------------------------------------------------------------- command line
def add_smooth_argument(ap):
    ap.add_argument("--smooth", default=None, metavar="SPEC",
                    help="thin the raw scan before it is voxelised (pcgcv1_amd/smooth.py): R[:ITERS[:KMIN]] projects every point onto "
                         "the plane fitted to the points within R voxels of it (at most %g), ITERS times (default %d, 1..%d); a point "
                         "with fewer than KMIN (default %d) such points, itself included, stays where it is.  Runs before the "
                         "voxelisation and before --clean" % (MAX_RADIUS, DEFAULT_ITERS, MAX_ITERS, DEFAULT_KMIN))


def check_smooth_argument(ap, args):
    """parse the spec with the other argument errors; args.smooth becomes a Spec or None"""
    if args.smooth is not None:
        try:
            args.smooth = parse_spec(args.smooth)
        except ValueError as e:
            ap.error(str(e))
