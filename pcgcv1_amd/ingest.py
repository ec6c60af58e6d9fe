"""Raw scans onto the codec's grid: float coordinates in the scanner's units, several points per voxel, colours and normals
-> one integer point per occupied voxel with merged attributes, and the frame that maps it back.

    python -m pcgcv1_amd.ingest --input scan.ply --output scan_vox10.ply --bits 10      # or --voxel_size 0.002
                                [--smooth 3:2]              # thin the noisy shell first: pcgcv1_amd/smooth.py
                                [--clean stat:20:2.0]       # drop outlier voxels and refit the frame: voxelize_scan_clean

writes the voxelised ply and scan_vox10.frame next to it.  The rule (include/pcgc.h, pcgc_ingest_*; DESIGN.md §7f;
tests/_ingest_ref.py restates it in numpy), all position arithmetic in float64:

  frame  = (origin[3], step, bits), 1 <= bits <= 12, R = 2^bits - 1
  bits given:        origin = per-axis minimum, step = (largest axis extent) / R, or 1 when the extent is 0
  voxel_size given:  step = voxel_size, origin = floor(min / step) * step, bits = the fewest that hold every coordinate
  q      = clamp(floor((p - origin) / step + 0.5), 0, R);     p' = origin + q * step  (apply_frame)
  merge  = per occupied voxel, in np.unique's order: the count, the exact colour mean (half up) and the normalised sum of
           the normals (2^30 fixed point, so the sum is an integer and order-free)

Rows with a non-finite coordinate are dropped and counted.  Bounds, quantisation and merge run in csrc/ingest.hip.
"""
import argparse
import struct

import numpy as np

from . import _lib

MAX_BITS = 12
FRAME_MAGIC, FRAME_VERSION, FRAME_BYTES = b"PCFR", 1, 40


class Frame(object):
    """origin float64 [3], step > 0, bits 1..12: grid coordinate q <-> origin + q * step"""

    def __init__(self, origin, step, bits):
        self.origin = np.array(origin, np.float64).reshape(3)
        self.step = float(step)
        self.bits = int(bits)
        if not 1 <= self.bits <= MAX_BITS:
            raise ValueError("frame: bits = %d outside 1..%d" % (self.bits, MAX_BITS))
        if not (np.isfinite(self.origin).all() and np.isfinite(self.step) and self.step > 0):
            raise ValueError("frame: origin %s and step %r must be finite, the step positive" % (self.origin.tolist(), self.step))

    @property
    def R(self):
        return 2 ** self.bits - 1

    def __eq__(self, other):
        return (isinstance(other, Frame) and self.bits == other.bits and self.step == other.step
                and self.origin.tobytes() == other.origin.tobytes())

    def __repr__(self):
        return "Frame(origin=%s, step=%r, bits=%d)" % (self.origin.tolist(), self.step, self.bits)


def _frame_from_bounds(lo, hi, bits, voxel_size):
    """the two fitting modes on the bounds of the finite rows.  + 0.0: a -0.0 minimum becomes +0.0 (min does not order them)"""
    if (bits is None) == (voxel_size is None):
        raise ValueError("fit_frame: give bits or voxel_size, one of them")
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    if bits is not None:
        if not 1 <= int(bits) <= MAX_BITS:
            raise ValueError("fit_frame: bits = %r outside 1..%d" % (bits, MAX_BITS))
        ext = float((hi - lo).max())
        return Frame(lo + 0.0, ext / (2 ** int(bits) - 1) if ext != 0 else 1.0, bits)
    s = float(voxel_size)
    if not (np.isfinite(s) and s > 0):
        raise ValueError("fit_frame: voxel_size must be positive and finite (got %r)" % (voxel_size,))
    with np.errstate(over="ignore"):                            # an absurd voxel size overflows to inf: refused below
        origin = np.floor(lo / s) * s + 0.0
        qmax = float(np.floor((hi - origin) / s + 0.5).max())   # quantisation is monotone: the largest coordinate of all
    if not qmax < 2 ** MAX_BITS:
        raise ValueError("fit_frame: an extent of %r at voxel size %r needs more than %d bits (coordinates up to %.0f); use a larger "
                         "voxel size" % (float((hi - lo).max()), s, MAX_BITS, qmax))
    return Frame(origin, s, max(1, int(qmax).bit_length()))


def _device_points(points):
    """float64 [n,3] on the device, from numpy or a tensor"""
    import torch
    dev = _lib.require_gpu()
    p = points if torch.is_tensor(points) else torch.from_numpy(np.ascontiguousarray(np.asarray(points, np.float64).reshape(-1, 3)))
    return p.to(dev, torch.float64).reshape(-1, 3).contiguous()


def bounds(points):
    """-> (min float64 [3], max float64 [3], n_dropped) over the rows whose coordinates are all finite, on the device
    (pcgc_ingest_bounds).  ValueError when no row remains."""
    import torch
    p_d = _device_points(points)
    n = int(p_d.shape[0])
    if n == 0:
        raise ValueError("ingest: the cloud has no points")
    out = torch.empty(6, dtype=torch.float64, device=p_d.device)
    dropped = torch.empty(1, dtype=torch.int64, device=p_d.device)
    _lib.check(_lib.hip().pcgc_ingest_bounds(_lib.dptr(p_d), n, _lib.dptr(out), _lib.dptr(dropped), _lib.stream()), "pcgc_ingest_bounds")
    out, n_dropped = out.cpu().numpy(), int(dropped.item())
    if n_dropped == n:
        raise ValueError("ingest: none of the %d rows has three finite coordinates" % n)
    return out[:3], out[3:], n_dropped


def fit_frame(points, bits=None, voxel_size=None):
    """The frame of a cloud (float [N,3]) for a grid of 2^bits cells per axis, or for voxels of edge voxel_size.  Min and
    max do not depend on the order they are taken in: a numpy array is reduced where it lies, on the host; a device tensor
    on the device (what voxelize_scan does with the cloud it has uploaded).  ValueError: no finite row, or a voxel_size
    that needs more than 12 bits."""
    import torch
    if torch.is_tensor(points) and points.is_cuda:
        lo, hi, _ = bounds(points)
    else:
        p = np.asarray(points, np.float64).reshape(-1, 3)
        p = p[np.isfinite(p).all(1)]
        if not len(p):
            raise ValueError("ingest: no row has three finite coordinates")
        lo, hi = p.min(0), p.max(0)
    return _frame_from_bounds(lo, hi, bits, voxel_size)


def quantize(points, frame):
    """-> (q int32 [n,3], keys int64 [n]) device tensors (pcgc_ingest_quantize); a dropped row has q = -1 and key -1"""
    import torch
    p_d = _device_points(points)
    n = int(p_d.shape[0])
    q = torch.empty((n, 3), dtype=torch.int32, device=p_d.device)
    keys = torch.empty(n, dtype=torch.int64, device=p_d.device)
    _lib.check(_lib.hip().pcgc_ingest_quantize(_lib.dptr(p_d), n, _lib.nptr(frame.origin), frame.step, frame.bits, _lib.dptr(q),
                                               _lib.dptr(keys), _lib.stream()), "pcgc_ingest_quantize")
    return q, keys


def merge(keys, bits, colors=None, normals=None):
    """keys: device int64 [n]; colors uint8 [n,3] / normals float32 [n,3]: numpy, tensors or None -> host arrays
    (points int32 [m,3], counts int32 [m], colors | None, normals | None), rows in ascending key (pcgc_ingest_merge)"""
    import torch
    pts, counts, oc, on, n_out = merge_device(keys, bits, colors, normals)
    m = int(n_out.item())

    def down(t):
        # through page-locked memory: a copy into fresh pageable memory is staged in small pieces (the 55 MB of 2.9 M rows
        # took 20 to 40 ms that way, several times everything else: profiles/ingest_bench.txt)
        if t is None:
            return None
        host = torch.empty((m,) + tuple(t.shape[1:]), dtype=t.dtype, pin_memory=m > 0)
        host.copy_(t[:m], non_blocking=True)
        return host

    out = [down(t) for t in (pts, counts, oc, on)]
    torch.cuda.current_stream().synchronize()
    return tuple(None if h is None else h.numpy() for h in out)


def merge_device(keys, bits, colors=None, normals=None):
    """merge without the read-back: device tensors sized for min(n, res^3) rows, of which the first n_out (device int64 [1])
    are written"""
    import torch
    dev = keys.device
    n = int(keys.shape[0])
    lib = _lib.hip()

    def up(a, dtype, name):
        if a is None:
            return None
        t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
        if tuple(t.shape) != (n, 3):
            raise ValueError("ingest: %d points, %s of shape %s" % (n, name, tuple(t.shape)))
        if dtype == torch.uint8 and t.dtype != torch.uint8:
            raise ValueError("ingest: colours must be uint8 (got %s)" % t.dtype)
        return t.to(dev, dtype).contiguous()

    c_d, n_d = up(colors, torch.uint8, "colours"), up(normals, torch.float32, "normals")
    cap = min(n, 8 ** bits)
    ws = torch.empty(int(lib.pcgc_ingest_workspace_bytes(bits, n)), dtype=torch.uint8, device=dev)
    pts = torch.empty((cap, 3), dtype=torch.int32, device=dev)
    counts = torch.empty(cap, dtype=torch.int32, device=dev)
    oc = torch.empty((cap, 3), dtype=torch.uint8, device=dev) if c_d is not None else None
    on = torch.empty((cap, 3), dtype=torch.float32, device=dev) if n_d is not None else None
    n_out = torch.zeros(1, dtype=torch.int64, device=dev)
    _lib.check(lib.pcgc_ingest_merge(_lib.dptr(keys), n, bits, _lib.dptr(c_d), _lib.dptr(n_d), _lib.dptr(pts), _lib.dptr(counts),
                                     _lib.dptr(oc), _lib.dptr(on), cap, _lib.dptr(n_out), _lib.dptr(ws), ws.numel(), _lib.stream()),
               "pcgc_ingest_merge")
    return pts, counts, oc, on, n_out


def smooth_points(points, frame=None, bits=None, voxel_size=None, smooth=None):
    """The smoothing stage in front of the voxelisation (a --smooth spec, pcgcv1_amd/smooth.py) -> (points float64 [N,3] in
    the scan's units, a device tensor; smooth.smooth_scan's report).  The radius is in voxels of `frame`, or of the frame fitted
    to the raw scan for `bits` or `voxel_size`."""
    from . import smooth as smoother
    spec = smoother.parse_spec(smooth)
    p_d = _device_points(points)
    if frame is None:
        lo, hi, _ = bounds(p_d)
        frame = _frame_from_bounds(lo, hi, bits, voxel_size)
    return smoother.smooth_scan_device(p_d, frame, spec)


def voxel_count(points, frame):
    """occupied voxels of a float cloud on `frame` (quantise and merge, nothing read back but the count)"""
    _, keys = quantize(points, frame)
    return int(merge_device(keys, frame.bits)[4].item())


def smooth_line(raw, smoothed, report, bits=None, voxel_size=None, frame=None):
    """the 'smooth: ...' line of the command lines: the occupied voxels of the raw and of the smoothed cloud, both on the frame
    the voxelisation fits to the smoothed one (or on `frame`)"""
    from . import smooth as smoother
    if frame is None:
        frame = fit_frame(smoothed, bits, voxel_size)
    return smoother.summary_line(report, voxel_count(raw, frame), voxel_count(smoothed, frame))


def voxelize_scan(points, colors=None, normals=None, frame=None, bits=None, voxel_size=None, clean=None, smooth=None):
    """A scan (float [N,3]; colors uint8 [N,3], normals float [N,3] or None) on the grid of `frame`, or of the frame fitted to it
    for `bits` or `voxel_size` -> (points int32 [M,3] in np.unique's order, colors uint8 [M,3] | None, normals float32
    [M,3] | None, counts int32 [M], frame, n_dropped).  Points outside a given frame are clamped to its grid.
    clean (a --clean spec or a list of them, pcgcv1_amd/clean.py): voxelize_scan_clean's eight values instead.
    smooth (a --smooth spec, pcgcv1_amd/smooth.py): the positions go through smooth_points first, and everything else is
    this function as it stands on what comes back, the fit of its own frame included."""
    if clean:
        if frame is not None:
            raise ValueError("voxelize_scan: clean refits the frame to what it keeps: give bits or voxel_size, not a frame")
        return voxelize_scan_clean(points, colors, normals, bits, voxel_size, clean, smooth)
    if frame is not None and (bits is not None or voxel_size is not None):
        raise ValueError("voxelize_scan: give a frame, or bits / voxel_size to fit one")
    if smooth:
        points = smooth_points(points, frame, bits, voxel_size, smooth)[0]
    p_d = _device_points(points)
    lo, hi, n_dropped = bounds(p_d)
    if frame is None:
        frame = _frame_from_bounds(lo, hi, bits, voxel_size)
    _, keys = quantize(p_d, frame)
    pts, counts, c, nrm = merge(keys, frame.bits, colors, normals)
    return pts, c, nrm, counts, frame, n_dropped


def voxelize_scan_clean(points, colors=None, normals=None, bits=None, voxel_size=None, clean=(), smooth=None):
    """voxelize_scan with the outlier voxels of pcgcv1_amd/clean.py dropped and the frame fitted again to what is left ->
    (points, colors, normals, counts, frame, n_dropped, n_removed_voxels, n_removed_points):
      1. fit the frame, quantise, merge, and run the filters `clean` (a spec or a list, applied in order) on the voxels;
      2. drop the input rows whose voxel was removed, as well as the non-finite ones;
      3. bounds over the kept rows, the frame fitted again with the same bits / voxel_size;
      4. quantise and merge again.
    There is no second cleaning pass: the result is not filtered on its own, finer, grid.  With bits the resolution the
    outliers took comes back; with voxel_size the origin stays a multiple of the step, so the result is the kept voxels of
    pass 1 shifted by whole cells, in possibly fewer bits.  ValueError when the filters would leave nothing.
    smooth: as voxelize_scan, in front of step 1."""
    if smooth:
        points = smooth_points(points, None, bits, voxel_size, smooth)[0]
    return _voxelize_scan_clean(points, colors, normals, bits, voxel_size, clean)[0]


def _voxelize_scan_clean(points, colors, normals, bits, voxel_size, clean, report=None):
    """-> (voxelize_scan_clean's values, the voxels of pass 1 as a device tensor: what the command lines report on); report:
    as clean.keep_mask"""
    import torch
    from . import clean as cleaner
    specs = cleaner.parse_specs(clean)
    p_d = _device_points(points)
    lo, hi, n_dropped = bounds(p_d)
    frame = _frame_from_bounds(lo, hi, bits, voxel_size)
    _, keys = quantize(p_d, frame)
    vox, _, _, _, n_out = merge_device(keys, frame.bits)
    vox = vox[:int(n_out.item())]
    keep = torch.from_numpy(cleaner.keep_mask_all(vox, frame.bits, specs, report)).to(p_d.device)
    # a row's voxel: the voxels are in ascending key, a dropped row (key -1) finds some voxel and is refused by its key
    res = 1 << frame.bits
    vox_keys = (vox[:, 0].long() * res + vox[:, 1].long()) * res + vox[:, 2].long()
    row_keep = keep[torch.searchsorted(vox_keys, keys).clamp_(max=len(vox_keys) - 1)] & (keys >= 0)
    n_removed_points = int(p_d.shape[0]) - n_dropped - int(row_keep.sum().item())

    def rows(a, dtype):
        if a is None:
            return None
        t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
        if tuple(t.shape) != (int(p_d.shape[0]), 3):
            raise ValueError("ingest: %d points, attribute of shape %s" % (int(p_d.shape[0]), tuple(t.shape)))
        if dtype == torch.uint8 and t.dtype != torch.uint8:
            raise ValueError("ingest: colours must be uint8 (got %s)" % t.dtype)
        return t.to(p_d.device, dtype)[row_keep]

    kept = p_d[row_keep]
    lo, hi, _ = bounds(kept)
    frame = _frame_from_bounds(lo, hi, bits, voxel_size)
    _, keys = quantize(kept, frame)
    pts, counts, c, nrm = merge(keys, frame.bits, rows(colors, torch.uint8), rows(normals, torch.float32))
    return (pts, c, nrm, counts, frame, n_dropped, int((~keep).sum().item()), n_removed_points), vox


def apply_frame(points, frame):
    """grid coordinates [N,3] -> float64 [N,3] in the scan's own units: origin + q * step, as mul then add"""
    q = np.asarray(points).astype(np.float64).reshape(-1, 3)
    return frame.origin + q * np.float64(frame.step)


# ---------------------------------------------------------------------------- <name>.frame
def frame_bytes(frame):
    """40 bytes: 'PCFR', u8 version = 1, u8 bits, two zero bytes, origin 3 x float64 LE, step float64 LE"""
    return struct.pack("<4sBBH3dd", FRAME_MAGIC, FRAME_VERSION, frame.bits, 0, *frame.origin.tolist(), frame.step)


def write_frame(filename, frame):
    with open(filename, "wb") as f:
        f.write(frame_bytes(frame))


def read_frame(filename):
    with open(filename, "rb") as f:
        data = f.read()
    if len(data) != FRAME_BYTES:
        raise ValueError("%s: a frame file holds %d bytes, this one %d" % (filename, FRAME_BYTES, len(data)))
    magic, version, bits, pad, ox, oy, oz, step = struct.unpack("<4sBBH3dd", data)
    if magic != FRAME_MAGIC:
        raise ValueError("%s: magic %r is not %r" % (filename, magic, FRAME_MAGIC))
    if version != FRAME_VERSION:
        raise ValueError("%s: frame version %d, this reader knows version %d" % (filename, version, FRAME_VERSION))
    if not 1 <= bits <= MAX_BITS:
        raise ValueError("%s: bits = %d outside 1..%d" % (filename, bits, MAX_BITS))
    try:
        return Frame((ox, oy, oz), step, bits)
    except ValueError as e:
        raise ValueError("%s: %s" % (filename, e))


def frame_path(ply_or_stem):
    """scan_vox10.ply -> scan_vox10.frame"""
    return (ply_or_stem[:-4] if ply_or_stem.lower().endswith(".ply") else ply_or_stem) + ".frame"


# ---------------------------------------------------------------------------- command line
def voxelize_scan_report(points, colors=None, normals=None, bits=None, voxel_size=None, clean=None, smooth=None):
    """what the command lines run -> (voxelize_scan's six values, the 'clean: ...' summary line, or None without clean; a
    component filter adds a line of its own: clean.components_line).  smooth: the 'smooth: ...' line comes first."""
    if smooth:
        smoothed, moved = smooth_points(points, None, bits, voxel_size, smooth)
        out, line = voxelize_scan_report(smoothed, colors, normals, bits, voxel_size, clean)
        return out, "\n".join([smooth_line(points, smoothed, moved, bits, voxel_size)] + ([line] if line else []))
    if not clean:
        return voxelize_scan(points, colors, normals, bits=bits, voxel_size=voxel_size), None
    from . import clean as cleaner
    import torch
    report = []
    out, vox = _voxelize_scan_clean(points, colors, normals, bits, voxel_size, clean, report)
    cube = vox >> 6                                             # 64^3 cubes of pass 1: at most 6 bits per axis are left
    cubes = len(torch.unique((cube[:, 0] << 12) | (cube[:, 1] << 6) | cube[:, 2]))
    return out[:6], "\n".join([cleaner.summary_line(clean, len(vox), out[6], cubes, cleaner.n_cubes(out[0]), out[7])] + report)


def ingest_file(filename, bits=None, voxel_size=None, clean=None, smooth=None):
    """load_ply_scan + voxelize_scan -> (points, colors | None, normals | None, counts, frame, n_dropped, n_input), and with
    clean the 'clean: ...' summary line (and a component filter's line below it) as an eighth value; with smooth the
    'smooth: ...' line, in front of clean's"""
    from .dataprocess.inout_points import load_ply_scan
    points, colors, normals = load_ply_scan(filename)
    if not len(points):
        raise ValueError("%s holds no points" % filename)
    out, line = voxelize_scan_report(points, colors, normals, bits, voxel_size, clean, smooth)
    return out + (len(points),) + ((line,) if clean or smooth else ())


def summary_line(n_input, n_dropped, counts, frame):
    return "ingest: {} input points, {} dropped (non-finite), {} occupied voxels, at most {} points in one voxel, step {!r} ({} bits)".format(
        n_input, n_dropped, len(counts), int(counts.max()), frame.step, frame.bits)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="voxelise a raw scan (float coordinates, colours, normals) for the codec")
    ap.add_argument("--input", required=True, help="the scan: ASCII or binary ply")
    ap.add_argument("--output", required=True, help="the voxelised ply; <output without .ply>.frame is written next to it")
    ap.add_argument("--bits", type=int, default=None, help="fit the scan into a grid of 2^bits cells per axis (1..12)")
    ap.add_argument("--voxel_size", type=float, default=None, help="voxel edge in the scan's units; the grid grows to hold the scan")
    ap.add_argument("--attributes", choices=("colors", "normals"), default="colors",
                    help="which attribute the ply carries when the scan has both (it has room for one)")
    from .clean import add_clean_argument, check_clean_argument
    add_clean_argument(ap)
    from .smooth import add_smooth_argument, check_smooth_argument
    add_smooth_argument(ap)
    args = ap.parse_args(argv)
    check_clean_argument(ap, args)
    check_smooth_argument(ap, args)
    if (args.bits is None) == (args.voxel_size is None):
        ap.error("give --bits or --voxel_size, one of them")
    if args.bits is not None and not 1 <= args.bits <= MAX_BITS:
        ap.error("--bits=%d outside 1..%d" % (args.bits, MAX_BITS))
    if args.voxel_size is not None and not (np.isfinite(args.voxel_size) and args.voxel_size > 0):
        ap.error("--voxel_size must be positive (got %r)" % args.voxel_size)
    return args


def main(argv=None):
    from .dataprocess.inout_points import write_ply_colors, write_ply_data, write_ply_normals
    args = parse_args(argv)
    try:
        out = ingest_file(args.input, args.bits, args.voxel_size, args.clean, args.smooth)
        points, colors, normals, counts, frame, n_dropped, n_input = out[:7]
    except ValueError as e:
        raise SystemExit("ingest: %s" % e)
    if colors is not None and (normals is None or args.attributes == "colors"):
        write_ply_colors(args.output, points, colors)
    elif normals is not None:
        write_ply_normals(args.output, points, normals)
    else:
        write_ply_data(args.output, points)
    write_frame(frame_path(args.output), frame)
    print(summary_line(n_input, n_dropped, counts, frame))
    if args.clean or args.smooth:
        print(out[7])
    print("wrote {} and {}".format(args.output, frame_path(args.output)))


if __name__ == "__main__":
    main()
