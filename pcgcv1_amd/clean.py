"""Outlier voxels of a scan: flying pixels, reflections and stray returns, dropped before the codec opens a 64^3 cube for each.

    python -m pcgcv1_amd.clean --input vox.ply --output vox_clean.ply --clean stat:20:2.0        # repeatable, applied in order

(a raw scan: python -m pcgcv1_amd.ingest ... --clean SPEC, which also refits the frame).  The rule (include/pcgc.h,
pcgc_clean_neighbors; tests/_clean_ref.py restates it in numpy), all of it integer on the device:

  N(p)  = the squared distances d2(p, q) over the occupied voxels q != p with d2 <= R * R (a Euclidean ball), cnt(p) = |N(p)|
  S(p)  = the sum of isqrt16(d2) = floor(sqrt(d2 * 2^32)) over the min(k, cnt) nearest, every one of the k the ball does not
          hold charged (R + 1) << 16

  radius:R:MIN       keep p when cnt(p) >= MIN                                       1 <= R <= 32, 1 <= MIN <= (2R+1)^3 - 1
  stat:K:RATIO[:R]   keep p when S(p) <= np.mean(S) + RATIO * np.std(S), k = K        1 <= K <= 64, RATIO >= 0, R = 8 when left out

The statistic runs in csrc/clean.hip; mean and std are numpy's float64 reductions over the int64 array read back from the
device, so the mask is exact as well.
"""
import argparse
import math

import numpy as np

from . import _lib

MAX_BITS, MAX_K, MAX_RADIUS, DEFAULT_RADIUS = 12, 64, 32, 8


class Spec(object):
    """one --clean filter: kind 'radius' (radius, min_count) or 'stat' (k, ratio, radius); text = the spec as given"""

    def __init__(self, kind, radius, k=0, ratio=0.0, min_count=0, text=""):
        self.kind, self.radius, self.k, self.ratio, self.min_count, self.text = kind, radius, k, ratio, min_count, text

    def __eq__(self, other):
        return isinstance(other, Spec) and self._key() == other._key()

    def _key(self):
        return self.kind, self.radius, self.k, self.ratio, self.min_count

    def __repr__(self):
        return "Spec(%r)" % self.text


def _int_field(text, name, value, lo, hi):
    try:
        v = int(value)
    except ValueError:
        raise ValueError("--clean %s: %s = %r is not an integer" % (text, name, value))
    if not lo <= v <= hi:
        raise ValueError("--clean %s: %s = %d outside %d..%d" % (text, name, v, lo, hi))
    return v


def parse_spec(text):
    """'radius:R:MIN' or 'stat:K:RATIO[:R]' -> Spec; ValueError names the field that is wrong"""
    if isinstance(text, Spec):
        return text
    fields = str(text).split(":")
    kind = fields[0]
    if kind == "radius":
        if len(fields) != 3:
            raise ValueError("--clean %s: the radius filter is radius:R:MIN (%d fields given)" % (text, len(fields)))
        radius = _int_field(text, "R", fields[1], 1, MAX_RADIUS)
        return Spec("radius", radius, min_count=_int_field(text, "MIN", fields[2], 1, (2 * radius + 1) ** 3 - 1), text=str(text))
    if kind == "stat":
        if len(fields) not in (3, 4):
            raise ValueError("--clean %s: the statistical filter is stat:K:RATIO[:R] (%d fields given)" % (text, len(fields)))
        k = _int_field(text, "K", fields[1], 1, MAX_K)
        try:
            ratio = float(fields[2])
        except ValueError:
            raise ValueError("--clean %s: RATIO = %r is not a number" % (text, fields[2]))
        if not (math.isfinite(ratio) and ratio >= 0):
            raise ValueError("--clean %s: RATIO = %r must be finite and >= 0" % (text, fields[2]))
        radius = _int_field(text, "R", fields[3], 1, MAX_RADIUS) if len(fields) == 4 else DEFAULT_RADIUS
        return Spec("stat", radius, k=k, ratio=ratio, text=str(text))
    raise ValueError("--clean %s: the filter %r is neither 'radius' nor 'stat'" % (text, kind))


def parse_specs(specs):
    """a spec, or a list of them (strings or Spec) -> [Spec]"""
    if isinstance(specs, (str, Spec)):
        specs = [specs]
    return [parse_spec(s) for s in specs]


def threshold(S, ratio):
    """the statistical filter's bound on S (int64 numpy): mean + ratio * population std, numpy's float64 reductions"""
    return np.mean(S) + ratio * np.std(S)


def bits_for(points):
    """the fewest bits that hold the largest coordinate of an integer cloud (at least 1)"""
    points = np.asarray(points)
    if not len(points):
        raise ValueError("clean: the cloud has no points")
    if int(points.min()) < 0:
        raise ValueError("clean: a voxelised cloud has no negative coordinates (smallest: %d)" % int(points.min()))
    bits = max(1, int(points.max()).bit_length())
    if bits > MAX_BITS:
        raise ValueError("clean: the largest coordinate %d needs %d bits, the grid holds %d" % (int(points.max()), bits, MAX_BITS))
    return bits


def _device_voxels(points):
    """int32 [n,3] on the device, from numpy or a tensor"""
    import torch
    dev = _lib.require_gpu()
    p = points if torch.is_tensor(points) else torch.from_numpy(np.ascontiguousarray(np.asarray(points).reshape(-1, 3).astype(np.int32)))
    return p.to(dev, torch.int32).reshape(-1, 3).contiguous()


def neighbor_statistics(points, bits, k, radius, want_counts=True):
    """points int32 [n,3] (distinct voxels; numpy or a tensor) -> device tensors (S int64 [n] | None when k == 0, cnt int32 [n] |
    None when not wanted): pcgc_clean_neighbors"""
    import torch
    p_d = _device_voxels(points)
    n = int(p_d.shape[0])
    if n == 0:
        raise ValueError("clean: the cloud has no points")
    if k == 0 and not want_counts:
        raise ValueError("clean: k = 0 and no counts: nothing to compute")
    lib = _lib.hip()
    size = int(lib.pcgc_clean_workspace_bytes(bits, n))
    if size == 0:
        raise ValueError("clean: bits = %r outside 1..%d, or %d points too many" % (bits, MAX_BITS, n))
    ws = torch.empty(size, dtype=torch.uint8, device=p_d.device)
    S = torch.empty(n, dtype=torch.int64, device=p_d.device) if k else None
    cnt = torch.empty(n, dtype=torch.int32, device=p_d.device) if want_counts else None
    _lib.check(lib.pcgc_clean_neighbors(_lib.dptr(p_d), n, bits, k, radius, _lib.dptr(S), _lib.dptr(cnt), _lib.dptr(ws), ws.numel(),
                                        _lib.stream()), "pcgc_clean_neighbors")
    return S, cnt


def _download(t):
    """a device vector to the host through page-locked memory, as ingest.merge reads its rows back"""
    import torch
    host = torch.empty(tuple(t.shape), dtype=t.dtype, pin_memory=True)
    host.copy_(t, non_blocking=True)
    torch.cuda.current_stream().synchronize()
    return host.numpy()


def keep_mask(points, bits, spec):
    """-> host bool [n]: the voxels one filter keeps"""
    spec = parse_spec(spec)
    if spec.kind == "radius":
        return _download(neighbor_statistics(points, bits, 0, spec.radius)[1]) >= spec.min_count
    S = _download(neighbor_statistics(points, bits, spec.k, spec.radius, want_counts=False)[0])
    return S <= threshold(S, spec.ratio)


def keep_mask_all(points, bits, specs):
    """-> host bool [n]: what the filters keep, applied in order, each on what the one before kept.  ValueError when nothing
    would remain."""
    import torch
    specs = parse_specs(specs)
    p_d = _device_voxels(points)
    mask = None
    for spec in specs:
        if mask is None:
            mask = keep_mask(p_d, bits, spec)
        else:
            alive = np.flatnonzero(mask)
            mask[alive[~keep_mask(p_d[torch.from_numpy(alive).to(p_d.device)], bits, spec)]] = False
        if not mask.any():
            raise ValueError("--clean %s removes every voxel that was left" % spec.text)
    return mask if mask is not None else np.ones(int(p_d.shape[0]), bool)


def clean_cloud(points, colors, normals, counts, bits, specs):
    """A voxelised cloud (points int32 [n,3], distinct; colors, normals, counts [n, ...] or None) through the filters in order
    -> (points, colors, normals, counts, mask bool [n]), the kept rows in their order.  ValueError when nothing would remain."""
    points = np.asarray(points)
    mask = keep_mask_all(points, bits, specs)
    pick = lambda a: None if a is None else np.asarray(a)[mask]
    return points[mask], pick(colors), pick(normals), pick(counts), mask


def n_cubes(points, cube_bits=6):
    """occupied 64^3 cubes of an integer cloud"""
    c = np.asarray(points).astype(np.int64) >> cube_bits
    return len(np.unique((c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]))


def summary_line(specs, n_before, n_removed, cubes_before, cubes_after, n_input_points=None):
    """clean: stat:20:2.0 removed 412 of 183004 voxels (455 input points); 64^3 cubes 391 -> 207"""
    rows = "" if n_input_points is None else " ({} input points)".format(n_input_points)
    return "clean: {} removed {} of {} voxels{}; 64^3 cubes {} -> {}".format(" ".join(s.text for s in parse_specs(specs)), n_removed,
                                                                              n_before, rows, cubes_before, cubes_after)


# ---------------------------------------------------------------------------- command line
def add_clean_argument(ap):
    ap.add_argument("--clean", action="append", default=None, metavar="SPEC",
                    help="drop outlier voxels (pcgcv1_amd/clean.py): radius:R:MIN keeps a voxel with at least MIN occupied voxels within "
                         "R cells; stat:K:RATIO[:R] keeps one whose summed distance to its K nearest voxels within R (default 8) cells "
                         "is at most mean + RATIO * std over the cloud.  Repeatable: applied in order")


def check_clean_argument(ap, args):
    """parse the specs with the other argument errors; args.clean becomes [Spec] or None"""
    if args.clean:
        try:
            args.clean = parse_specs(args.clean)
        except ValueError as e:
            ap.error(str(e))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="drop the outlier voxels of a voxelised ply")
    ap.add_argument("--input", required=True, help="the voxelised ply: integer coordinates, one point per voxel")
    ap.add_argument("--output", required=True, help="the cleaned ply; colours or normals are carried through")
    add_clean_argument(ap)
    args = ap.parse_args(argv)
    if not args.clean:
        ap.error("give at least one --clean SPEC")
    check_clean_argument(ap, args)
    return args


def main(argv=None):
    from .dataprocess.inout_points import load_ply_scan, write_ply_colors, write_ply_data, write_ply_normals
    args = parse_args(argv)
    try:
        scan, colors, normals = load_ply_scan(args.input)
        if not len(scan):
            raise ValueError("no points")
        if not (np.isfinite(scan).all() and (scan == np.floor(scan)).all()):
            raise ValueError("not a voxelised ply: a coordinate is not an integer (python -m pcgcv1_amd.ingest voxelises a scan)")
        points = scan.astype(np.int32)
        if len(np.unique(points, axis=0)) != len(points):
            raise ValueError("not a voxelised ply: a voxel holds several points (python -m pcgcv1_amd.ingest merges them)")
        kept, colors, normals, _, mask = clean_cloud(points, colors, normals, None, bits_for(points), args.clean)
    except ValueError as e:
        raise SystemExit("clean: %s: %s" % (args.input, e))
    if colors is not None:
        write_ply_colors(args.output, kept, colors)
    elif normals is not None:
        write_ply_normals(args.output, kept, normals)
    else:
        write_ply_data(args.output, kept)
    print(summary_line(args.clean, len(points), len(points) - len(kept), n_cubes(points), n_cubes(kept)))
    print("wrote {}".format(args.output))


if __name__ == "__main__":
    main()
