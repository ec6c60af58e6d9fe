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

Both judge a voxel by its own neighbourhood, so a small dense island (a clump of flying pixels, a piece of the turntable, a
second object) passes them.  Connected components (include/pcgc.h, pcgc_clean_components; csrc/components.hip;
tests/_components_ref.py): two voxels are linked when max(|dx|, |dy|, |dz|) <= G, the gap; label(p) = the smallest key
(x * res + y) * res + z of p's component, size(p) = its number of voxels.

  component:MIN[:G]  keep p when size(p) >= MIN                                      1 <= MIN <= 2^31 - 1, 1 <= G <= 8, G = 1 when left out
  largest[:G]        keep p when label(p) is the label of the largest component, the smallest label among equals

    python -m pcgcv1_amd.clean --input vox.ply --output vox_clean.ply --clean stat:20:2.0 --clean largest:2

The command lines print one more line per such filter: the number of components and the sizes of the three largest, as that
filter saw them.

`largest` drops a piece of the turntable only when that piece is already detached.  The surface a scanned object stands on is
dense and touches the object, so all four filters above keep it; the plane filter finds it and takes it away, after which the
object is an island and `largest` finishes the job (include/pcgc.h, pcgc_plane_count and pcgc_plane_select; csrc/plane.hip;
tests/_plane_ref.py).  A plane is five int64 numbers (a, b, c, d, T) and a voxel is an inlier when |a x + b y + c z - d| <= T:

  plane:D[:FRAC[:DRAWS[:SEED]]]   drop the voxels within D cells of the dominant plane when they are at least FRAC of the cloud
                                  D a multiple of 0.5 in 0.5 .. 32 (D2 = 2 D), 0 < FRAC <= 1 (0.05), 1 <= DRAWS <= 65536 (1024),
                                  0 <= SEED <= 2^31 - 1 (0)

  1. draws: np.random.default_rng(SEED).integers(0, n, (DRAWS, 3)) names three rows p0, p1, p2 per draw; (a, b, c) = cross(p1 - p0,
     p2 - p0), d = (a, b, c) . p0, T = isqrt(D2^2 (a^2 + b^2 + c^2)) // 2 in Python integers (exactly 2 |s| <= D2 |(a, b, c)|), T = -1
     for a repeated or collinear triple.  The host needs only those 3 DRAWS rows of the cloud.
  2. score: the device counts every draw's inliers; the best draw has the most, the lowest index among equals.  All counts 0: no
     plane.
  3. refit: the device sums 1, x, y, z, x^2, y^2, z^2, xy, xz, yz over the best draw's inliers (int64); the host forms the float64
     covariance, takes np.linalg.eigh's eigenvector v of the smallest eigenvalue, nq = rint(2^16 v), and the plane (N nq, nq . sum p,
     isqrt(D2^2 N^2 |nq|^2) // 2).  The final plane is the one of the two with more inliers, the refit among equals.
  4. decision: final count >= FRAC * n drops the final inliers, anything less keeps every voxel.

    python -m pcgcv1_amd.clean --input vox.ply --output vox_clean.ply --clean stat:20:2.0 --clean plane:1.5 --clean largest:2

It prints a line of its own as well: the unit normal, the offset along it, the final count, the best draw's and the draws.
"""
import argparse
import math

import numpy as np

from . import _lib

MAX_BITS, MAX_K, MAX_RADIUS, DEFAULT_RADIUS = 12, 64, 32, 8
MAX_GAP, DEFAULT_GAP, MAX_MIN_SIZE = 8, 1, 2 ** 31 - 1
MAX_DIST2, DEFAULT_FRAC, MAX_DRAWS, DEFAULT_DRAWS, MAX_SEED = 64, 0.05, 65536, 1024, 2 ** 31 - 1
NORMAL_BITS = 16


class Spec(object):
    """one --clean filter: kind 'radius' (radius, min_count), 'stat' (k, ratio, radius), 'component' (min_count, gap), 'largest'
    (gap) or 'plane' (dist2 = twice the distance in cells, frac, draws, seed); text = the spec as given"""

    def __init__(self, kind, radius=0, k=0, ratio=0.0, min_count=0, text="", gap=DEFAULT_GAP, dist2=0, frac=DEFAULT_FRAC,
                 draws=DEFAULT_DRAWS, seed=0):
        self.kind, self.radius, self.k, self.ratio, self.min_count, self.text, self.gap = kind, radius, k, ratio, min_count, text, gap
        self.dist2, self.frac, self.draws, self.seed = dist2, frac, draws, seed

    def __eq__(self, other):
        return isinstance(other, Spec) and self._key() == other._key()

    def _key(self):
        return self.kind, self.radius, self.k, self.ratio, self.min_count, self.gap, self.dist2, self.frac, self.draws, self.seed

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
    """'radius:R:MIN', 'stat:K:RATIO[:R]', 'component:MIN[:G]', 'largest[:G]' or 'plane:D[:FRAC[:DRAWS[:SEED]]]' -> Spec; ValueError
    names the field that is wrong"""
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
    if kind == "component":
        if len(fields) not in (2, 3):
            raise ValueError("--clean %s: the component filter is component:MIN[:G] (%d fields given)" % (text, len(fields)))
        min_count = _int_field(text, "MIN", fields[1], 1, MAX_MIN_SIZE)
        gap = _int_field(text, "G", fields[2], 1, MAX_GAP) if len(fields) == 3 else DEFAULT_GAP
        return Spec("component", min_count=min_count, gap=gap, text=str(text))
    if kind == "largest":
        if len(fields) not in (1, 2):
            raise ValueError("--clean %s: the largest-component filter is largest[:G] (%d fields given)" % (text, len(fields)))
        return Spec("largest", gap=_int_field(text, "G", fields[1], 1, MAX_GAP) if len(fields) == 2 else DEFAULT_GAP, text=str(text))
    if kind == "plane":
        if len(fields) not in (2, 3, 4, 5):
            raise ValueError("--clean %s: the plane filter is plane:D[:FRAC[:DRAWS[:SEED]]] (%d fields given)" % (text, len(fields)))
        try:
            dist2 = 2 * float(fields[1])
        except ValueError:
            raise ValueError("--clean %s: D = %r is not a number" % (text, fields[1]))
        if not (math.isfinite(dist2) and dist2 == math.floor(dist2) and 1 <= dist2 <= MAX_DIST2):
            raise ValueError("--clean %s: D = %r must be a multiple of 0.5 in 0.5..%d" % (text, fields[1], MAX_DIST2 // 2))
        frac = DEFAULT_FRAC
        if len(fields) > 2:
            try:
                frac = float(fields[2])
            except ValueError:
                raise ValueError("--clean %s: FRAC = %r is not a number" % (text, fields[2]))
            if not 0 < frac <= 1:                                            # a nan fails both
                raise ValueError("--clean %s: FRAC = %r must be above 0 and at most 1" % (text, fields[2]))
        draws = _int_field(text, "DRAWS", fields[3], 1, MAX_DRAWS) if len(fields) > 3 else DEFAULT_DRAWS
        seed = _int_field(text, "SEED", fields[4], 0, MAX_SEED) if len(fields) > 4 else 0
        return Spec("plane", text=str(text), dist2=int(dist2), frac=frac, draws=draws, seed=seed)
    raise ValueError("--clean %s: the filter %r is neither 'radius', 'stat', 'component', 'largest' nor 'plane'" % (text, kind))


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


def components(points, bits, gap=DEFAULT_GAP):
    """points int32 [n,3] (distinct voxels; numpy or a tensor) -> device tensors (label int64 [n], size int32 [n], n_components
    int64 [1]): pcgc_clean_components.  A point outside the grid gets label -1 and size 0."""
    import torch
    p_d = _device_voxels(points)
    n = int(p_d.shape[0])
    if n == 0:
        raise ValueError("clean: the cloud has no points")
    lib = _lib.hip()
    size = int(lib.pcgc_clean_components_workspace_bytes(bits, n))
    if size == 0:
        raise ValueError("clean: bits = %r outside 1..%d, or %d points too many" % (bits, MAX_BITS, n))
    ws = torch.empty(size, dtype=torch.uint8, device=p_d.device)
    label = torch.empty(n, dtype=torch.int64, device=p_d.device)
    sizes = torch.empty(n, dtype=torch.int32, device=p_d.device)
    n_components = torch.empty(1, dtype=torch.int64, device=p_d.device)
    _lib.check(lib.pcgc_clean_components(_lib.dptr(p_d), n, bits, gap, _lib.dptr(label), _lib.dptr(sizes), _lib.dptr(n_components),
                                         _lib.dptr(ws), ws.numel(), _lib.stream()), "pcgc_clean_components")
    return label, sizes, n_components


def plane_counts(points, bits, planes):
    """points int32 [n,3] (numpy or a tensor), planes int64 [K,5] (a, b, c, d, T) -> device tensor int32 [K], the inliers of every
    plane: pcgc_plane_count"""
    import torch
    p_d = _device_voxels(points)
    planes = planes if torch.is_tensor(planes) else torch.from_numpy(np.ascontiguousarray(np.asarray(planes, np.int64).reshape(-1, 5)))
    planes = planes.to(p_d.device, torch.int64).reshape(-1, 5).contiguous()
    counts = torch.empty(int(planes.shape[0]), dtype=torch.int32, device=p_d.device)
    _lib.check(_lib.hip().pcgc_plane_count(_lib.dptr(p_d), int(p_d.shape[0]), bits, _lib.dptr(planes), int(planes.shape[0]),
                                           _lib.dptr(counts), _lib.stream()), "pcgc_plane_count")
    return counts


def plane_select(points, bits, plane, want_sums=True):
    """points int32 [n,3], plane int64 [5] -> device tensors (mask uint8 [n], 1 = inlier; sums int64 [10] over the inliers: N, x,
    y, z, x^2, y^2, z^2, xy, xz, yz | None when not wanted): pcgc_plane_select"""
    import torch
    p_d = _device_voxels(points)
    plane = plane if torch.is_tensor(plane) else torch.from_numpy(np.ascontiguousarray(np.asarray(plane, np.int64).reshape(5)))
    plane = plane.to(p_d.device, torch.int64).reshape(5).contiguous()
    mask = torch.empty(int(p_d.shape[0]), dtype=torch.uint8, device=p_d.device)
    sums = torch.empty(10, dtype=torch.int64, device=p_d.device) if want_sums else None
    _lib.check(_lib.hip().pcgc_plane_select(_lib.dptr(p_d), int(p_d.shape[0]), bits, _lib.dptr(plane), _lib.dptr(mask), _lib.dptr(sums),
                                            _lib.stream()), "pcgc_plane_select")
    return mask, sums


def plane_threshold(D2, nn):
    """T of a plane whose normal has the squared length nn (a Python integer): |s| <= T is exactly 2 |s| <= D2 sqrt(nn)"""
    return math.isqrt(D2 * D2 * int(nn)) // 2


def draw_planes(points_at, D2, draws, seed, n):
    """step 1 of the plane rule on the host -> int64 [draws,5].  points_at(rows int64 [m]) -> the voxels of those rows [m,3]: the
    3 * draws rows the triples name are all it reads of the cloud"""
    tri = np.random.default_rng(seed).integers(0, n, (draws, 3))
    p = np.asarray(points_at(tri.reshape(-1)), np.int64).reshape(draws, 3, 3)
    normal = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    nn = (normal * normal).sum(1)
    planes = np.empty((draws, 5), np.int64)
    planes[:, :3] = normal
    planes[:, 3] = (normal * p[:, 0]).sum(1)
    planes[:, 4] = [plane_threshold(D2, v) if v else -1 for v in nn.tolist()]     # a repeated or collinear triple matches nothing
    return planes


def refit_plane(sums, D2):
    """step 3 of the plane rule on the host: the ten int64 sums over a plane's inliers -> the least-squares plane int64 [5]"""
    N, sx, sy, sz, xx, yy, zz, xy, xz, yz = [int(v) for v in sums]
    mu = np.array([sx, sy, sz], np.float64) / N
    cov = np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]], np.float64) / N - np.outer(mu, mu)
    v = np.linalg.eigh(cov)[1][:, 0]                                          # ascending eigenvalues
    nq = [int(c) for c in np.rint(v * 2.0 ** NORMAL_BITS).astype(np.int64)]
    return np.array([N * nq[0], N * nq[1], N * nq[2], nq[0] * sx + nq[1] * sy + nq[2] * sz,
                     plane_threshold(D2, N * N * (nq[0] * nq[0] + nq[1] * nq[1] + nq[2] * nq[2]))], np.int64)


def segment_plane(points, bits, spec):
    """The plane rule for one spec -> (plane int64 [5] | None when no draw has an inlier, mask: device uint8 [n], 1 = within D of
    that plane, info: n, draws, best_count (the best draw's inliers), count (the final plane's), dropped (count >= FRAC * n))"""
    import torch
    spec = parse_spec(spec)
    p_d = _device_voxels(points)
    n = int(p_d.shape[0])
    if n == 0:
        raise ValueError("clean: the cloud has no points")
    planes = draw_planes(lambda rows: _download(p_d[torch.from_numpy(rows).to(p_d.device)]), spec.dist2, spec.draws, spec.seed, n)
    counts = _download(plane_counts(p_d, bits, planes))
    best = int(np.argmax(counts))                                         # the lowest index among equals
    info = dict(n=n, draws=spec.draws, best_count=int(counts[best]), count=0, dropped=False)
    if info["best_count"] == 0:
        return None, torch.zeros(n, dtype=torch.uint8, device=p_d.device), info
    plane = planes[best]
    mask, sums = plane_select(p_d, bits, plane)
    refit = refit_plane(_download(sums), spec.dist2)
    refit_mask, refit_sums = plane_select(p_d, bits, refit)
    info["count"] = int(_download(refit_sums)[0])
    if info["count"] >= info["best_count"]:
        plane, mask = refit, refit_mask
    else:
        info["count"] = info["best_count"]
    info["dropped"] = info["count"] >= spec.frac * n
    return plane, mask, info


def plane_line(spec, plane, info):
    """plane: plane:1.5 dropped normal (-0.1261 0.2032 0.9710) offset 41.77: 26987 of 41014 voxels (best of 1024 draws: 26069), or
    plane: plane:4:0.9 no plane holds 0.9 of the voxels: the best has normal ...; plane = None: no draw had an inlier"""
    if plane is None:
        return "plane: {} no plane holds {:g} of the voxels: none of {} draws spans a plane".format(spec.text, spec.frac, info["draws"])
    a, b, c, d = [int(v) for v in plane[:4]]
    length = math.sqrt(a * a + b * b + c * c)
    if max((a, b, c), key=abs) < 0:                                      # the same plane: its largest component points up
        a, b, c, d = -a, -b, -c, -d
    found = "normal ({:.4f} {:.4f} {:.4f}) offset {:.2f}: {} of {} voxels (best of {} draws: {})".format(
        a / length, b / length, c / length, d / length, info["count"], info["n"], info["draws"], info["best_count"])
    if info["dropped"]:
        return "plane: {} dropped {}".format(spec.text, found)
    return "plane: {} no plane holds {:g} of the voxels: the best has {}".format(spec.text, spec.frac, found)


def _download(t):
    """a device vector to the host through page-locked memory, as ingest.merge reads its rows back"""
    import torch
    host = torch.empty(tuple(t.shape), dtype=t.dtype, pin_memory=True)
    host.copy_(t, non_blocking=True)
    torch.cuda.current_stream().synchronize()
    return host.numpy()


def components_line(spec, label, size):
    """components: largest:2 saw 28 components, the largest of 3002 125 5 voxels (label, size: host arrays, one row per voxel)"""
    first = np.unique(label[label >= 0], return_index=True)[1]           # one row of every component
    top = np.sort(size[label >= 0][first])[::-1][:3]
    return "components: {} saw {} components, the largest of {} voxels".format(spec.text, len(first), " ".join(str(int(s)) for s in top))


def keep_mask(points, bits, spec, report=None):
    """-> host bool [n]: the voxels one filter keeps.  report (a list): a component filter appends its components_line, a plane
    filter its plane_line"""
    spec = parse_spec(spec)
    if spec.kind == "plane":
        plane, mask, info = segment_plane(points, bits, spec)
        if report is not None:
            report.append(plane_line(spec, plane, info))
        return _download(mask) == 0 if info["dropped"] else np.ones(info["n"], bool)
    if spec.kind in ("component", "largest"):
        label, size, _ = components(points, bits, spec.gap)
        label, size = _download(label), _download(size)
        if report is not None:
            report.append(components_line(spec, label, size))
        if spec.kind == "component":
            return size >= spec.min_count
        return label == label[size == size.max()].min()                  # the largest; the smallest label among equals
    if spec.kind == "radius":
        return _download(neighbor_statistics(points, bits, 0, spec.radius)[1]) >= spec.min_count
    S = _download(neighbor_statistics(points, bits, spec.k, spec.radius, want_counts=False)[0])
    return S <= threshold(S, spec.ratio)


def keep_mask_all(points, bits, specs, report=None):
    """-> host bool [n]: what the filters keep, applied in order, each on what the one before kept.  ValueError when nothing
    would remain.  report: as keep_mask"""
    import torch
    specs = parse_specs(specs)
    p_d = _device_voxels(points)
    mask = None
    for spec in specs:
        if mask is None:
            mask = keep_mask(p_d, bits, spec, report)
        else:
            alive = np.flatnonzero(mask)
            mask[alive[~keep_mask(p_d[torch.from_numpy(alive).to(p_d.device)], bits, spec, report)]] = False
        if not mask.any():
            raise ValueError("--clean %s removes every voxel that was left" % spec.text)
    return mask if mask is not None else np.ones(int(p_d.shape[0]), bool)


def clean_cloud(points, colors, normals, counts, bits, specs, report=None):
    """A voxelised cloud (points int32 [n,3], distinct; colors, normals, counts [n, ...] or None) through the filters in order
    -> (points, colors, normals, counts, mask bool [n]), the kept rows in their order.  ValueError when nothing would remain.
    report: as keep_mask"""
    points = np.asarray(points)
    mask = keep_mask_all(points, bits, specs, report)
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
                         "is at most mean + RATIO * std over the cloud; component:MIN[:G] keeps a voxel whose connected component "
                         "(voxels at most G cells apart per axis are linked, default 1) has at least MIN voxels; largest[:G] keeps the "
                         "largest component; plane:D[:FRAC[:DRAWS[:SEED]]] drops the voxels within D cells (a multiple of 0.5) of the "
                         "dominant plane, found by DRAWS seeded RANSAC draws (default 1024, seed 0) and refitted by least squares, "
                         "when they are at least FRAC of the cloud (default 0.05): the floor or the table.  Repeatable: applied in "
                         "order")


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
        report = []
        kept, colors, normals, _, mask = clean_cloud(points, colors, normals, None, bits_for(points), args.clean, report)
    except ValueError as e:
        raise SystemExit("clean: %s: %s" % (args.input, e))
    if colors is not None:
        write_ply_colors(args.output, kept, colors)
    elif normals is not None:
        write_ply_normals(args.output, kept, normals)
    else:
        write_ply_data(args.output, kept)
    print("\n".join([summary_line(args.clean, len(points), len(points) - len(kept), n_cubes(points), n_cubes(kept))] + report))
    print("wrote {}".format(args.output))


if __name__ == "__main__":
    main()
