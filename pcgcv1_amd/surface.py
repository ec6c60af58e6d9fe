"""A triangle mesh from a voxel cloud, on the GPU (include/pcgc.h, pcgc_surface_*; csrc/surface.hip; DESIGN.md §7l;
tests/_surface_ref.py is the rule in numpy).

Three parts: the estimated normals, which come unoriented, are given one consistent side per component by parallel propagation
from a seed; a moving-least-squares signed distance is evaluated at the corners of the unit boxes around the voxels and their
neighbours; marching tetrahedra over the Kuhn cut of those boxes give an indexed mesh, closed and consistently wound wherever the
cloud is a closed sheet.  torch sorts and uniques (the seeds per component, the lattice edges that carry a vertex); everything
else is a kernel.

A fourth, optional part makes the mesh small enough to use (pcgc_simplify_*; csrc/simplify.hip; DESIGN.md §7m;
tests/_simplify_ref.py is its rule): the vertices in a cube of CELL voxels become one, placed by the quadric of the triangles
that touch the cube, and the triangles follow as a chain.  It runs on the device, before the mesh goes to the host.

    python -m pcgcv1_amd.surface --input X_rec.ply --output X.obj [--radius R] [--orient given|propagate[:G]|view:X,Y,Z]
                                 [--estimate_normals] [--frame X.frame] [--simplify CELL] [--error]

--error measures the voxels against the mesh that is written (metrics.mesh_error): one more line of the summary.
"""
import argparse
import ctypes
import os

import numpy as np

from . import _lib

MAX_BITS = 12
MIN_RADIUS, MAX_RADIUS, DEFAULT_RADIUS = 3, 8, 3
MAX_GAP, DEFAULT_GAP = 8, 1
DEFAULT_TAU = (0.9, 0.0)
MAX_STAGES = 8
NORM_TOLERANCE = 1e-3
MAX_CELL = 64               # simplify: the largest cluster cube, in voxels
PACK_LIMIT = 1 << 21        # simplify: three indices below this pack into one int64 sort key
ROUNDS_PER_READ = 32       # rounds queued per read-back of the state word; the result does not depend on it


# ---------------------------------------------------------------------------- specs
class Orient(object):
    """--orient: kind 'given', 'propagate' (gap) or 'view' (view = the three coordinates of the eye, in voxels)"""

    def __init__(self, kind, gap=DEFAULT_GAP, view=None, text=""):
        self.kind, self.gap, self.view, self.text = kind, gap, view, text or kind

    def __eq__(self, other):
        return isinstance(other, Orient) and (self.kind, self.gap, self.view) == (other.kind, other.gap, other.view)

    def __repr__(self):
        return "Orient(%r)" % self.text


def parse_orient(text):
    """'given' | 'propagate' | 'propagate:G' | 'view:X,Y,Z' -> Orient; a ValueError says what is wrong"""
    if isinstance(text, Orient):
        return text
    text = str(text)
    head, sep, rest = text.partition(":")
    if head == "given" and not sep:
        return Orient("given", text=text)
    if head == "propagate":
        if not sep:
            return Orient("propagate", DEFAULT_GAP, text=text)
        try:
            gap = int(rest)
        except ValueError:
            raise ValueError("surface: --orient %s: the gap %r is not an integer" % (text, rest))
        return Orient("propagate", check_gap(gap), text=text)
    if head == "view" and sep:
        f = rest.split(",")
        try:
            view = tuple(float(v) for v in f)
        except ValueError:
            view = ()
        if len(f) != 3 or len(view) != 3 or not all(np.isfinite(view)):
            raise ValueError("surface: --orient %s: view takes three finite numbers X,Y,Z" % text)
        return Orient("view", view=view, text=text)
    raise ValueError("surface: --orient %r is none of given, propagate[:G], view:X,Y,Z" % text)


def check_gap(gap):
    if not 1 <= int(gap) <= MAX_GAP:
        raise ValueError("surface: gap = %r outside 1..%d" % (gap, MAX_GAP))
    return int(gap)


def check_radius(radius):
    if int(radius) != radius or not MIN_RADIUS <= int(radius) <= MAX_RADIUS:
        raise ValueError("surface: radius = %r outside %d..%d" % (radius, MIN_RADIUS, MAX_RADIUS))
    return int(radius)


def check_tau(tau):
    tau = tuple(float(t) for t in tau)
    if not 1 <= len(tau) <= MAX_STAGES or not all(0.0 <= t <= 1.0 for t in tau):
        raise ValueError("surface: the stage thresholds %r must be 1 to %d values within [0, 1]" % (tau, MAX_STAGES))
    if tau[-1] != 0.0:
        raise ValueError("surface: the last stage threshold is %r, it must be 0.0 (the propagation would not end)" % (tau[-1],))
    return tau


def check_cell(cell):
    if isinstance(cell, bool) or int(cell) != cell or not 1 <= int(cell) <= MAX_CELL:
        raise ValueError("surface: simplify: cell = %r outside 1..%d" % (cell, MAX_CELL))
    return int(cell)


def check_bits(bits):
    if int(bits) != bits or not 1 <= int(bits) <= MAX_BITS:
        raise ValueError("surface: bits = %r outside 1..%d" % (bits, MAX_BITS))
    return int(bits)


# ---------------------------------------------------------------------------- mesh helpers (host)
def canonical(triangles):
    """every triangle rotated so that its smallest index comes first, the rows sorted: two meshes that differ in the order of the
    triangles and the rotation of each compare equal"""
    t = np.asarray(triangles).reshape(-1, 3)
    first = np.argmin(t, 1)
    t = np.stack([t[np.arange(len(t)), (first + s) % 3] for s in range(3)], 1)
    return t[np.lexsort((t[:, 2], t[:, 1], t[:, 0]))]


def boundary_edges(triangles):
    """the number of undirected edges that lie in exactly one triangle (0 for a closed mesh)"""
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    if not len(t):
        return 0
    e = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), 1)
    _, count = np.unique(e[:, 0] * (int(t.max()) + 1) + e[:, 1], return_counts=True)
    return int((count == 1).sum())


def write_mesh(filename, vertices, triangles):
    """.obj or .off; floats as repr writes them, so that read_triangle_mesh returns the same float64 and int32 arrays"""
    ext = os.path.splitext(filename)[1].lower()
    if ext not in (".obj", ".off"):
        raise ValueError("%s: a mesh is written as .obj or .off" % filename)
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    if len(t) and (t.min() < 0 or t.max() >= len(v)):
        raise ValueError("write_mesh: a triangle names a vertex outside 0..%d" % (len(v) - 1))
    rows = [" ".join(repr(x) for x in row) for row in v.tolist()]
    if ext == ".obj":
        lines = ["v " + r for r in rows] + ["f %d %d %d" % tuple(r) for r in (t + 1).tolist()]
    else:
        lines = ["OFF", "%d %d 0" % (len(v), len(t))] + rows + ["3 %d %d %d" % tuple(r) for r in t.tolist()]
    with open(filename, "w") as f:
        f.write("\n".join(lines) + "\n")


# ---------------------------------------------------------------------------- device
def _validated(points, normals, bits):
    """int32 [n,3] and float32 [n,3] (or None) on the device; a ValueError names the first bad row"""
    import torch
    dev = _lib.require_gpu()
    bits = check_bits(bits)
    p = points if torch.is_tensor(points) else torch.from_numpy(np.ascontiguousarray(np.asarray(points).reshape(-1, 3).astype(np.int32)))
    p = p.to(dev, torch.int32).reshape(-1, 3).contiguous()
    n = int(p.shape[0])
    if n == 0:
        raise ValueError("surface: the cloud has no points")
    res = 1 << bits
    out = ((p < 0) | (p >= res)).any(1)
    key = (p[:, 0].long() * res + p[:, 1].long()) * res + p[:, 2].long()
    skey, at = torch.sort(key)
    same = skey[1:] == skey[:-1]
    bad = None
    if normals is not None:
        nr = normals if torch.is_tensor(normals) else torch.from_numpy(np.ascontiguousarray(np.asarray(normals, np.float32).reshape(-1, 3)))
        nr = nr.to(dev, torch.float32).reshape(-1, 3).contiguous()
        if nr.shape[0] != n:
            raise ValueError("surface: %d points and %d normals" % (n, nr.shape[0]))
        d = nr.double()
        bad = ~(torch.isfinite(d).all(1) & ((d * d).sum(1).sub(1.0).abs() <= NORM_TOLERANCE))
    else:
        nr = None
    flags = torch.stack([out.any(), same.any(), bad.any() if bad is not None else out.any() & False]).tolist()   # one read-back
    if flags[0]:
        row = int(out.nonzero()[0])
        raise ValueError("surface: row %d, voxel %s, lies outside the grid of %d cells per axis" % (row, p[row].tolist(), res))
    if flags[1]:
        k = int(same.nonzero()[0])
        raise ValueError("surface: rows %d and %d are the same voxel %s: the voxels must be distinct (a duplicate)" % (
            int(at[k]), int(at[k + 1]), p[int(at[k])].tolist()))
    if flags[2]:
        row = int(bad.nonzero()[0])
        raise ValueError("surface: row %d: the normal %s is not finite or not of unit length (| |n|^2 - 1 | <= %g)" % (
            row, nr[row].tolist(), NORM_TOLERANCE))
    return p, nr, key, bits


class _Lattice(object):
    """the workspace of one cloud and the calls that share it"""

    def __init__(self, p, bits):
        import torch
        self.p, self.bits, self.n = p, bits, int(p.shape[0])
        self.lib = _lib.hip()
        size = int(self.lib.pcgc_surface_workspace_bytes(bits, self.n))
        if size == 0:
            raise ValueError("surface: bits = %r outside 1..%d, or %d points too many" % (bits, MAX_BITS, self.n))
        self.ws = torch.empty(size, dtype=torch.uint8, device=p.device)
        self.torch = torch

    def _args(self):
        return _lib.dptr(self.ws), self.ws.numel(), _lib.stream()

    def orient(self, normals, seed, gap, tau, batch=ROUNDS_PER_READ):
        torch = self.torch
        sign = torch.empty(self.n, dtype=torch.int8, device=self.p.device)
        tau_c = (ctypes.c_double * len(tau))(*tau)
        rounds, reads = ctypes.c_int32(0), ctypes.c_int32(0)
        _lib.check(self.lib.pcgc_surface_orient(_lib.dptr(self.p), _lib.dptr(normals), _lib.dptr(seed), self.n, self.bits, gap,
                                                ctypes.cast(tau_c, ctypes.c_void_p), len(tau), batch, _lib.dptr(sign),
                                                ctypes.cast(ctypes.byref(rounds), ctypes.c_void_p),
                                                ctypes.cast(ctypes.byref(reads), ctypes.c_void_p), *self._args()), "pcgc_surface_orient")
        return sign, int(rounds.value), int(reads.value)

    def lattice(self):
        counts = self.torch.empty(2, dtype=self.torch.int64, device=self.p.device)
        _lib.check(self.lib.pcgc_surface_lattice(_lib.dptr(self.p), self.n, self.bits, _lib.dptr(counts), *self._args()),
                   "pcgc_surface_lattice")
        self.n_cells, self.n_vertices = (int(v) for v in counts.tolist())
        return self.n_cells, self.n_vertices

    def implicit(self, oriented, radius):
        torch = self.torch
        vkeys = torch.empty(self.n_vertices, dtype=torch.int64, device=self.p.device)
        f = torch.empty(self.n_vertices, dtype=torch.float64, device=self.p.device)
        _lib.check(self.lib.pcgc_surface_implicit(_lib.dptr(oriented), self.n, self.bits, radius, self.n_vertices, _lib.dptr(vkeys),
                                                  _lib.dptr(f), *self._args()), "pcgc_surface_implicit")
        return vkeys, f

    def triangle_ids(self, f):
        torch = self.torch
        count = torch.empty(1, dtype=torch.int64, device=self.p.device)
        _lib.check(self.lib.pcgc_surface_triangles(_lib.dptr(f), self.n_vertices, self.n, self.bits, 0, None, _lib.dptr(count), *self._args()),
                   "pcgc_surface_triangles")
        T = int(count.item())
        ids = torch.empty((T, 3), dtype=torch.int64, device=self.p.device)
        if T:
            _lib.check(self.lib.pcgc_surface_triangles(_lib.dptr(f), self.n_vertices, self.n, self.bits, T, _lib.dptr(ids), None, *self._args()),
                       "pcgc_surface_triangles")
        return ids

    def mesh(self, f, tri_ids):
        torch = self.torch
        T = int(tri_ids.shape[0])
        if T == 0:
            return (torch.empty((0, 3), dtype=torch.float64, device=self.p.device), torch.empty((0, 3), dtype=torch.int32, device=self.p.device))
        edge_ids = torch.unique(tri_ids.reshape(-1))                      # sorted: ascending id
        V = int(edge_ids.shape[0])
        vertices = torch.empty((V, 3), dtype=torch.float64, device=self.p.device)
        triangles = torch.empty((T, 3), dtype=torch.int32, device=self.p.device)
        _lib.check(self.lib.pcgc_surface_mesh(_lib.dptr(edge_ids), V, _lib.dptr(tri_ids), T, _lib.dptr(f), self.n_vertices, self.n, self.bits,
                                              _lib.dptr(vertices), _lib.dptr(triangles), *self._args()), "pcgc_surface_mesh")
        return vertices, triangles


def _seeds(p, key, bits, gap):
    """uint8 [n]: 1 at the voxel with the largest key of every component -> (seed, number of components).  Two sorts, by key and
    then stably by label, leave every component's largest key at the end of its run: no atomic maximum, which on a cloud of one
    component is n updates of one word."""
    import torch
    from .clean import components
    label, _, n_components = components(p, bits, gap)
    _, at = torch.sort(key)
    lab, idx = torch.sort(label[at], stable=True)
    last = torch.ones_like(lab, dtype=torch.bool)
    last[:-1] = lab[1:] != lab[:-1]
    seed = torch.zeros(p.shape[0], dtype=torch.uint8, device=p.device)
    seed[at[idx[last]]] = 1
    return seed, n_components


def _orient(lat, nr, key, spec, tau, report):
    import torch
    p = lat.p
    if spec.kind == "given":
        return torch.ones(lat.n, dtype=torch.int8, device=p.device), 0
    if spec.kind == "view":
        d, q = nr.double(), p.double()
        X, Y, Z = spec.view
        dot = (d[:, 0] * (X - q[:, 0]) + d[:, 1] * (Y - q[:, 1])) + d[:, 2] * (Z - q[:, 2])
        return torch.where(dot < 0, -1, 1).to(torch.int8), 0
    seed, n_components = _seeds(p, key, lat.bits, spec.gap)
    sign, rounds, reads = lat.orient(nr, seed, spec.gap, tau)
    if report is not None:
        report["components"] = int(n_components.item())
        report["readbacks"] = reads
    return sign, rounds


def _spec(mode, gap):
    spec = parse_orient(mode)
    if spec.kind == "propagate" and ":" not in spec.text:
        spec = Orient("propagate", check_gap(gap), text=spec.text)
    return spec


def orient(points, normals, bits, mode="propagate", gap=DEFAULT_GAP, tau=DEFAULT_TAU, report=None):
    """points int32 [n,3] distinct voxels, normals float32 [n,3] of unit length -> (sign int8 [n] numpy, rounds): the oriented
    normal is sign * normal.  mode: 'given', 'view:X,Y,Z' or 'propagate[:G]' (gap is used when the mode names none)."""
    spec, tau = _spec(mode, gap), check_tau(tau)
    p, nr, key, bits = _validated(points, normals, bits)
    if nr is None:
        raise ValueError("surface: orient needs normals")
    sign, rounds = _orient(_Lattice(p, bits), nr, key, spec, tau, report)
    return sign.cpu().numpy(), rounds


def _boundary_edges_device(triangles, n_vertices):
    """boundary_edges on the device tensor: a sort of the 3 T undirected edges"""
    import torch
    if triangles.shape[0] == 0:
        return 0
    t = triangles.long()
    a, b = torch.cat([t[:, 0], t[:, 1], t[:, 2]]), torch.cat([t[:, 1], t[:, 2], t[:, 0]])
    _, count = torch.unique(torch.minimum(a, b) * n_vertices + torch.maximum(a, b), return_counts=True)
    return int((count == 1).sum().item())


def _oriented_device(oriented_normals, n, dev):
    import torch
    N = oriented_normals if torch.is_tensor(oriented_normals) else torch.from_numpy(np.ascontiguousarray(np.asarray(oriented_normals, np.float64)))
    N = N.to(dev, torch.float64).reshape(-1, 3).contiguous()
    if N.shape[0] != n:
        raise ValueError("surface: %d points and %d normals" % (n, N.shape[0]))
    return N


def implicit(points, oriented_normals, bits, radius=DEFAULT_RADIUS):
    """-> (vertex_keys int64 [V] ascending, f float64 [V]) numpy: the signed distance at the lattice vertices"""
    radius = check_radius(radius)
    p, _, _, bits = _validated(points, None, bits)
    N = _oriented_device(oriented_normals, int(p.shape[0]), p.device)
    lat = _Lattice(p, bits)
    lat.lattice()
    vkeys, f = lat.implicit(N, radius)
    return vkeys.cpu().numpy(), f.cpu().numpy()


def bits_for(points):
    """the fewest bits that hold the largest coordinate (at least 1)"""
    from .clean import bits_for as clean_bits_for
    return clean_bits_for(points)


# ---------------------------------------------------------------------------- simplification
def _validated_mesh(vertices, triangles, bits):
    """float64 [V,3] and int32 [T,3] on the device; a ValueError names the first bad row (one read-back)"""
    import torch
    dev = _lib.require_gpu()
    v = vertices if torch.is_tensor(vertices) else torch.from_numpy(np.ascontiguousarray(np.asarray(vertices, np.float64).reshape(-1, 3)))
    v = v.to(dev, torch.float64).reshape(-1, 3).contiguous()
    t = triangles if torch.is_tensor(triangles) else torch.from_numpy(np.ascontiguousarray(np.asarray(triangles).reshape(-1, 3).astype(np.int64)))
    t = t.to(dev).reshape(-1, 3)
    V, T = int(v.shape[0]), int(t.shape[0])
    if V >= 2 ** 31 or 3 * T >= 2 ** 31:
        raise ValueError("surface: simplify: %d vertices and %d triangles are too many (V and 3 T below 2^31)" % (V, T))
    hi = float((1 << bits) + 2)
    bad_v = ~(torch.isfinite(v) & (v >= -2.0) & (v < hi)).all(1)
    bad_t = ((t < 0) | (t >= V)).any(1)
    flags = torch.stack([bad_v.any(), bad_t.any()]).tolist()             # one read-back
    if flags[0]:
        row = int(bad_v.nonzero()[0])
        raise ValueError("surface: simplify: vertex row %d, %s, is not finite or lies outside [-2, %d)" % (row, v[row].tolist(), int(hi)))
    if flags[1]:
        row = int(bad_t.nonzero()[0])
        raise ValueError("surface: simplify: triangle row %d, %s, names a vertex outside 0..%d" % (row, t[row].tolist(), V - 1))
    return v, t.to(torch.int32).contiguous()


def _sorted_rows(a, b, c, limit, pack_limit):
    """the order that sorts the rows (a, b, c) of int64 columns below `limit` lexicographically: one sort of the packed rows
    where three columns fit 63 bits, stable sorts from the last column to the first otherwise"""
    import torch
    if limit <= pack_limit <= PACK_LIMIT:
        return torch.argsort(a << 42 | b << 21 | c, stable=True)
    order = torch.argsort(c, stable=True)
    return order[torch.argsort((a << 31 | b)[order], stable=True)]


def _canonical_device(t, n_vertices, pack_limit):
    """canonical() on the device tensor int32 [T,3]"""
    import torch
    t = t.long()
    first = torch.where((t[:, 0] <= t[:, 1]) & (t[:, 0] <= t[:, 2]), 0, torch.where(t[:, 1] <= t[:, 2], 1, 2))
    cols = [torch.gather(t, 1, ((first + s) % 3)[:, None])[:, 0] for s in range(3)]
    order = _sorted_rows(cols[0], cols[1], cols[2], n_vertices, pack_limit)
    return torch.stack(cols, 1)[order].to(torch.int32).contiguous()


class _Simplifier(object):
    """the steps of the rule on device tensors, one method per part (tools/surface_bench.py times them one by one)"""

    def __init__(self, v, bits, cell, pack_limit=None):
        import torch
        self.torch, self.lib, self.v, self.bits, self.cell = torch, _lib.hip(), v, bits, cell
        self.V, self.dev = int(v.shape[0]), v.device
        self.pack_limit = PACK_LIMIT if pack_limit is None else int(pack_limit)

    def clusters(self):
        torch = self.torch
        keys = torch.empty(self.V, dtype=torch.int64, device=self.dev)
        _lib.check(self.lib.pcgc_simplify_keys(_lib.dptr(self.v), self.V, self.bits, self.cell, _lib.dptr(keys), _lib.stream()), "pcgc_simplify_keys")
        self.keys, rank = torch.unique(keys, return_inverse=True)
        self.K = int(self.keys.shape[0])
        self.rank = rank.to(torch.int32).contiguous()
        self.marks = torch.arange(self.K + 1, dtype=torch.int32, device=self.dev)
        by_rank, self.vert_index = torch.sort(self.rank, stable=True)
        self.vert_start = torch.searchsorted(by_rank, self.marks).contiguous()
        return self.K

    def incidence(self, t):
        torch = self.torch
        T = int(t.shape[0])
        if T == 0:
            self.tri_entry, self.tri_start = None, torch.zeros(self.K + 1, dtype=torch.int64, device=self.dev)
            return
        words = torch.empty(T * 3, dtype=torch.int32, device=self.dev)
        _lib.check(self.lib.pcgc_simplify_incidence(_lib.dptr(t), T, _lib.dptr(self.rank), self.V, self.K, _lib.dptr(words), _lib.stream()),
                   "pcgc_simplify_incidence")
        words, self.tri_entry = torch.sort(words, stable=True)
        self.tri_start = torch.searchsorted(words, self.marks).contiguous()

    def place(self, t):
        torch = self.torch
        placed = torch.empty((self.K, 3), dtype=torch.float64, device=self.dev)
        fallback = torch.empty(self.K, dtype=torch.uint8, device=self.dev)
        T = int(t.shape[0])
        _lib.check(self.lib.pcgc_simplify_place(_lib.dptr(self.v), self.V, _lib.dptr(t) if T else None, T, _lib.dptr(self.keys), self.K, self.bits,
                                                self.cell, _lib.dptr(self.tri_start), _lib.dptr(self.tri_entry), _lib.dptr(self.vert_start),
                                                _lib.dptr(self.vert_index), _lib.dptr(placed), _lib.dptr(fallback), _lib.stream()),
                   "pcgc_simplify_place")
        return placed, fallback

    def remap(self, t):
        """-> (rows int64 [n,3]: the distinct triples ascending, mult int64 [n], total int64 [n], the number of degenerate triangles
        (a device scalar))"""
        torch = self.torch
        T = int(t.shape[0])
        if T == 0:
            none = torch.zeros(0, dtype=torch.int64, device=self.dev)
            return none.reshape(0, 3), none, none, none.sum()
        packs = self.K <= self.pack_limit <= PACK_LIMIT
        triples = torch.empty((T, 3), dtype=torch.int32, device=self.dev)
        sign = torch.empty(T, dtype=torch.int32, device=self.dev)
        packed = torch.empty(T, dtype=torch.int64, device=self.dev) if packs else None
        _lib.check(self.lib.pcgc_simplify_remap(_lib.dptr(t), T, _lib.dptr(self.rank), self.V, self.K, _lib.dptr(triples), _lib.dptr(sign),
                                                _lib.dptr(packed), _lib.stream()), "pcgc_simplify_remap")
        keep = triples[:, 0] >= 0
        sign = sign[keep].long()
        n_degenerate = T - keep.sum()
        if packs:
            uk, inv, total = torch.unique(packed[keep], return_inverse=True, return_counts=True)
            rows = torch.stack([uk >> 42, (uk >> 21) & (PACK_LIMIT - 1), uk & (PACK_LIMIT - 1)], 1)
        else:
            rows = triples[keep].long()
            order = _sorted_rows(rows[:, 0], rows[:, 1], rows[:, 2], self.K, self.pack_limit)
            rows, sign = rows[order], sign[order]
            new = torch.ones(rows.shape[0], dtype=torch.bool, device=self.dev)
            new[1:] = (rows[1:] != rows[:-1]).any(1)
            inv = torch.cumsum(new, 0) - 1
            rows = rows[new]
            total = torch.zeros(rows.shape[0], dtype=torch.int64, device=self.dev).index_add_(0, inv, torch.ones_like(inv))
        mult = torch.zeros(rows.shape[0], dtype=torch.int64, device=self.dev).index_add_(0, inv, sign)      # integer: any order, the same sum
        return rows, mult, total, n_degenerate


def _simplify_device(v, t, bits, cell, pack_limit=None):
    """the rule on validated device tensors -> (vertices float64 [V',3], triangles int32 [T',3], report), on the device"""
    import torch
    V, T = int(v.shape[0]), int(t.shape[0])
    report = dict(cell=cell, clusters=0, vertices_in=V, triangles_in=T, degenerate=0, cancelled=0, merged=0, folded=0, fallback=0, unused=0)
    if V == 0:
        return v, t, report
    s = _Simplifier(v, bits, cell, pack_limit)
    t = _canonical_device(t, V, s.pack_limit)
    K = s.clusters()
    s.incidence(t)
    placed, fallback = s.place(t)
    rows, mult, total, n_degenerate = s.remap(t)
    live = mult != 0
    kept, positive = rows[live], (mult[live] > 0)[:, None]
    tri = torch.where(positive, kept, kept[:, [0, 2, 1]])
    used = torch.unique(tri)
    counts = torch.stack([n_degenerate, (~live).sum(), (total > 1).sum(), (mult.abs() >= 2).sum(), fallback.sum()]).tolist()    # one read-back
    report.update(clusters=K, degenerate=counts[0], cancelled=counts[1], merged=counts[2], folded=counts[3], fallback=counts[4],
                  unused=K - int(used.shape[0]))
    return placed[used].contiguous(), torch.searchsorted(used, tri.contiguous()).to(torch.int32).reshape(-1, 3), report


def simplify(vertices, triangles, bits, cell, report=None, _pack_limit=None):
    """Quadric vertex clustering (include/pcgc.h, pcgc_simplify_*; tests/_simplify_ref.py is the rule in numpy): one vertex per
    cube of `cell` voxels, placed where the summed squared distance to the planes of the triangles that touch the cube is
    smallest; the triangles are the image of the input's oriented triangles.  vertices float64 [V,3] in voxel units within
    [-2, 2^bits + 2), triangles int32 [T,3] -> (vertices, triangles), numpy arrays or device tensors as given.  report (a dict)
    gains cell, clusters, vertices_in, triangles_in, degenerate, cancelled, merged, folded, fallback and unused.  _pack_limit (the
    tests'): the largest count whose rows are still ordered by one packed sort."""
    import torch
    bits, cell = check_bits(bits), check_cell(cell)
    as_tensors = torch.is_tensor(vertices)
    v, t = _validated_mesh(vertices, triangles, bits)
    v, t, rep = _simplify_device(v, t, bits, cell, _pack_limit)
    if report is not None:
        report.update(rep)
    return (v, t) if as_tensors else (v.cpu().numpy(), t.cpu().numpy())


def reconstruct(points, normals=None, bits=None, radius=DEFAULT_RADIUS, orient="propagate", frame=None, gap=DEFAULT_GAP, tau=DEFAULT_TAU,
                simplify=None, error=False):
    """points int32 [n,3] distinct voxels -> (vertices float64 [V,3], triangles int32 [T,3], report dict), numpy.  Without normals
    metrics.estimate_normals supplies them; without bits the frame's, or the fewest that hold the cloud.  The vertices are in
    voxel units (voxel q is the unit box about q), or with an ingest.Frame in the scan's own.  simplify: a cell size in voxels;
    the mesh goes through `simplify` on the device before it is measured and brought to the host (report["simplify"]).  error:
    the voxels are measured against the final mesh, on the device and in voxel units (metrics.mesh_error -> report["error"])."""
    radius, spec, tau = check_radius(radius), _spec(orient, gap), check_tau(tau)
    cell = None if simplify is None else check_cell(simplify)
    if bits is None:
        bits = frame.bits if frame is not None else bits_for(points.cpu().numpy() if hasattr(points, "cpu") else points)
    if normals is None:
        from .metrics import estimate_normals
        normals = estimate_normals(points)
    p, nr, key, bits = _validated(points, normals, bits)
    report = {"voxels": int(p.shape[0]), "readbacks": 0}
    lat = _Lattice(p, bits)
    sign, rounds = _orient(lat, nr, key, spec, tau, report)
    if "components" not in report:
        from .clean import components
        report["components"] = int(components(p, bits, DEFAULT_GAP)[2].item())
    N = (sign.double()[:, None] * nr.double()).contiguous()
    n_cells, n_lattice = lat.lattice()
    _, f = lat.implicit(N, radius)
    vertices, triangles = lat.mesh(f, lat.triangle_ids(f))
    if cell is not None:                                                  # in voxel units, before anything crosses to the host
        vertices, triangles, report["simplify"] = _simplify_device(vertices, triangles, bits, cell)
    if error:                                                             # the mesh as it leaves, before a frame rescales it
        from .metrics import mesh_error
        report["error"] = mesh_error(p, vertices, triangles)
    n_boundary = _boundary_edges_device(triangles, int(vertices.shape[0]))
    vertices, triangles = vertices.cpu().numpy(), triangles.cpu().numpy()
    report.update(rounds=rounds, cells=n_cells, lattice_vertices=n_lattice, vertices=len(vertices), triangles=len(triangles),
                  boundary_edges=n_boundary, sign=sign.cpu().numpy())
    if frame is not None:
        from .ingest import apply_frame
        vertices = apply_frame(vertices, frame)
    return vertices, triangles, report


def summary_line(report):
    """one line; a second one where the mesh was simplified, one more where it was measured against its voxels:
    simplify: cell 2, 6086 vertices and 12168 triangles -> 458 and 912, 18 of 458 clusters placed at their mean
    error: rms 0.423, max 1.055 voxels over 1954 points (cell edge 2, 3331 pairs)"""
    line = "surface: %d voxels, %d components, %d rounds, %d vertices, %d triangles, %d boundary edges" % tuple(
        report[k] for k in ("voxels", "components", "rounds", "vertices", "triangles", "boundary_edges"))
    if "simplify" in report:
        s = report["simplify"]
        line += "\nsimplify: cell %d, %d vertices and %d triangles -> %d and %d, %d of %d clusters placed at their mean" % (
            s["cell"], s["vertices_in"], s["triangles_in"], report["vertices"], report["triangles"], s["fallback"], s["clusters"])
    if "error" in report:
        e = report["error"]
        line += "\nerror: rms %.3f, max %.3f voxels over %d points (cell edge %d, %d pairs)" % (
            e["rms (p2mesh)"], float(np.sqrt(e["h. (p2mesh)"])), e["points"] - e["far"], e["edge"], e["pairs"])
    return line


# ---------------------------------------------------------------------------- command line
def check_output(filename):
    if os.path.splitext(filename)[1].lower() not in (".obj", ".off"):
        raise ValueError("%s: a mesh is written as .obj or .off" % filename)
    return filename


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="reconstruct a triangle mesh (.obj / .off) from a voxelised cloud (.ply) on the GPU",
                                 formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    ap.add_argument("--input", required=True, help="the voxelised cloud (.ply), with nx ny nz or with --estimate_normals")
    ap.add_argument("--output", required=True, help="the mesh to write (.obj or .off)")
    ap.add_argument("--radius", type=int, default=DEFAULT_RADIUS, help="support of the signed distance in voxels, %d..%d" % (MIN_RADIUS, MAX_RADIUS))
    ap.add_argument("--orient", default="propagate", metavar="given|propagate[:G]|view:X,Y,Z",
                    help="how the normals get a side: as they are, by propagation over links of gap G, or towards an eye")
    ap.add_argument("--estimate_normals", action="store_true", help="estimate the normals (radius 10, 20 neighbours) instead of reading them")
    ap.add_argument("--frame", default="", metavar="X.frame", help="write the vertices in the scan's units (pcgcv1_amd/ingest.py)")
    ap.add_argument("--simplify", type=int, default=None, metavar="CELL",
                    help="simplify the mesh on the GPU before it is written: one vertex per cube of CELL voxels (1..%d), placed by its quadric" % MAX_CELL)
    ap.add_argument("--error", action="store_true", help="measure the voxels against the mesh that is written: rms and largest distance, in voxels")
    args = ap.parse_args(argv)
    try:                                                                  # before any file is read
        if args.simplify is not None:
            check_cell(args.simplify)
        args.radius = check_radius(args.radius)
        args.orient = parse_orient(args.orient)
        check_output(args.output)
    except ValueError as e:
        ap.error(str(e))
    return args


def mesh_file(points, normals, output, radius=DEFAULT_RADIUS, orient="propagate", frame=None, simplify=None, error=False):
    """reconstruct (and simplify, and measure) and write -> the summary line (one more line with simplify, one more with error)"""
    vertices, triangles, report = reconstruct(points, normals, frame.bits if frame is not None else None, radius, orient, frame,
                                              simplify=simplify, error=error)
    write_mesh(output, vertices, triangles)
    return summary_line(report)


def main(argv=None):
    from .dataprocess.inout_points import load_ply_normals
    args = parse_args(argv)
    frame = None
    if args.frame:
        from .ingest import read_frame
        frame = read_frame(args.frame)
    points, normals = load_ply_normals(args.input)
    if args.estimate_normals:
        normals = None
    elif normals is None:
        raise SystemExit("%s has no nx ny nz properties: write them into the ply, or pass --estimate_normals" % args.input)
    print(mesh_file(points, normals, args.output, args.radius, args.orient, frame, args.simplify, args.error))
    print("wrote " + args.output)


if __name__ == "__main__":
    main()
