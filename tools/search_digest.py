"""One SHA-256 per output array of every kernel that searches a float32 cloud through the cells of csrc/offgrid_cells.h, on the
seeded cases the tests share (tests/_offgrid_ref.cases(), the uniform case of tests/test_gpu_register.py at n = 257 and 300 000).

    python tools/search_digest.py > profiles/search_digest.txt

The float64 sums of these kernels are added in a fixed order, so the same code on the same device gives the same bits.  A
refactor that claims to keep that order is checked by running this tool on a build of either commit: the listings must be
equal line for line.  (The tests bound the sums by the reference's summation error, which a reordering would pass.)  Only
Python entry points are used; a call that raises is listed with its message."""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _offgrid_ref as oref                                              # noqa: E402
from pcgcv1_amd import _lib, metrics, register, smooth                   # noqa: E402

GATES = {"twelve_ties": 4.0, "far": 100.0, "rod_edge_2": 60.0}           # tests/test_gpu_register.py; 2 for every other case


def emit(what, names, fn):
    try:
        arrays = fn()
    except (ValueError, RuntimeError) as e:
        print("%-44s %s: %s" % (what, type(e).__name__, e))
        return None
    for name, a in zip(names, arrays):
        a = np.ascontiguousarray(a.cpu().numpy() if torch.is_tensor(a) else a)
        print("%-44s %s %s %s" % ("%s %s" % (what, name), hashlib.sha256(a.tobytes()).hexdigest(), a.dtype, list(a.shape)))
    return arrays


def pose_about(c):
    """a small rotation about c and a shift, with entries that are not float32 numbers"""
    R = register.rodrigues(np.array([0.01, -0.02, 0.015]))
    return R, c - R @ c + np.array([0.3, -0.2, 0.1])


def colours(seed, n):
    return np.random.default_rng(seed).integers(0, 256, (n, 3)).astype(np.uint8)


def cells_of_edge(points, h):
    lo, hi = (np.floor(f(points.astype(np.float64), axis=0) / h) for f in (np.min, np.max))
    return (h, int(lo[0]), int(lo[1]), int(lo[2]), int((hi - lo).max()) + 1)


def digest(name, a, b, normals_b, gate):
    m = register.Matcher(a, b, normals_b)
    R, t = pose_about(m.centre)
    for sort in (False, True):
        if sort:
            m.sort_source(R, t)
        emit("%s step%s" % (name, " sorted" if sort else ""), ("S", "best", "ties"), lambda: m.step(R, t, m.centre, gate, per_point=True))
    emit("%s step no normals" % name, ("S",), lambda: (m.step(R, t, m.centre, gate, with_normals=False),))
    ca, cb = colours(len(a), len(a)), colours(len(b) + 1, len(b))

    def color_steps():
        cm = register.ColorMatcher(a, b, normals_b, ca, cb)
        out = cm.step(R, t, cm.centre, gate, per_point=True)
        cm.sort_source(R, t)
        return out + cm.step(R, t, cm.centre, gate, per_point=True)
    emit("%s color step" % name, ("S", "best", "ties", "S sorted", "best sorted", "ties sorted"), color_steps)
    Y = register.intensity(cb, len(b), "target")
    emit("%s gradient" % name, ("g", "valid", "K", "Q", "B"), lambda: register.color_gradient(b, normals_b, Y, debug=True))

    def smooth_once():
        g = torch.from_numpy(b).to(_lib.require_gpu())
        g64 = b.astype(np.float64)
        cells = register.cells_from_bounds(g64.min(0), g64.max(0), 3.0, "smooth")
        return smooth.smooth_step(g[register.cell_order(g, cells)].contiguous(), cells, 3.0, 6, debug=True)
    emit("%s smooth" % name, ("out", "moved", "K", "S", "Q"), smooth_once)
    for h in (None, 2.0, 1.0):                                  # feature_cells' own edge (4: one cell each way), then windows of 2 and 4
        cells, what = (None, "features") if h is None else (cells_of_edge(b, h), "features edge %g" % h)
        if cells is not None and cells[4] > 1024:
            continue
        got = emit("%s %s pairs" % (name, what), ("S", "k"), lambda: register.feature_pairs(b, normals_b, 3.0, cells))
        if got is not None:
            emit("%s %s combine" % (name, what), ("feat", "valid"),
                 lambda: register.feature_combine(b, normals_b, 3.0, got[0], got[1], cells))


def main():
    _lib.require_gpu()
    cases = dict(oref.cases())
    rng = np.random.default_rng(21)                            # the uniform case of tests/test_gpu_register.py
    q = rng.uniform(0, 20, (1000, 3)).astype(np.float32)
    p = rng.uniform(-1, 21, (300000, 3)).astype(np.float32)
    p[0] = q[0] + np.float32(0.125)
    for name in sorted(cases):
        a, b, normals_a = cases[name]
        digest(name, a, b, oref._normals(500 + len(b), len(b)), GATES.get(name, 2.0))

        def d1d2():
            figures, per = metrics.pc_error_float(a, b, normals_a, per_point=True)
            return (np.array([figures[k] for k in sorted(figures)]),) + per["1"] + per["2"] + (per["normals_b"],)
        emit("%s pc_error_float" % name, ("figures", "best1", "plane1", "ties1", "best2", "plane2", "ties2", "normals_b"), d1d2)
    for n in (257, 300000):
        digest("uniform n=%d" % n, p[:n], q, oref._normals(22, 1000), 1.5)


if __name__ == "__main__":
    main()
