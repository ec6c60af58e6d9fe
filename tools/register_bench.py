"""What registration costs (pcgcv1_amd/register.py, csrc/offgrid.hip: pcgc_register_*): two independent 1 M-point samplings
of the surface of tools/ingest_bench.py, squeezed to an ellipsoid with a bump so that no rotation leaves it unchanged, on
a 10-bit grid; the source is turned by 1 degree and shifted by a voxel.

    python tools/register_bench.py [--repeats 7] > profiles/register_bench.txt
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/register_bench.py --profile      # kernel times: tools/rocpd_stats.py

Medians (and ranges) of `repeats` calls after two warm calls, a host clock around the call and a device synchronise:
pcgc_register_prepare, one step with and without normals (the 45 sums read back, as the loop reads them), the whole icp, and
the same correspondences from scipy's cKDTree on the host's CPUs (build, and a query of every moved source point)."""
import argparse
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pcgcv1_amd import _lib, ingest, register                            # noqa: E402

SQUEEZE = np.array([1.0, 0.8, 0.6])


def timed(fn, repeats, warmup=2):
    for _ in range(warmup):
        out = fn()
    ts = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return out, ts


def make_scan(n, seed):
    """-> (points in metres, unit normals): ingest_bench's noisy sphere, squeezed per axis, with a bump along a skew direction"""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    bump = 1.0 + 0.08 * np.sin(3.0 * d[:, 0] + 2.0 * d[:, 1] + 0.7) * np.cos(2.0 * d[:, 2] - 0.4)
    points = 0.5 + 0.35 * SQUEEZE * d * bump[:, None] + rng.normal(0, 0.00025, (n, 3))
    normals = d / SQUEEZE                                      # the ellipsoid's; the bump tilts them by a few degrees
    return points, normals / np.linalg.norm(normals, axis=1, keepdims=True)


def line(name, ts, note=""):
    print("%-52s median %9.2f ms   (min %9.2f, max %9.2f)%s" % (name, 1e3 * statistics.median(ts), 1e3 * min(ts), 1e3 * max(ts), note))
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--bits", type=int, default=10)
    ap.add_argument("--profile", action="store_true", help="one prepare and three steps of each kind, nothing else: for a kernel trace")
    ap.add_argument("--threads", type=int, default=16, help="workers of the k-d tree query")
    a = ap.parse_args()
    _lib.require_gpu()
    (tp, tn), (sp, _) = make_scan(a.points, 1), make_scan(a.points, 2)
    frame = ingest.fit_frame(tp, bits=a.bits)
    target, src = register.to_grid(tp, frame), register.to_grid(sp, frame)
    centre = np.rint((target.astype(np.float64).min(0) + target.astype(np.float64).max(0)) / 2.0)
    R0 = register.rodrigues(np.array([1.0, 2.0, 3.0]) / math.sqrt(14.0) * math.radians(1.0))
    source = (src.astype(np.float64) @ R0.T + (centre - R0 @ centre) + np.array([0.6, -0.6, 0.5])).astype(np.float32)
    m = register.Matcher(source, target, tn)
    eye, zero = np.eye(3), np.zeros(3)
    if a.profile:
        for flag in (True, False):
            for _ in range(3):
                m.step(eye, zero, centre, 4.0, with_normals=flag)
        torch.cuda.synchronize()
        return
    print("pair: 2 x %d points, %d bits (step %.6g m), cells of edge %g, %d per axis; %d repeats" % (
        a.points, a.bits, frame.step, m.cells.h, m.cells.res, a.repeats))
    lib = _lib.hip()
    _, ts = timed(lambda: _lib.check(lib.pcgc_register_prepare(_lib.dptr(m.cells.points), m.m, *m.cells.grid(), _lib.dptr(m.ws),
                                                               m.ws.numel(), _lib.stream())), a.repeats)
    line("pcgc_register_prepare", ts, "   workspace %.0f MiB" % (m.ws.numel() / 2.0 ** 20))
    _, ts = timed(lambda: register.Matcher(source, target, tn), a.repeats)
    line("Matcher(...): upload, sort by cell, prepare", ts)
    for gate in (4.0, 1.0):
        for flag in (True, False):
            S, ts = timed(lambda: m.step(eye, zero, centre, gate, with_normals=flag), a.repeats)
            line("step, gate %g, %s" % (gate, "with normals" if flag else "no normals"), ts, "   n_used %d" % S[0])
    # the same source sorted by the cell it starts in, as icp sorts it once per stage: a wave's lanes then walk neighbouring cells
    ms = register.Matcher(source, target, tn)
    _, ts = timed(lambda: ms.sort_source(eye, zero), a.repeats)
    line("Matcher.sort_source", ts)
    for gate in (4.0, 1.0):
        S, ts = timed(lambda: ms.step(eye, zero, centre, gate), a.repeats)
        line("step, gate %g, with normals, source sorted by cell" % gate, ts, "   n_used %d" % S[0])
    for metric in ("plane", "point"):
        r, ts = timed(lambda: register.icp(source, target, tn, metric=metric), max(3, a.repeats // 2), warmup=1)
        line("icp, %s, schedule (4, 2, 1)" % metric, ts, "   steps %s, converged %s, fitness %.3f, rmse %.4f" % (
            r["iterations"], r["converged"], r["fitness"], r["rmse"]))
        moved = source.astype(np.float64) @ r["R"].T + r["t"]
        print("    the pose puts the source %.4f voxel (largest) from where it was sampled" % float(np.linalg.norm(moved - src, axis=1).max()))
    from scipy.spatial import cKDTree
    t64, s64 = target.astype(np.float64), source.astype(np.float64)
    tree, ts = timed(lambda: cKDTree(t64), 3, warmup=1)
    line("host: cKDTree(target)", ts)
    for gate in (4.0, 1.0):
        (d, _), ts = timed(lambda: tree.query(s64, k=1, distance_upper_bound=gate, workers=a.threads), a.repeats, warmup=1)
        line("host: tree.query, gate %g, %d workers" % (gate, a.threads), ts, "   n_used %d (one neighbour, no ties, no sums)" % int(np.isfinite(d).sum()))


if __name__ == "__main__":
    main()
