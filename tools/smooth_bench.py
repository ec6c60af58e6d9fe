"""What thinning a scan costs: ingest.voxelize_scan with and without smooth="3:2" (csrc/smooth.hip) on the scan of
tools/ingest_bench.py: `--points` points (default 4 000 000) scattered within half a millimetre of a sphere of radius 0.35 m,
at --bits 10 (a step of about 0.7 mm, so the noise is about 0.36 voxel per axis and a ball of 3 voxels holds about 35 points).

    python tools/smooth_bench.py [--repeats 5] > profiles/smooth_bench.txt
    python tools/smooth_bench.py --host              # also the host's way: scipy's cKDTree.query_ball_point (16 workers) + the moments
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/smooth_bench.py --profile      # kernel times: tools/rocpd_stats.py

Per line: two warm-up calls, then the median (and the range) of `repeats` calls, each timed with a host clock around the call
and a device synchronise.  "whole call" starts from numpy arrays on the host and ends with numpy arrays on the host; the stage
lines work on a cloud that is already on the device and sorted by cell."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from ingest_bench import line, make_scan, timed                          # noqa: E402
from pcgcv1_amd import _lib, ingest, register, smooth                    # noqa: E402


def host_rule(g, radius, workers, chunk=250000):
    """the neighbourhoods and the moments on the host, float64, `chunk` query points at a time (the lists of 4 M balls do not
    fit otherwise) -> (seconds for the tree and the ball queries, seconds for the moments, K).  The eigenvectors and the move
    are left out: they are n small solves either way."""
    from scipy.spatial import cKDTree
    g64 = g.astype(np.float64)
    t0 = time.perf_counter()
    tree = cKDTree(g64)
    t_ball, t_moments, counts = time.perf_counter() - t0, 0.0, []
    for c0 in range(0, len(g64), chunk):
        t0 = time.perf_counter()
        ball = tree.query_ball_point(g64[c0:c0 + chunk], radius, workers=workers, return_sorted=False)
        t1 = time.perf_counter()
        K = np.fromiter((len(b) for b in ball), np.int64, len(ball))
        j = np.concatenate(ball).astype(np.int64)
        i = np.repeat(np.arange(c0, c0 + len(K)), K)
        o = np.rint((g64[j] - g64[i]) * 65536.0).astype(np.int64)
        first = np.concatenate([[0], np.cumsum(K)[:-1]])
        np.add.reduceat(np.concatenate([o, o[:, :1] * o, o[:, 1:2] * o[:, 1:], o[:, 2:] * o[:, 2:]], 1), first, axis=0)
        t_ball, t_moments = t_ball + (t1 - t0), t_moments + (time.perf_counter() - t1)
        counts.append(K)
    return t_ball, t_moments, np.concatenate(counts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--points", type=int, default=4000000)
    ap.add_argument("--bits", type=int, default=10)
    ap.add_argument("--spec", default="3:2")
    ap.add_argument("--host", action="store_true", help="time the host rule on the same points as well (tens of seconds)")
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--profile", action="store_true", help="three smoothed whole calls and nothing else: for a kernel trace")
    a = ap.parse_args()
    _lib.require_gpu()
    spec = smooth.parse_spec(a.spec)
    points, colors = make_scan(a.points)
    if a.profile:
        for _ in range(3):
            ingest.voxelize_scan(points, colors, bits=a.bits, smooth=spec)
        torch.cuda.synchronize()
        return
    plain, ts_plain = timed(lambda: ingest.voxelize_scan(points, colors, bits=a.bits), a.repeats)
    thin, ts_thin = timed(lambda: ingest.voxelize_scan(points, colors, bits=a.bits, smooth=spec), a.repeats)
    frame = plain[4]
    print("scan: %d points with colours, %d bits, step %.6g, --smooth %s; %d repeats" % (a.points, a.bits, frame.step, spec.text, a.repeats))
    print("occupied voxels: %d raw, %d smoothed (each on its own fitted frame)" % (len(plain[0]), len(thin[0])))
    line("whole call, no smoothing", ts_plain)
    line("whole call, smooth=%s" % spec.text, ts_thin)
    g = register.to_grid(points, frame)
    line("  to grid units on the host (float64 -> float32)", timed(lambda: register.to_grid(points, frame), a.repeats)[1])
    line("  smooth_grid: %d passes, host arrays in and out" % spec.iters, timed(lambda: smooth.smooth_grid(g, spec.radius, spec.iters, spec.kmin),
                                                                              a.repeats)[1])
    g_d = torch.from_numpy(g).cuda()
    cells = register.cells_from_bounds(g.min(0).astype(np.float64), g.max(0).astype(np.float64), spec.radius, "smooth")
    order, ts = timed(lambda: register.cell_order(g_d, cells), a.repeats)
    line("  sort by cell on the device (torch)", ts)
    sorted_d = g_d[order].contiguous()
    (out, moved, K, _, _), ts = timed(lambda: smooth.smooth_step(sorted_d, cells, spec.radius, spec.kmin, debug=True), a.repeats)
    line("  pcgc_smooth_step, one pass, with K S Q", ts)
    line("  pcgc_smooth_step, one pass (cells, kernel, flag)", timed(lambda: smooth.smooth_step(sorted_d, cells, spec.radius, spec.kmin), a.repeats)[1])
    K = K.cpu().numpy()
    print("cells of edge %g, %d per axis; neighbours per point: mean %.1f, most %d; moved %d of %d"
          % (cells[0], cells[4], K.mean(), K.max(), int((moved != 0).sum().item()), a.points))
    sys.stdout.flush()
    if a.host:
        t_ball, t_moments, K_host = host_rule(g, spec.radius, a.workers)
        print("%-46s        %9.2f ms   (host, one run, %d workers)" % ("cKDTree build + query_ball_point", 1e3 * t_ball, a.workers))
        print("%-46s        %9.2f ms   (host, one run, numpy)" % ("the moments of those neighbourhoods", 1e3 * t_moments))
        # the tree decides membership by its own float64 distance: the counts may differ from the rule's by points at exactly r
        print("neighbour counts, host against device: %d of %d differ" % (int((K_host[order.cpu().numpy()] != K).sum()), a.points))


if __name__ == "__main__":
    main()
