"""What D1 / D2 of a scaled-back (off-grid) reconstruction costs per call: metrics.pc_error(..., off_grid="host") against
off_grid="device", and the on-grid kernels on the same A against the rounded B as the yardstick of a grid search at that
size.  The pair is tests/_clouds.faces(1, 1024, 700000) and its reconstruction at scale 5/8, normals all ones.

    python tools/offgrid_bench.py [--repeats 7] > profiles/offgrid_bench.txt

Per path: two warm-up calls, then the median (and the range) of `repeats` calls, each timed with a host clock around the
call and a device synchronise (every path ends in a device-to-host read of its figures anyway)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from _clouds import faces                                                # noqa: E402
from pcgcv1_amd import _lib, metrics                                     # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--points", type=int, default=700000)
    a_ = ap.parse_args()
    _lib.require_gpu()
    scale = 5 / 8.
    a = faces(1, a_.res, a_.points)[0]
    b = np.unique(np.round(a.astype("float32") * scale), axis=0).astype("float32") * float(1 / scale)       # process.py's round trip
    b_grid = np.unique(np.rint(b).astype(np.int32), axis=0)
    na = np.ones((len(a), 3), np.float32)
    assert metrics._off_grid(b)
    print("pair: faces(1, %d, %d), scale 5/8: %d / %d points (%d after rounding B to the grid), normals all ones; %d repeats"
          % (a_.res, a_.points, len(a), len(b), len(b_grid), a_.repeats))
    paths = (("off-grid, host (scipy k-d tree)", lambda: metrics.pc_error(a, b, na, a_.res - 1, off_grid="host")),
             ("off-grid, device (csrc/offgrid.hip)", lambda: metrics.pc_error(a, b, na, a_.res - 1, off_grid="device")),
             ("on-grid kernels, B rounded", lambda: metrics.pc_error(a, b_grid, na, a_.res - 1)))
    results = {}
    for name, fn in paths:
        out, ts = timed(fn, a_.repeats)
        results[name] = out
        print("%-38s median %9.2f ms   (min %9.2f, max %9.2f)   mseF,PSNR p2point %.4f  p2plane %.4f"
              % (name, 1e3 * statistics.median(ts), 1e3 * min(ts), 1e3 * max(ts), out["mseF,PSNR (p2point)"], out["mseF,PSNR (p2plane)"]))
        sys.stdout.flush()
    _, ts = timed(lambda: np.unique(b, axis=0), a_.repeats)
    print("%-38s median %9.2f ms   (host only: both off-grid paths start with it)" % ("np.unique of B's rows", 1e3 * statistics.median(ts)))
    host, dev = results[paths[0][0]], results[paths[1][0]]
    worst = max(abs(dev[k] - host[k]) / max(abs(host[k]), 1e-300) for k in host)
    print("device against host, largest relative difference over the %d keys: %.3g" % (len(host), worst))


if __name__ == "__main__":
    main()
