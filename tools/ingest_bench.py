"""What putting a raw scan on the grid costs: ingest.voxelize_scan (csrc/ingest.hip) against the numpy rule of
tests/_ingest_ref.py on one synthetic scan with colours: `--points` points (default 4 000 000) scattered within half a
millimetre of a sphere of radius 0.35 m, at --bits 10 (a step of about 0.7 mm, 1.4 points per occupied voxel), and the same
scan at --bits 5 (about 900 points per voxel: the atomic passes under contention).

    python tools/ingest_bench.py [--repeats 7] > profiles/ingest_bench.txt
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/ingest_bench.py --profile 10      # kernel times: tools/rocpd_stats.py

Per line: two warm-up calls, then the median (and the range) of `repeats` calls, each timed with a host clock around the call
and a device synchronise.  "whole call" starts from numpy arrays on the host and ends with numpy arrays on the host; the stage
lines work on a cloud that is already on the device."""
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
import _ingest_ref as ref                                                # noqa: E402
from pcgcv1_amd import _lib, ingest                                      # noqa: E402


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


def make_scan(n, seed=1):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    points = 0.5 + 0.35 * d + rng.normal(0, 0.00025, (n, 3))           # metres
    colors = np.clip(128 + 100 * np.sin(9 * points) + rng.normal(0, 10, (n, 3)), 0, 255).astype(np.uint8)
    return points, colors


def line(name, ts, note=""):
    print("%-46s median %9.2f ms   (min %9.2f, max %9.2f)%s" % (name, 1e3 * statistics.median(ts), 1e3 * min(ts), 1e3 * max(ts), note))
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--points", type=int, default=4000000)
    ap.add_argument("--profile", type=int, default=0, metavar="BITS", help="three whole calls at that grid and nothing else: for a kernel trace")
    a = ap.parse_args()
    _lib.require_gpu()
    points, colors = make_scan(a.points)
    if a.profile:
        for _ in range(3):
            ingest.voxelize_scan(points, colors, bits=a.profile)
        torch.cuda.synchronize()
        return
    p_d, c_d = torch.from_numpy(points).cuda(), torch.from_numpy(colors).cuda()
    for bits in (10, 5):
        out, ts = timed(lambda: ingest.voxelize_scan(points, colors, bits=bits), a.repeats)
        frame, counts = out[4], out[3]
        print("scan: %d points with colours, %d bits, step %.6g: %d occupied voxels, %.2f points per voxel, at most %d; %d repeats"
              % (a.points, bits, frame.step, len(counts), a.points / len(counts), counts.max(), a.repeats))
        line("whole call (host arrays in and out)", ts)
        line("  pcgc_ingest_bounds (+ read-back)", timed(lambda: ingest.bounds(p_d), a.repeats)[1])
        (_, keys), ts = timed(lambda: ingest.quantize(p_d, frame), a.repeats)
        line("  pcgc_ingest_quantize", ts)
        rows, ts = timed(lambda: ingest.merge_device(keys, bits, c_d), a.repeats)
        line("  pcgc_ingest_merge", ts)
        line("  pcgc_ingest_merge + rows to the host (pinned)", timed(lambda: ingest.merge(keys, bits, c_d), a.repeats)[1])
        m = int(rows[4].item())
        line("  rows to the host, pageable (t.cpu())", timed(lambda: [t[:m].cpu() for t in rows[:3]], a.repeats)[1])
        line("  host -> device copy of points and colours", timed(lambda: (torch.from_numpy(points).cuda(), torch.from_numpy(colors).cuda()),
                                                                  a.repeats)[1])
        t0 = time.perf_counter()
        want = ref.voxelize_scan(points, colors, bits=bits)
        t_ref = time.perf_counter() - t0
        print("%-46s        %9.2f ms   (host, one run)" % ("numpy rule (tests/_ingest_ref.py)", 1e3 * t_ref))
        same = all(np.array_equal(out[k], want[k]) for k in (0, 1, 3)) and out[4] == ingest.Frame(*want[4])
        print("device against the numpy rule: points, colours, counts and frame %s" % ("identical" if same else "DIFFER"))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
