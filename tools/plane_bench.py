"""What the plane filter costs: pcgc_plane_count alone at 256, 1024 and 4096 draws and pcgc_plane_select with and without its sums
on the voxels of tools/ingest_bench.py's scan (4 000 000 points with colours near a sphere, 10 bits, 2.9 M occupied voxels), then
clean.keep_mask for plane:1.5 as a whole.  The scan holds no plane, so the filter keeps everything; the kernels do the same work
per voxel and draw whatever the cloud is.

    python tools/plane_bench.py [--repeats 10] > profiles/plane_bench.txt
    python tools/plane_bench.py --numpy           # for scale: the scorer of tests/_plane_ref.py on the CPU, 64 draws
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/plane_bench.py --profile 1024     # kernel times: tools/rocpd_stats.py

Per line: two warm-up calls, then the median (and the range) of `repeats` calls, each timed with a host clock around the call
and a device synchronise."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from ingest_bench import line, make_scan, timed                           # noqa: E402
from components_bench import voxels                                       # noqa: E402
from pcgcv1_amd import _lib, clean                                       # noqa: E402

DRAWS = (256, 1024, 4096)
D2 = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--points", type=int, default=4000000)
    ap.add_argument("--bits", type=int, default=10)
    ap.add_argument("--profile", type=int, default=0, metavar="DRAWS", help="three calls of pcgc_plane_count at that many draws and three of pcgc_plane_select, nothing else: for a kernel trace")
    ap.add_argument("--numpy", action="store_true", help="tests/_plane_ref.py's scorer on the CPU as well (64 draws, one run)")
    a = ap.parse_args()
    _lib.require_gpu()
    points, _ = make_scan(a.points)
    vox = voxels(points, a.bits)
    n = len(vox)
    host = vox.cpu().numpy()
    planes = {k: torch.from_numpy(clean.draw_planes(lambda rows: host[rows], D2, k, 0, n)).cuda() for k in set(DRAWS) | {a.profile or DRAWS[0]}}
    if a.profile:
        for _ in range(3):
            clean.plane_counts(vox, a.bits, planes[a.profile])
        for _ in range(3):
            clean.plane_select(vox, a.bits, planes[a.profile][0])
        torch.cuda.synchronize()
        return
    print("the scan of tools/ingest_bench.py: %d points, %d bits: %d occupied voxels; D = %.1f; %d repeats" % (len(points), a.bits, n, D2 / 2, a.repeats))
    for k in DRAWS:
        counts, ts = timed(lambda: clean.plane_counts(vox, a.bits, planes[k]), a.repeats)
        tests = n * k / statistics.median(ts)
        line("pcgc_plane_count, %d draws" % k, ts, "   %.0f G point-plane tests per second; the best draw holds %d voxels" % (tests / 1e9, counts.max().item()))
    best = planes[DRAWS[1]][int(clean.plane_counts(vox, a.bits, planes[DRAWS[1]]).argmax().item())]
    (mask, sums), ts = timed(lambda: clean.plane_select(vox, a.bits, best), a.repeats)
    line("pcgc_plane_select, mask and sums", ts, "   %d inliers" % sums[0].item())
    refit = clean.refit_plane(sums.cpu().numpy(), D2)
    (mask, sums), ts = timed(lambda: clean.plane_select(vox, a.bits, refit), a.repeats)
    line("pcgc_plane_select, the refit plane", ts, "   %d inliers, |a| up to 2^%d" % (sums[0].item(), int(np.abs(refit[:3]).max()).bit_length()))
    line("pcgc_plane_select, mask only", timed(lambda: clean.plane_select(vox, a.bits, refit, want_sums=False), a.repeats)[1])
    t0 = time.perf_counter()
    drawn = clean.draw_planes(lambda rows: host[rows], D2, DRAWS[1], 0, n)
    print("%-46s        %9.2f ms   (host, one run)" % ("clean.draw_planes, %d draws (rows on the host)" % DRAWS[1], 1e3 * (time.perf_counter() - t0)))
    for spec in ("plane:1.5:0.05:256", "plane:1.5", "plane:1.5:0.05:4096"):
        report = []
        keep, ts = timed(lambda: clean.keep_mask(vox, a.bits, spec, report), a.repeats)
        line("keep_mask %s (draws, rows, counts, two selects)" % spec, ts, "   kept %d of %d" % (keep.sum(), n))
    print(report[-1])
    if a.numpy:
        import _plane_ref as ref
        t0 = time.perf_counter()
        want = ref.counts(host, a.bits, drawn[:64])
        dt = time.perf_counter() - t0
        same = np.array_equal(want, clean.plane_counts(vox, a.bits, drawn[:64]).cpu().numpy())
        print("numpy scorer (tests/_plane_ref.py), 64 draws (CPU, one call): %.2f s, %.2f G tests per second; the device's counts %s"
              % (dt, n * 64 / dt / 1e9, "identical" if same else "DIFFER"))


if __name__ == "__main__":
    main()
