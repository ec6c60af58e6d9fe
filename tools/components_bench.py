"""What the component filters cost: pcgc_clean_components alone at G = 1, 2 and 8 on the voxels of tools/ingest_bench.py's scan
(4 000 000 points with colours near a sphere, 10 bits, 2.9 M occupied voxels), and ingest.voxelize_scan with clean="largest:2"
next to clean="stat:20:2.0" and to no clean at all.

    python tools/components_bench.py [--repeats 10] > profiles/components_bench.txt
    python tools/components_bench.py --scipy          # for scale: scipy.ndimage.label (3x3x3) on the dense grid, on the CPU
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/components_bench.py --profile G     # kernel times: tools/rocpd_stats.py

Per line: two warm-up calls, then the median (and the range) of `repeats` calls, each timed with a host clock around the call
and a device synchronise."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from ingest_bench import line, make_scan, timed                           # noqa: E402
from pcgcv1_amd import _lib, clean, ingest                               # noqa: E402

GAPS = (1, 2, 8)


def voxels(points, bits):
    """pass 1 of voxelize_scan_clean: the scan's voxels on the device"""
    p_d = torch.from_numpy(points).cuda()
    _, keys = ingest.quantize(p_d, ingest.fit_frame(p_d, bits=bits))
    rows = ingest.merge_device(keys, bits)
    return rows[0][:int(rows[4].item())]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--points", type=int, default=4000000)
    ap.add_argument("--bits", type=int, default=10)
    ap.add_argument("--profile", type=int, default=0, metavar="G", help="three calls of pcgc_clean_components at that gap and nothing else: for a kernel trace")
    ap.add_argument("--scipy", action="store_true", help="scipy.ndimage.label on the dense grid as well (gigabytes of host memory, tens of seconds)")
    a = ap.parse_args()
    _lib.require_gpu()
    points, colors = make_scan(a.points)
    vox = voxels(points, a.bits)
    if a.profile:
        for _ in range(3):
            clean.components(vox, a.bits, a.profile)
        torch.cuda.synchronize()
        return
    print("the scan of tools/ingest_bench.py: %d points with colours, %d bits: %d occupied voxels; %d repeats" % (len(points), a.bits, len(vox), a.repeats))
    for gap in GAPS:
        (label, size, n), ts = timed(lambda: clean.components(vox, a.bits, gap), a.repeats)
        line("pcgc_clean_components, G = %d" % gap, ts, "   %d components, the largest of %d voxels" % (n.item(), size.max().item()))
    out, ts = timed(lambda: ingest.voxelize_scan(points, colors, bits=a.bits), a.repeats)
    line("voxelize_scan (host arrays in and out)", ts)
    for spec in ("stat:20:2.0", "largest:2"):
        out, ts = timed(lambda: ingest.voxelize_scan(points, colors, bits=a.bits, clean=spec), a.repeats)
        line("voxelize_scan, clean=%s" % spec, ts, "   removed %d voxels (%d points), %d left" % (out[6], out[7], len(out[0])))
    spec = clean.parse_spec("largest:2")
    line("  keep_mask largest:2 (the call, label and size to the host, the mask)", timed(lambda: clean.keep_mask(vox, a.bits, spec), a.repeats)[1])
    if a.scipy:
        from scipy import ndimage
        res = 1 << a.bits
        v = vox.cpu().numpy()
        grid = np.zeros((res, res, res), bool)
        grid[v[:, 0], v[:, 1], v[:, 2]] = True
        t0 = time.perf_counter()
        _, count = ndimage.label(grid, structure=np.ones((3, 3, 3)))
        dt = time.perf_counter() - t0
        n = clean.components(vox, a.bits, 1)[2].item()
        print("scipy.ndimage.label, 3x3x3, on the dense %d^3 grid (CPU, one call): %.2f s, %d components (the device at G = 1: %d)" % (res, dt, count, n))


if __name__ == "__main__":
    main()
