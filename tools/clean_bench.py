"""What --clean costs on top of putting a raw scan on the grid: ingest.voxelize_scan with and without clean="stat:20:2.0" on the
scan of tools/ingest_bench.py (4 000 000 points with colours near a sphere, 10 bits, 2.9 M occupied voxels), and on the same
scan with 1 % stray points in a box three times its extent and one point ten extents away.

    python tools/clean_bench.py [--repeats 10] > profiles/clean_bench.txt
    python tools/clean_bench.py --unclean_only        # the first line alone: runs on a tree that has no --clean yet
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/clean_bench.py --profile      # kernel times: tools/rocpd_stats.py

Per line: two warm-up calls, then the median (and the range) of `repeats` calls, each timed with a host clock around the call
and a device synchronise.  The stage lines repeat what voxelize_scan_clean does, one step at a time, on tensors that are
already on the device."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from ingest_bench import line, make_scan, timed                           # noqa: E402
from pcgcv1_amd import _lib, ingest                                      # noqa: E402

SPEC = "stat:20:2.0"


def dirty(points, colors, seed=2):
    rng = np.random.default_rng(seed)
    lo, hi = points.min(0), points.max(0)
    mid, ext = (lo + hi) / 2, hi - lo
    strays = mid + rng.uniform(-1.5, 1.5, (len(points) // 100, 3)) * ext
    far = mid + np.array([[10.0, 0.0, 0.0]]) * ext.max()
    more = rng.integers(0, 256, (len(strays) + 1, 3)).astype(np.uint8)
    return np.r_[points, strays, far], np.r_[colors, more]


def stages(points, colors, bits, repeats):
    from pcgcv1_amd import clean
    spec = clean.parse_spec(SPEC)
    p_d, c_d = torch.from_numpy(points).cuda(), torch.from_numpy(colors).cuda()
    frame = ingest.fit_frame(p_d, bits=bits)
    _, keys = ingest.quantize(p_d, frame)
    rows, ts = timed(lambda: ingest.merge_device(keys, bits), repeats)
    line("  pass 1: pcgc_ingest_merge, positions only", ts)
    vox = rows[0][:int(rows[4].item())]
    (S, _), ts = timed(lambda: clean.neighbor_statistics(vox, bits, spec.k, spec.radius, want_counts=False), repeats)
    line("  pcgc_clean_neighbors (k = %d, R = %d), S only" % (spec.k, spec.radius), ts)
    line("  pcgc_clean_neighbors, S and cnt", timed(lambda: clean.neighbor_statistics(vox, bits, spec.k, spec.radius), repeats)[1])
    S_h, ts = timed(lambda: clean._download(S), repeats)
    line("  S to the host (page-locked, 8 bytes a voxel)", ts)
    line("  mean, std and the mask on the host (numpy)", timed(lambda: S_h <= clean.threshold(S_h, spec.ratio), repeats)[1])
    mask, ts = timed(lambda: clean.keep_mask(vox, bits, spec), repeats)
    line("  keep_mask: the four lines above together", ts)
    keep = torch.from_numpy(mask).cuda()
    res = 1 << bits

    def select():
        vox_keys = (vox[:, 0].long() * res + vox[:, 1].long()) * res + vox[:, 2].long()
        row_keep = keep[torch.searchsorted(vox_keys, keys).clamp_(max=len(vox_keys) - 1)] & (keys >= 0)
        return p_d[row_keep], c_d[row_keep]
    (kept, kept_c), ts = timed(select, repeats)
    line("  rows of the kept voxels (searchsorted, indexing)", ts)
    frame2 = ingest.fit_frame(kept, bits=bits)
    _, keys2 = ingest.quantize(kept, frame2)
    line("  pass 2: pcgc_ingest_merge + rows to the host", timed(lambda: ingest.merge(keys2, bits, kept_c), repeats)[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--points", type=int, default=4000000)
    ap.add_argument("--bits", type=int, default=10)
    ap.add_argument("--unclean_only", action="store_true")
    ap.add_argument("--profile", action="store_true", help="three whole calls with clean and nothing else: for a kernel trace")
    a = ap.parse_args()
    _lib.require_gpu()
    points, colors = make_scan(a.points)
    if a.profile:
        for _ in range(3):
            ingest.voxelize_scan(points, colors, bits=a.bits, clean=SPEC)
        torch.cuda.synchronize()
        return
    for name, (p, c) in (("the scan of tools/ingest_bench.py", (points, colors)), ("the same with 1 % strays and a far point", dirty(points, colors))):
        out, ts = timed(lambda: ingest.voxelize_scan(p, c, bits=a.bits), a.repeats)
        print("%s: %d points with colours, %d bits: %d occupied voxels, step %.6g; %d repeats" % (name, len(p), a.bits, len(out[0]), out[4].step, a.repeats))
        line("voxelize_scan (host arrays in and out)", ts)
        if a.unclean_only:
            break
        out, ts = timed(lambda: ingest.voxelize_scan(p, c, bits=a.bits, clean=SPEC), a.repeats)
        line("voxelize_scan, clean=%s" % SPEC, ts, "   removed %d voxels (%d points), %d left, step %.6g" % (out[6], out[7], len(out[0]), out[4].step))
        stages(p, c, a.bits, a.repeats)
        sys.stdout.flush()


if __name__ == "__main__":
    main()
