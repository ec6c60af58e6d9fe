"""What the colour metric of the registration costs (pcgcv1_amd/register.py, metric="color"; csrc/color_icp.hip:
pcgc_color_gradient; csrc/offgrid.hip: pcgc_register_color_step): the 1 M-point pair of tools/register_bench.py with a texture
of three sinusoids painted on it.

    python tools/color_icp_bench.py [--repeats 7] > profiles/color_icp_bench.txt
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/color_icp_bench.py --profile     # kernel times: tools/rocpd_stats.py

Medians (and ranges) of `repeats` calls after two warm calls, a host clock around the call and a device synchronise:
pcgc_color_gradient on the target sorted by cell, one pcgc_register_color_step and one pcgc_register_step on the same inputs at
gates 4 and 1 with the source sorted by cell (the sums read back, as the loop reads them), and the whole icp in both metrics."""
import argparse
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from pcgcv1_amd import _lib, ingest, register                            # noqa: E402
from register_bench import line, make_scan, timed                        # noqa: E402

WAVES = ((np.array([0.9, 0.3, 0.2]), 19.0, 0.4), (np.array([-0.2, 0.8, 0.5]), 31.0, 1.7), (np.array([0.4, -0.5, 0.7]), 70.0, 2.9))
MIX = np.array([[0.5, 0.3, 0.2], [0.2, 0.5, 0.3], [0.3, 0.2, 0.5]])


def texture(x):
    """uint8 colours [n,3] at the places x (voxels): per channel a mix of three sinusoids of period 19, 31 and 70 voxels"""
    s = np.stack([np.sin(2.0 * np.pi * (x @ (k / np.linalg.norm(k))) / period + phase) for k, period, phase in WAVES], 1)
    return np.clip(np.rint((0.5 + 0.45 * s @ MIX.T) * 255.0), 0, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--bits", type=int, default=10)
    ap.add_argument("--profile", action="store_true", help="one gradient call and three steps of each kind, nothing else: for a kernel trace")
    a = ap.parse_args()
    _lib.require_gpu()
    (tp, tn), (sp, _) = make_scan(a.points, 1), make_scan(a.points, 2)
    frame = ingest.fit_frame(tp, bits=a.bits)
    target, src = register.to_grid(tp, frame), register.to_grid(sp, frame)
    ct, cs = texture(target.astype(np.float64)), texture(src.astype(np.float64))
    centre = np.rint((target.astype(np.float64).min(0) + target.astype(np.float64).max(0)) / 2.0)
    R0 = register.rodrigues(np.array([1.0, 2.0, 3.0]) / math.sqrt(14.0) * math.radians(1.0))
    source = (src.astype(np.float64) @ R0.T + (centre - R0 @ centre) + np.array([0.6, -0.6, 0.5])).astype(np.float32)
    eye, zero = np.eye(3), np.zeros(3)
    cm = register.ColorMatcher(source, target, tn, cs, ct)
    pm = register.Matcher(source, target, tn)
    cm.sort_source(eye, zero)
    pm.sort_source(eye, zero)
    # the gradient call as ColorMatcher makes it: the target sorted by the cells of the gradient's own radius
    dev = cm.source_d.device
    t64 = target.astype(np.float64)
    cells = register.cells_from_bounds(t64.min(0), t64.max(0), register.DEFAULT_COLOR_RADIUS, "icp")
    t_d = torch.from_numpy(target).to(dev)
    order = register.cell_order(t_d, cells)
    g_d = t_d[order].contiguous()
    n_d = torch.from_numpy(register._unit_normals(tn, len(target))).to(dev)[order].contiguous()
    Y_d = torch.from_numpy(register.intensity(ct, len(target), "target")).to(dev)[order].contiguous()

    def gradient():
        return register.color_gradient_step(g_d, n_d, Y_d, cells, register.DEFAULT_COLOR_RADIUS, register.DEFAULT_COLOR_KMIN)

    if a.profile:
        gradient()
        for m in (cm, pm):
            for _ in range(3):
                m.step(eye, zero, centre, 4.0)
        torch.cuda.synchronize()
        return
    print("pair: 2 x %d points, %d bits (step %.6g m), matcher cells of edge %g, %d per axis; gradient cells of edge %g, %d per axis; "
          "%d repeats" % (a.points, a.bits, frame.step, cm.cells.h, cm.cells.res, cells[0], cells[4], a.repeats))
    (_, valid), ts = timed(gradient, a.repeats)
    line("pcgc_color_gradient, radius %g, kmin %d" % (register.DEFAULT_COLOR_RADIUS, register.DEFAULT_COLOR_KMIN), ts,
         "   %d of %d points have a gradient" % (int((valid != 0).sum().item()), len(target)))
    _, ts = timed(lambda: register.ColorMatcher(source, target, tn, cs, ct), max(3, a.repeats // 2), warmup=1)
    line("ColorMatcher(...): upload, sort, prepare, gradients", ts)
    medians = {}
    for gate in (4.0, 1.0):
        for name, m in (("colour", cm), ("plane", pm)):
            S, ts = timed(lambda: m.step(eye, zero, centre, gate), a.repeats)
            medians[(name, gate)] = statistics.median(ts)
            line("%s step, gate %g, source sorted by cell" % (name, gate), ts, "   n_used %d" % S[0])
        print("    colour step / plane step at gate %g: %.3f" % (gate, medians[("colour", gate)] / medians[("plane", gate)]))
    for metric in ("color", "plane"):
        kw = dict(source_colors=cs, target_colors=ct) if metric == "color" else {}
        r, ts = timed(lambda: register.icp(source, target, tn, metric=metric, **kw), max(3, a.repeats // 2), warmup=1)
        line("icp, %s, schedule (4, 2, 1)" % metric, ts, "   steps %s, converged %s, fitness %.3f, rmse %.4f" % (
            r["iterations"], r["converged"], r["fitness"], r["rmse"]))
        moved = source.astype(np.float64) @ r["R"].T + r["t"]
        print("    the pose puts the source %.4f voxel (largest) from where it was sampled" % float(np.linalg.norm(moved - src, axis=1).max()))


if __name__ == "__main__":
    main()
