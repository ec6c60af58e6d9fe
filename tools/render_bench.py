"""What drawing the bench cloud costs: render.render of synthetic.make_cloud() (828 225 points) at 1024 x 1024 with the
default view window and point size, end to end (host arrays in, image out), and its two kernels on their own.

    python tools/render_bench.py [--repeats 9] [--output profiles/render_bench.txt]

End to end: two warm-up calls, then the median and the range of `repeats` calls, a host clock around a call that ends in
the device-to-host copy of the image.  Kernels: the cloud already on the device, `--batch` launches between two device
events per sample (one launch is too short to time alone), two warm-up samples, then the median and the range of
`repeats` samples, per launch.  Next to the splat stands the traffic it cannot avoid, 12 B read per point and one 8-byte
atomic per point and covered pixel, and the time the measured copy rate of the chip (6.29 TB/s) would need for it."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pcgcv1_amd import _lib, render, synthetic                           # noqa: E402

COPY_RATE = 6.29e12               # B/s, float4 copy measured on an MI355X


def host_timed(fn, repeats, warmup=2):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return ts


def device_timed(fn, repeats, batch, warmup=2):
    ts = []
    for r in range(warmup + repeats):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(batch):
            fn()
        end.record()
        end.synchronize()
        if r >= warmup:
            ts.append(start.elapsed_time(end) * 1e-3 / batch)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--output", default=os.path.join(ROOT, "profiles", "render_bench.txt"))
    a = ap.parse_args()
    dev = _lib.require_gpu()
    side = a.size
    p = synthetic.make_cloud().astype(np.float32)
    colors = np.random.default_rng(1).integers(0, 256, (len(p), 3)).astype(np.uint8)
    R = render.view_matrix("front")
    window = render.fit_window(p, R, side, side)
    ps = render.default_point_size(window)
    lines = []

    def say(s):
        print(s)
        sys.stdout.flush()
        lines.append(s)
    say("cloud: synthetic.make_cloud(), %d points; %d x %d, front view, %.3f pixels per voxel, point_size %d, shade %d; %d repeats"
        % (len(p), side, side, window.scale / 4096.0, ps, render.DEFAULT_K, a.repeats))
    ts = host_timed(lambda: render.render(p, colors, size=(side, side)), a.repeats)
    say("%-44s median %9.3f ms   (min %9.3f, max %9.3f)" % ("render(), host arrays in, image out", 1e3 * statistics.median(ts), 1e3 * min(ts), 1e3 * max(ts)))
    p_d, c_d = torch.from_numpy(p).to(dev), torch.from_numpy(colors).to(dev)
    assert render.fit_window(p_d, R, side, side) == window
    ts = host_timed(lambda: render.fit_window(p_d, R, side, side), a.repeats)
    say("%-44s median %9.3f ms   (the extents of the projection, on the device: what render() does)" % ("  of which fit_window, device tensor", 1e3 * statistics.median(ts)))
    ts = host_timed(lambda: render.fit_window(p, R, side, side), a.repeats)
    say("%-44s median %9.3f ms   (the same from a host array: numpy projects every point)" % ("  fit_window, host array", 1e3 * statistics.median(ts)))
    zbuf = render.splat(p_d, R, window, side, side, ps)
    out = render.resolve(zbuf, side, side, c_d)
    covered = int((out[1] >= 0).sum())
    shown = int(torch.unique(out[1]).numel()) - 1
    pairs = len(p) * ps * ps                                    # the fitted window keeps every square inside the image
    nbytes = 12 * len(p) + 8 * pairs
    ts = device_timed(lambda: render.splat(p_d, R, window, side, side, ps, workspace=zbuf), a.repeats, a.batch)
    med = statistics.median(ts)
    say("%-44s median %9.3f ms   (min %9.3f, max %9.3f)   per launch, with the clearing of the z-buffer (%d x launches per sample)"
        % ("splat (pcgc_render_splat)", 1e3 * med, 1e3 * min(ts), 1e3 * max(ts), a.batch))
    say("  %d points x %d pixels = %d keys offered, %d pixels covered, %d points visible" % (len(p), ps * ps, pairs, covered, shown))
    say("  12 B per point + 8 B per key offered = %.1f MB: %.3f ms at the chip's copy rate of 6.29 TB/s; measured / that bound = %.1f"
        % (nbytes / 1e6, 1e3 * nbytes / COPY_RATE, med / (nbytes / COPY_RATE)))
    for other in (1, 3, 5, 7):                                  # how the time follows the keys offered, same points and window
        if other != ps:
            ts = device_timed(lambda: render.splat(p_d, R, window, side, side, other, workspace=zbuf), a.repeats, a.batch)
            say("  the same at point_size %d (%d keys offered): median %9.3f ms" % (other, len(p) * other * other, 1e3 * statistics.median(ts)))
    render.splat(p_d, R, window, side, side, ps, workspace=zbuf)
    ts = device_timed(lambda: render.resolve(zbuf, side, side, c_d, out=out), a.repeats, a.batch)
    say("%-44s median %9.3f ms   (min %9.3f, max %9.3f)   per launch, rgb + index + depth" % ("resolve (pcgc_render_resolve)", 1e3 * statistics.median(ts),
                                                                                              1e3 * min(ts), 1e3 * max(ts)))
    values = torch.rand(len(p), device=dev) * 5
    lut = torch.from_numpy(render.colormap_lut()).to(dev)
    col = torch.empty((len(p), 3), dtype=torch.uint8, device=dev)
    ts = device_timed(lambda: _lib.check(_lib.hip().pcgc_colormap(_lib.dptr(values), len(p), 64.0, _lib.dptr(lut), _lib.dptr(col), _lib.stream())),
                      a.repeats, a.batch)
    say("%-44s median %9.3f ms   (min %9.3f, max %9.3f)   per launch, %d values" % ("colormap (pcgc_colormap)", 1e3 * statistics.median(ts), 1e3 * min(ts),
                                                                                   1e3 * max(ts), len(p)))
    with open(a.output, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
