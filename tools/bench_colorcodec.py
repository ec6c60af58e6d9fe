"""Time and measure the RAHT colour codec (csrc/raht.hip, pcgcv1_amd/colorcodec.py) on the decoded geometry of the synthetic
bench cloud (828 225 points, 205 cubes, a6 checkpoint) with a textured colour field, and measure the entropy layer against the
numpy reference's empirical entropy on the rate test's cloud.

    python tools/bench_colorcodec.py [--reps 20] [--warmup 3] [--out-dir profiles] [--coder range|rans|both] [--target]

Writes <out-dir>/colorcodec_bench.txt (encode / decode split into stages, median of --reps after warm-up, every stage ended by a
device synchronise; launches per direction with and without the fused tree top; tests/_raht_ref.py on the host as baseline) and
<out-dir>/colorcodec_rd.txt (bits per point, bits / H and c[i],PSNRF coded and recoloured-uncoded at the six steps).
--coder rans / both (stream version 2, the entropy coder on the GPU: csrc/rans.hip) writes <out-dir>/colorcodec_rans_bench.txt
(the same stages for the chosen coders, interleaved in one loop of one process, and the format constants' alternatives) and
<out-dir>/colorcodec_rans_rd.txt (bytes of both versions at the six steps on both clouds, version 2's overhead split into
states, chunk table and range-coded levels, bits / H on the test cloud) and leaves the two version 1 files alone.
--target (the rate control: csrc/color_rc.hip, colorcodec.encode_colors_target) writes <out-dir>/colorcodec_rc.txt alone: the time of
one sweep launch of 32 steps and of one PSNR probe, encode_colors_target in both modes against a plain encode_colors at the step it
chose (taking turns inside one loop of one process), and the size estimate against real files on both clouds.
Needs an MI355X: there is no host path to time."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STEPS = (1, 2, 4, 8, 16, 32)
STAGES = ("sort + structure", "transform", "quantise + symbols", "host coding")


def textured(points, res, sigma, seed):
    """a smooth colour field plus Gaussian noise (the rate test's field, at any resolution)"""
    t = points.astype(np.float64) / res
    col = np.stack([128 + 100 * np.sin(7 * t[:, 0] + 3 * t[:, 1]), 128 + 100 * np.cos(5 * t[:, 1] - 2 * t[:, 2]), 255 * t[:, 2]], -1)
    return np.clip(np.rint(col + np.random.default_rng(seed).normal(0, sigma, col.shape)), 0, 255).astype(np.uint8)


def overhead(cc, data, points):
    """(states, chunk table, range-coded levels, rANS words) bytes of a version 2 file"""
    import struct
    plan = cc.Plan(points)
    counts = [int(c) for c in plan.level_counts]
    _, _, _, kinds, streams, chunk_sizes, _, _ = cc.unpack_v2(data, plan.d, plan.m, counts)
    per = cc.RANS_LANES * cc.RANS_STEPS
    states = sum(4 * min(cc.RANS_LANES, 3 * counts[l] - per * i) for l in range(len(kinds)) for i in range(len(chunk_sizes[l])))
    table = 4 * sum(len(c) for c in chunk_sizes)
    rows = [struct.unpack("<HHHHHI", data[36 + 14 * l:50 + 14 * l]) for l in range(len(kinds))]
    ranged = sum(r[5] for r in rows if r[4] == cc.CODER_RANGE)
    return states, table, ranged, sum(len(x) for x in streams) - states


def rans_report(a, ref, cc, rc, synthetic, model, postprocess_points, preprocess_points, compress_hyper):
    coders = ("range", "rans") if a.coder == "both" else ("rans",)
    s0, t0_ = cc.RANS_STEPS, cc.RANS_MIN_SYMBOLS
    pts = synthetic.make_cloud(seed=5, res=128, n_shells=3, rmin=0.2, rmax=0.4).astype(np.int32)
    col = textured(pts, 128, 10, 5)
    src = synthetic.make_cloud(1300).astype(np.int32)
    src_col = textured(src, 1024, 10, 1300)
    cubes, pos, nums = preprocess_points(src, 1.0, 64, 64)
    logits = compress_hyper(cubes, model, a.ckpt, decompress=True)[8]
    rec = np.unique(np.rint(postprocess_points(logits, nums, pos, 1.0, 64, 1.0, None)).astype(np.int32), axis=0)
    rec_col = rc.recolor(src, src_col, rec)
    clouds = (("test cloud (tests/test_gpu_colorcodec.py::_coloured_cloud, %d points)" % len(pts), pts, col, True),
              ("bench cloud (synthetic.make_cloud(1300) decoded with the a6 checkpoint, %d points), textured colours (sigma 10)" % len(rec), rec, rec_col, False))
    rd = ["RAHT colour codec, stream version 2 (chunked 64-way interleaved rANS): bytes against version 1 (tools/bench_colorcodec.py --coder %s)" % a.coder,
          "format constants: S = RANS_STEPS = %d steps per chunk, T = RANS_MIN_SYMBOLS = %d symbols" % (s0, t0_), ""]
    for title, p, c, with_h in clouds:
        rd.append(title)
        rd.append("step  v1 bytes  v2 bytes  v2/v1   states  chunk table  range levels  rANS words" + ("  v1 bits/H  v2 bits/H" if with_h else ""))
        worst = 0.0
        for step in STEPS:
            v1 = cc.encode_colors(p, c, step)
            v2 = cc.encode_colors(p, c, step, coder="rans")
            assert np.array_equal(cc.decode_colors(p, v2), cc.decode_colors(p, v1))
            st, tb, rg, wd = overhead(cc, v2, p)
            line = "%4d  %8d  %8d  %6.4f  %6d  %11d  %12d  %10d" % (step, len(v1), len(v2), len(v2) / len(v1), st, tb, rg, wd)
            if with_h:
                _, q, sub, _ = ref.codec(p, c, step)
                h = ref.empirical_bits(q, sub)
                worst = max(worst, 8 * len(v2) / h)
                line += "  %9.4f  %9.4f" % (8 * len(v1) / h, 8 * len(v2) / h)
            rd.append(line)
        if with_h:
            rd.append("largest version 2 bits / H = %.4f  ->  the version 2 rate test's margin m2 = %.4f" % (worst, worst - 1 + 0.05))
        rd.append("")
    rd.append("alternatives: v2 / v1 bytes at steps 1, 4, 32 (test cloud | bench cloud)")
    for s_alt, t_alt in ((2048, 4096), (2048, 16384), (2048, 65536), (1024, 16384), (512, 16384), (256, 16384)):
        cc.RANS_STEPS, cc.RANS_MIN_SYMBOLS = s_alt, t_alt
        cells = []
        for _, p, c, _ in clouds:
            cells.append("  ".join("%.4f" % (len(cc.encode_colors(p, c, step, coder="rans")) / len(cc.encode_colors(p, c, step))) for step in (1, 4, 32)))
        rd.append("S %4d  T %5d:  %s" % (s_alt, t_alt, "  |  ".join(cells)))
    cc.RANS_STEPS, cc.RANS_MIN_SYMBOLS = s0, t0_
    with open(os.path.join(a.out_dir, "colorcodec_rans_rd.txt"), "w") as f:
        f.write("\n".join(rd) + "\n")
    print("\n".join(rd), flush=True)

    step = 4.0
    out = ["RAHT colour codec, both entropy coders: times on the decoded geometry of the bench cloud (%d points, d = %d), color_qstep %g" % (len(rec), cc.Plan(rec).d, step),
           "median of %d runs after %d warm-up runs, ms; every stage ends with a device synchronise; the coders take turns inside one loop of one process" % (a.reps, a.warmup),
           "(tools/bench_colorcodec.py --coder %s).  'host coding': the host range coder (range); the table work, the rANS kernels and the copies (rans)" % a.coder, ""]
    for s_alt in (s0,) + tuple(x for x in (512, 1024, 2048, 4096) if x != s0):
        cc.RANS_STEPS = s_alt
        runs = {(k, w): [] for k in coders for w in ("encode", "decode")}
        size = {}
        for i in range(a.warmup + a.reps):
            for k in coders:
                te, td = {}, {}
                t0 = time.perf_counter()
                data = cc.encode_colors(rec, rec_col, step, timings=te, coder=k)
                te["total"] = time.perf_counter() - t0
                t0 = time.perf_counter()
                cc.decode_colors(rec, data, timings=td)
                td["total"] = time.perf_counter() - t0
                size[k] = len(data)
                if i >= a.warmup:
                    runs[(k, "encode")].append(te)
                    runs[(k, "decode")].append(td)
        out.append("S = %d steps per chunk%s" % (s_alt, " (the format's)" if s_alt == s0 else " (alternative)"))
        med = {}
        for (k, w), r in runs.items():
            med[(k, w)] = {key: 1e3 * float(np.median([x[key] for x in r])) for key in STAGES + ("total",)}
        for w in ("encode", "decode"):
            for k in coders:
                out.append("  %-5s %s: %s | total %.3f | .colors %d bytes" % (k, w, "  ".join("%s %.3f" % (key, med[(k, w)][key]) for key in STAGES),
                                                                             med[(k, w)]["total"], size[k]))
            for k in coders:
                sub = sorted(key for key in runs[(k, w)][0] if key.startswith("sub: "))
                out.append("        %-5s %s, inside the stages above (each ended by its own synchronise): %s" % (
                    k, w, "; ".join("%s %.3f" % (key[5:], 1e3 * float(np.median([x[key] for x in runs[(k, w)]]))) for key in sub)))
            if len(coders) == 2:
                out.append("        %s: range / rans  host coding %.2fx  total %.2fx" % (w, med[("range", w)]["host coding"] / med[("rans", w)]["host coding"],
                                                                                       med[("range", w)]["total"] / med[("rans", w)]["total"]))
        out.append("")
    cc.RANS_STEPS = s0
    with open(os.path.join(a.out_dir, "colorcodec_rans_bench.txt"), "w") as f:
        f.write("\n".join(out) + "\n")
    print("\n".join(out))


def target_report(a, cc, rc, synthetic, model, postprocess_points, preprocess_points, compress_hyper):
    import torch
    from pcgcv1_amd import _lib
    pts = synthetic.make_cloud(seed=5, res=128, n_shells=3, rmin=0.2, rmax=0.4).astype(np.int32)
    col = textured(pts, 128, 10, 5)
    src = synthetic.make_cloud(1300).astype(np.int32)
    src_col = textured(src, 1024, 10, 1300)
    cubes, pos, nums = preprocess_points(src, 1.0, 64, 64)
    logits = compress_hyper(cubes, model, a.ckpt, decompress=True)[8]
    rec = np.unique(np.rint(postprocess_points(logits, nums, pos, 1.0, 64, 1.0, None)).astype(np.int32), axis=0)
    rec_col = rc.recolor(src, src_col, rec)
    clouds = (("test cloud (tests/test_gpu_colorcodec.py::_coloured_cloud, %d points)" % len(pts), pts, col),
              ("bench cloud (synthetic.make_cloud(1300) decoded with the a6 checkpoint, %d points), textured colours (sigma 10)" % len(rec), rec, rec_col))
    med = lambda x: 1e3 * float(np.median(x))                             # noqa: E731
    out = ["RAHT colour codec, rate control (tools/bench_colorcodec.py --target): times on the bench cloud's decoded geometry (%d points), ms," % len(rec),
           "median of %d runs after %d warm-up runs in one process" % (a.reps, a.warmup), ""]

    # ---- the kernels: one sweep launch of 32 steps (device events around the call), the sweep with its read-back, one probe
    search = cc._Search(rec, rec_col)
    lib, plan = _lib.hip(), search.plan
    steps = np.array([cc.grid_step(j) for j in range(cc.QSTEP_GRID_MIN, cc.QSTEP_GRID_MIN + 32)])
    sums = torch.empty((32, 37, 3), dtype=torch.int64, device=plan.dev)
    tops = torch.empty((32, 37), dtype=torch.int32, device=plan.dev)
    t_launch, t_sweep, t_grid, t_probe = [], [], [], []
    grid = [cc.grid_step(j) for j in range(cc.QSTEP_GRID_MIN, cc.QSTEP_GRID_MAX + 1)]
    for i in range(a.warmup + a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(lib.pcgc_raht_rate_sweep(_lib.dptr(search.coef), _lib.dptr(plan.order), _lib.dptr(plan.subband), plan.m, search.k_raw,
                                            _lib.nptr(steps), 32, _lib.dptr(sums), _lib.dptr(tops), _lib.stream()), "pcgc_raht_rate_sweep")
        e1.record()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        search.sweep(steps)
        t1 = time.perf_counter()
        search.sweep(grid)
        t2 = time.perf_counter()
        search.psnr_y(4.0)
        t3 = time.perf_counter()
        if i >= a.warmup:
            t_launch.append(e0.elapsed_time(e1) / 1e3)
            t_sweep.append(t1 - t0)
            t_grid.append(t2 - t1)
            t_probe.append(t3 - t2)
    out.append("pcgc_raht_rate_sweep, 32 steps, one launch with its two memsets (device events): %.3f" % med(t_launch))
    out.append("the same with the read-back of the sums (host clock): %.3f;  all 73 steps, three launches and the read-back: %.3f" % (med(t_sweep), med(t_grid)))
    out.append("one PSNR probe (requantise, inverse transform, store colours, six sums, 48 bytes back; host clock): %.3f" % med(t_probe))
    out.append("")

    # ---- the whole search against a plain encode at the step it chose, taking turns
    for coder in ("range", "rans"):
        for kw in ({"psnr": 38.0}, {"bpp": 0.6}):
            rep = cc.encode_colors_target(rec, rec_col, coder=coder, **kw)[1]
            t_target, t_plain, stages = [], [], []
            for i in range(a.warmup + a.reps):
                tm = {}
                t0 = time.perf_counter()
                cc.encode_colors_target(rec, rec_col, coder=coder, timings=tm, **kw)
                t1 = time.perf_counter()
                cc.encode_colors(rec, rec_col, rep["qstep"], coder=coder)
                t2 = time.perf_counter()
                if i >= a.warmup:
                    t_target.append(t1 - t0)
                    t_plain.append(t2 - t1)
                    stages.append(tm)
            name = "psnr:%g" % kw["psnr"] if "psnr" in kw else "bpp:%g" % kw["bpp"]
            out.append("%-5s %-8s encode_colors_target %.3f | plain encode_colors at its step %.3f | ratio %.2f | notch %d, step %.4f, luma PSNR %.4f dB, %d bytes, "
                       "%d probes, %d real encodes%s" % (coder, name, med(t_target), med(t_plain), med(t_target) / med(t_plain), rep["j"], rep["qstep"],
                                                          rep["psnr_y"], rep["bytes"], rep["probes"], rep["real_encodes"],
                                                          ", estimate %.0f bytes at notch %d" % (rep["est_bytes"], rep["j_est"]) if "j_est" in rep else ""))
            out.append("        inside (each stage ended by its own synchronise, so the parts add up to more than the untimed call): %s" % "; ".join(
                "%s %.3f" % (k, med([x[k] for x in stages])) for k in sorted(stages[0]) if k != "launches"))
    out.append("")

    # ---- the estimate against real files
    for title, p, c in clouds:
        out.append(title)
        search = cc._Search(p, c)
        counts = search.plan.level_counts
        fixed = (1.0, 4.0, 16.0, 64.0)
        sw = search.sweep(fixed)[0]
        for coder in ("range", "rans"):
            est = cc.estimate_bytes(counts, sw, coder)
            real = [len(cc.encode_colors(p, c, s, coder=coder)) for s in fixed]
            out.append("  %-5s est / real bytes at steps 1, 4, 16, 64: %s" % (coder, "  ".join("%.4f (%d / %d)" % (e / r, e, r) for e, r in zip(est, real))))
            cells = []
            for bpp in (0.25, 0.5, 1.0, 2.0):
                try:
                    rep = cc.encode_colors_target(p, c, bpp=bpp, coder=coder)[1]
                    cells.append("%g bpp: |%d - %d| = %d, %d real encodes" % (bpp, rep["j_est"], rep["j"], abs(rep["j_est"] - rep["j"]), rep["real_encodes"]))
                except ValueError as e:
                    cells.append("%g bpp: %s" % (bpp, e))
            out.append("        |j_est - j|: %s" % ";  ".join(cells))
        out.append("")
    with open(os.path.join(a.out_dir, "colorcodec_rc.txt"), "w") as f:
        f.write("\n".join(out) + "\n")
    print("\n".join(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ckpt", default=os.path.join(ROOT, "checkpoints", "hyper", "a6.00b3.00"))
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--coder", choices=("range", "rans", "both"), default="range",
                    help="entropy coder(s) of the colour stream to measure: range = version 1, rans = version 2, both = side by side")
    ap.add_argument("--target", action="store_true", help="measure the rate control (encode_colors_target) and write colorcodec_rc.txt alone")
    a = ap.parse_args()
    import _raht_ref as ref
    from pcgcv1_amd import _lib, metrics, synthetic
    from pcgcv1_amd import colorcodec as cc
    from pcgcv1_amd import recolor as rc
    from pcgcv1_amd.models import model_voxception as model
    from pcgcv1_amd.process import postprocess_points, preprocess_points
    from pcgcv1_amd.transform import compress_hyper
    _lib.require_gpu()
    os.makedirs(a.out_dir, exist_ok=True)
    if a.target:
        return target_report(a, cc, rc, synthetic, model, postprocess_points, preprocess_points, compress_hyper)
    if a.coder != "range":
        return rans_report(a, ref, cc, rc, synthetic, model, postprocess_points, preprocess_points, compress_hyper)

    # ---- the rate test's cloud: bits / H at the six steps
    rd = ["RAHT colour codec: rate and distortion (tools/bench_colorcodec.py)", ""]
    pts = synthetic.make_cloud(seed=5, res=128, n_shells=3, rmin=0.2, rmax=0.4).astype(np.int32)
    col = textured(pts, 128, 10, 5)
    rd.append("test cloud (tests/test_gpu_colorcodec.py::_coloured_cloud, %d points): H = sum over subbands of n H0(q) of the numpy reference" % len(pts))
    rd.append("step  bits/point  H/point  bits/H  header bytes")
    worst = 0.0
    for step in STEPS:
        _, q, sub, _ = ref.codec(pts, col, step)
        h = ref.empirical_bits(q, sub)
        data = cc.encode_colors(pts, col, step)
        assert np.array_equal(cc.decode_colors(pts, data), ref.codec(pts, col, step)[0])
        worst = max(worst, 8 * len(data) / h)
        rd.append("%4d  %10.4f  %7.4f  %6.4f  %d" % (step, 8 * len(data) / len(pts), h / len(pts), 8 * len(data) / h, cc.header_bytes(data)))
    rd.append("largest bits / H = %.4f  ->  the rate test's margin m = %.4f" % (worst, worst - 1 + 0.05))
    rd.append("")

    # ---- the bench cloud's decoded geometry
    src = synthetic.make_cloud(1300).astype(np.int32)
    src_col = textured(src, 1024, 10, 1300)
    cubes, pos, nums = preprocess_points(src, 1.0, 64, 64)
    logits = compress_hyper(cubes, model, a.ckpt, decompress=True)[8]
    rec = np.unique(np.rint(postprocess_points(logits, nums, pos, 1.0, 64, 1.0, None)).astype(np.int32), axis=0)
    rec_col = rc.recolor(src, src_col, rec)
    uncoded = metrics.color_metrics(src, src_col, rec, rec_col)
    rd.append("bench cloud (synthetic.make_cloud(1300), %d points; decoded geometry %d points, a6 checkpoint), textured colours (sigma 10)" % (len(src), len(rec)))
    rd.append("recoloured, uncoded: c[0],PSNRF %.4f  c[1],PSNRF %.4f  c[2],PSNRF %.4f" % tuple(uncoded["c[%d],PSNRF" % i] for i in range(3)))
    rd.append("step  bytes  bits/input point  coded c[0],PSNRF  c[1],PSNRF  c[2],PSNRF")
    for step in STEPS:
        data = cc.encode_colors(rec, rec_col, step)
        m = metrics.color_metrics(src, src_col, rec, cc.decode_colors(rec, data))
        rd.append("%4d  %8d  %8.4f  %8.4f  %8.4f  %8.4f" % (step, len(data), 8 * len(data) / len(src), m["c[0],PSNRF"], m["c[1],PSNRF"], m["c[2],PSNRF"]))
    with open(os.path.join(a.out_dir, "colorcodec_rd.txt"), "w") as f:
        f.write("\n".join(rd) + "\n")
    print("\n".join(rd))

    # ---- times
    step = 4.0
    out = ["RAHT colour codec: times on the decoded geometry of the bench cloud (%d points, d = %d), color_qstep %g" % (len(rec), cc.Plan(rec).d, step),
           "median of %d runs after %d warm-up runs, ms; every stage ends with a device synchronise (tools/bench_colorcodec.py)" % (a.reps, a.warmup), ""]
    for fuse in (True, False):
        enc, dec = [], []
        data = None
        for i in range(a.warmup + a.reps):
            te, td = {}, {}
            t0 = time.perf_counter()
            data = cc.encode_colors(rec, rec_col, step, fuse_top=fuse, timings=te)
            te["total"] = time.perf_counter() - t0
            t0 = time.perf_counter()
            cc.decode_colors(rec, data, fuse_top=fuse, timings=td)
            td["total"] = time.perf_counter() - t0
            if i >= a.warmup:
                enc.append(te)
                dec.append(td)
        out.append("fused tree top: %s   (.colors %d bytes)" % ("yes" if fuse else "no", len(data)))
        for name, runs in (("encode", enc), ("decode", dec)):
            med = {k: 1e3 * float(np.median([r[k] for r in runs])) for k in STAGES + ("total",)}
            out.append("  %s: %s | total %.3f | transform launches %d" % (name, "  ".join("%s %.3f" % (k, med[k]) for k in STAGES), med["total"],
                                                                         runs[0]["launches"]))
    t0 = time.perf_counter()
    want = ref.codec(rec, rec_col, step)[0]
    t_ref = time.perf_counter() - t0
    assert np.array_equal(cc.decode_colors(rec, cc.encode_colors(rec, rec_col, step)), want)
    out.append("")
    out.append("baseline: tests/_raht_ref.py (numpy, host) forward + quantise + inverse + reconstruct on the same input: %.1f ms; same colours bit for bit" % (1e3 * t_ref))
    with open(os.path.join(a.out_dir, "colorcodec_bench.txt"), "w") as f:
        f.write("\n".join(out) + "\n")
    print("\n".join(out))


if __name__ == "__main__":
    main()
