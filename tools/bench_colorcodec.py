"""Time and measure the RAHT colour codec (csrc/raht.hip, pcgcv1_amd/colorcodec.py) on the decoded geometry of the synthetic
bench cloud (828 225 points, 205 cubes, a6 checkpoint) with a textured colour field, and measure the entropy layer against the
numpy reference's empirical entropy on the rate test's cloud.

    python tools/bench_colorcodec.py [--reps 20] [--warmup 3] [--out-dir profiles]

Writes <out-dir>/colorcodec_bench.txt (encode / decode split into stages, median of --reps after warm-up, every stage ended by a
device synchronise; launches per direction with and without the fused tree top; tests/_raht_ref.py on the host as baseline) and
<out-dir>/colorcodec_rd.txt (bits per point, bits / H and c[i],PSNRF coded and recoloured-uncoded at the six steps).
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ckpt", default=os.path.join(ROOT, "checkpoints", "hyper", "a6.00b3.00"))
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
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
