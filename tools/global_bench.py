"""What the global alignment costs (pcgcv1_amd/register.py: global_align; csrc/global.hip: pcgc_feature_*, pcgc_ransac_score): two
independent 1 M-point samplings of the surface of tools/register_bench.py on a 10-bit grid, the source turned by 90 degrees
about a skew axis and shifted, keypoints at a feature_voxel that leaves about 20 000 of them per cloud, the other distances
in proportion (radius 8, corr_dist 2, min_edge 6 feature voxels).

    python tools/global_bench.py [--repeats 5] > profiles/global_bench.txt

Medians (and ranges) of `repeats` calls after one warm call, a host clock around the call and a device synchronise: the
keypoints, the two descriptor stages, the match, the host's draws with their batched solve, the scoring of the kept draws and of
100 000 poses, global_align as a whole, the pose error before and after icp, and the same stages from the rule in numpy
(tests/_global_ref.py, brute force) on the first keypoints, scaled by its own quadratic cost."""
import argparse
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from pcgcv1_amd import _lib, ingest, register                            # noqa: E402
from register_bench import make_scan                                     # noqa: E402


def timed(fn, repeats, warmup=1):
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


def line(name, ts, note=""):
    print("%-58s median %9.2f ms   (min %9.2f, max %9.2f)%s" % (name, 1e3 * statistics.median(ts), 1e3 * min(ts), 1e3 * max(ts), note))
    sys.stdout.flush()


def apart(R, t, moved, true):
    return float(np.linalg.norm(moved.astype(np.float64) @ np.asarray(R).T + np.asarray(t) - true, axis=1).max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--bits", type=int, default=10)
    ap.add_argument("--keypoints", type=int, default=20000)
    ap.add_argument("--reference_keypoints", type=int, default=6000, help="how many keypoints the numpy rule is timed on")
    a = ap.parse_args()
    _lib.require_gpu()
    (tp, tn), (sp, sn) = make_scan(a.points, 1), make_scan(a.points, 2)
    frame = ingest.fit_frame(tp, bits=a.bits)
    target, src = register.to_grid(tp, frame), register.to_grid(sp, frame)
    centre = np.rint((target.astype(np.float64).min(0) + target.astype(np.float64).max(0)) / 2.0)
    R0 = register.rodrigues(np.array([1.0, 2.0, 3.0]) / math.sqrt(14.0) * math.radians(90.0))
    source = (src.astype(np.float64) @ R0.T + (centre - R0 @ centre) + np.array([150.0, -80.0, 60.0])).astype(np.float32)
    source_normals = (sn @ R0.T).astype(np.float32)
    tn = tn.astype(np.float32)
    fv = 8.0
    for _ in range(3):                                          # the count goes with 1 / fv^2 on a surface
        n_kp = len(register.keypoints(target, tn, fv)[0])
        if abs(n_kp - a.keypoints) < 0.05 * a.keypoints:
            break
        fv = float(np.round(fv * math.sqrt(n_kp / float(a.keypoints)), 2))
    radius, corr, edge = 8.0 * fv, 2.0 * fv, 6.0 * fv
    print("pair: 2 x %d points, %d bits (step %.6g m), source turned by 90 degrees and shifted by (150, -80, 60) voxels; %d repeats"
          % (a.points, a.bits, frame.step, a.repeats))
    (kt, nt), ts = timed(lambda: register.keypoints(target, tn, fv), a.repeats)
    ks, ns = register.keypoints(source, source_normals, fv)
    print("feature_voxel %g: %d target and %d source keypoints; radius %g, corr_dist %g, min_edge %g; cells of edge %g"
          % (fv, len(kt), len(ks), radius, corr, edge, register.feature_cells(kt, radius)[0]))
    line("keypoints (1 M points: quantise, merge, read back)", ts)
    ct = register._FeatureCloud(kt, nt, radius)
    (S, k), ts = timed(ct.pairs, a.repeats)
    line("pcgc_feature_pairs", ts, "   %.0f neighbours per keypoint" % float(k.float().mean().item()))
    _, ts = timed(lambda: ct.combine(S, k), a.repeats)
    line("pcgc_feature_combine", ts)
    (ft, vt), ts = timed(lambda: register.features(kt, nt, radius), a.repeats)
    line("features(...): sort by cell, upload, both stages, read back", ts)
    fs, vs = register.features(ks, ns, radius)
    _, ts = timed(lambda: register.match_features(fs, vs, ft, vt), a.repeats)
    line("match_features (%d x %d rows, upload and read back)" % (len(fs), len(ft)), ts)
    P, Q, _, _ = register.correspondences(ks, fs, vs, kt, ft, vt)
    (poses, draw), ts = timed(lambda: register.draw_hypotheses(P, Q, edge, 100000, 0), a.repeats)
    line("host: 100 000 draws, edge checks, batched Kabsch", ts, "   %d kept" % len(poses))
    scorer = register.Scorer(P, Q, corr)
    if len(poses):
        _, ts = timed(lambda: scorer(poses), a.repeats)
        line("score of the kept draws (%d poses x %d pairs)" % (len(poses), len(P)), ts)
    many = np.tile(poses if len(poses) else np.concatenate([np.eye(3).reshape(9), np.zeros(3)])[None], (100000 // max(1, len(poses)) + 1, 1))[:100000]
    _, ts = timed(lambda: scorer(many), a.repeats)
    line("score of 100 000 poses x %d pairs" % len(P), ts)
    true = src.astype(np.float64)
    try:
        out, ts = timed(lambda: register.global_align(source, target, source_normals, tn, fv, radius, corr, edge), a.repeats)
        line("global_align as a whole", ts, "   %d inliers of %d, %d kept draws, winner draw %d" % (
            out["inliers"], out["correspondences"], out["hypotheses"], out["draw"]))
        before = apart(out["R"], out["t"], source, true)
        print("    the coarse pose puts the source %.3f voxel (largest) from where it was sampled" % before)
        gates = tuple(g for g in (32.0, 16.0, 8.0, 4.0, 2.0, 1.0) if g <= 2.0 * corr) or (4.0, 2.0, 1.0)
        r, ts = timed(lambda: register.icp(source, target, tn, "plane", gates, init=(out["R"], out["t"])), 1, warmup=0)
        line("icp from it, plane, schedule %s" % (gates,), ts, "   steps %s, converged %s, fitness %.3f" % (r["iterations"], r["converged"], r["fitness"]))
        print("    after icp: %.4f voxel (largest)" % apart(r["R"], r["t"], source, true))
    except ValueError as e:
        print("global_align failed: %s" % e)
    import _global_ref as ref
    n = min(a.reference_keypoints, len(kt), len(ks))
    t0 = time.perf_counter()
    rf = ref.features(kt[:n], nt[:n], radius)
    t1 = time.perf_counter()
    ref.match(fs[:n], vs[:n], ft[:n], vt[:n])
    t2 = time.perf_counter()
    scale = (len(kt) / float(n)) ** 2
    print("numpy rule on the first %d keypoints: features %.2f s, match %.2f s; by (N / n)^2 = %.1f for all %d: features %.1f s, match %.1f s"
          % (n, t1 - t0, t2 - t1, scale, len(kt), (t1 - t0) * scale, (t2 - t1) * scale))
    same = np.array_equal(rf[0], register.features(kt[:n], nt[:n], radius)[0])
    print("    its descriptors equal the device's on those keypoints: %s" % same)


if __name__ == "__main__":
    main()
