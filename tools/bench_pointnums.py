"""Time the encoder-side point-count search (csrc/pointnums.hip) on the synthetic cloud's 205 cubes under the a6 checkpoint:
the curves (pointnums.distortion_curves), the sweep + ladder (pointnums.sweep_curves) and the whole
optimize_points_numbers, host clock after a synchronise, after warm-up, median and min of --reps runs; then the same for the
point-to-plane curves (--pointnums d2: voxel_normals, distortion_curves_d2, optimize_points_numbers(metric="d2")) with the
normals of metrics.estimate_normals(points, 10, 20), in the same run.

    python tools/bench_pointnums.py [--reps 10] [--warmup 2] [--out FILE]

Run under `rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/bench_pointnums.py` for per-kernel times."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ckpt", default=os.path.join(ROOT, "checkpoints", "hyper", "a6.00b3.00"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from pcgcv1_amd import metrics, pointnums as pn, synthetic
    from pcgcv1_amd.models import model_voxception as model
    from pcgcv1_amd.process import preprocess_points
    from pcgcv1_amd.transform import compress_hyper
    pts = synthetic.make_cloud(1300)
    cubes, pos, nums = preprocess_points(pts, 1.0, 64, 64)
    logits = compress_hyper(cubes, model, a.ckpt, decompress=True)[8]
    torch.cuda.synchronize()

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(1e3 * (time.perf_counter() - t0))
        return {"median_ms": round(float(np.median(ts)), 3), "min_ms": round(float(np.min(ts)), 3), "reps": a.reps}

    m, A, B, off = pn.distortion_curves(cubes, logits, nums)
    lad = pn.ladder_counts(nums, np.diff(off), pn.RHOS_D1)
    res = {"cubes": int(len(nums)), "points": int(nums.astype(np.int64).sum()), "K_total": int(off[-1]),
           "K_mean": round(float(np.diff(off).mean()), 1)}
    p = pn._Prepared(cubes, logits, nums)
    res["segment_total"] = int(p.n_seg.sum())
    res["chunks"] = len(p.chunks)
    # distance evaluations of the brute-force forms: B = sum M_b N_b, A = sum N_b M_b, rank = sum M_b^2
    res["distance_evals"] = int(2 * (p.n_seg * p.n_pts).sum())
    res["rank_compares"] = int((p.n_seg ** 2).sum())
    res["curves"] = timed(lambda: pn.distortion_curves(cubes, logits, nums))
    res["sweep_J64_plus_ladder"] = timed(lambda: pn.sweep_curves(m, A, B, off, 64, lad))
    res["optimize_points_numbers"] = timed(lambda: pn.optimize_points_numbers(cubes, logits, nums))
    counts, rep = pn.optimize_points_numbers(cubes, logits, nums)
    res["choice"] = list(rep["choice"])
    res["local_psnr_count_db"] = round(rep["psnr_count"], 4)
    res["local_psnr_chosen_db"] = round(rep["psnr_chosen"], 4)
    normals = metrics.estimate_normals(pts, 10, 20)
    vn = pn.voxel_normals(pts, normals, pos, 1.0, 64)
    torch.cuda.synchronize()
    d2 = {"voxel_normals": timed(lambda: pn.voxel_normals(pts, normals, pos, 1.0, 64)),
          "curves": timed(lambda: pn.distortion_curves_d2(cubes, logits, nums, vn)),
          "optimize_points_numbers": timed(lambda: pn.optimize_points_numbers(cubes, logits, nums, metric="d2", normals=vn)),
          # the same two searches as d1; a dot product and a square per ranked voxel, and per change of an occupied voxel's nearest
          "distance_evals": res["distance_evals"], "plane_terms_B": int(p.n_seg.sum())}
    counts2, rep2 = pn.optimize_points_numbers(cubes, logits, nums, metric="d2", normals=vn)
    d2["choice"] = list(rep2["choice"])
    d2["local_psnr_count_db"] = round(rep2["psnr_count"], 4)
    d2["local_psnr_chosen_db"] = round(rep2["psnr_chosen"], 4)
    d2["counts_sum"] = int(counts2.astype(np.int64).sum())
    res["d2"] = d2
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
