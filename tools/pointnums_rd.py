"""Rate / whole-cloud D1 of the six in-repo checkpoints on the synthetic cloud for three decoder inputs: the true counts at
rho = 1, the true counts at eval's searched rho_d1 (select_optimal_rho over RHOS_D1), and `--pointnums d1` at rho = 1.
D1 is pc_error's "mseF,PSNR (p2point)" (metrics.pc_error on the deduplicated reconstruction, as eval.py measures it).

    python tools/pointnums_rd.py [--out FILE]

--metric d2: the same three columns for `--pointnums d2` and D2, pc_error's "mseF,PSNR (p2plane)" (metrics.d2_metrics) with the
normals of metrics.estimate_normals(points, 10, 20): the true counts at rho = 1, `d2` at rho = 1, the true counts at eval's
searched rho_d2 (select_optimal_rho over RHOS_D2); D1 of each alongside."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ALPHAS = ("0.75", "2.00", "3.50", "6.00", "10.00", "16.00")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--metric", choices=("d1", "d2"), default="d1")
    a = ap.parse_args()
    if a.metric == "d2":
        return main_d2(a)
    from pcgcv1_amd import eval as rd, metrics, synthetic
    from pcgcv1_amd.models import model_voxception as model
    from pcgcv1_amd.process import postprocess_points
    pts = synthetic.make_cloud(1300)
    res = 1023
    lines = ["checkpoint      bpp(count)  bpp(d1)   D1@rho=1   rho_d1  D1@rho_d1  D1 d1@rho=1   d1-rho1  d1-rho_d1"]
    for al in ALPHAS:
        ckpt = os.path.join(ROOT, "checkpoints", "hyper", "a%sb3.00" % al)

        def d1(cubes_d, nums, pos, rho):
            rec = postprocess_points(cubes_d, nums, pos, 1.0, 64, rho)
            rec = np.unique(np.rint(rec).astype(np.int32), axis=0)
            return metrics.pc_error(pts, rec, None, res)["mseF,PSNR (p2point)"]
        cubes_d, pos, nums, n, bpps = rd.rate_point(pts, model, ckpt, 1.0, 64, 64)
        cache = {}

        def measure(rho):
            if rho not in cache:
                cache[rho] = {"mseF,PSNR (p2point)": d1(cubes_d, nums, pos, rho)}
            return cache[rho]
        rho_d1 = rd.select_optimal_rho("mseF,PSNR (p2point)", rd.RHOS_D1, measure)
        p1, pr = measure(1.0)["mseF,PSNR (p2point)"], measure(rho_d1)["mseF,PSNR (p2point)"]
        cubes_e, pos_e, nums_e, _, bpps_e = rd.rate_point(pts, model, ckpt, 1.0, 64, 64, pointnums="d1")
        pd = d1(cubes_e, nums_e, pos_e, 1.0)
        lines.append("a%-8sb3.00  %9.5f  %9.5f  %9.4f  %6.2f  %9.4f  %11.4f  %+8.4f  %+8.4f" % (
            al, bpps[0], bpps_e[0], p1, rho_d1, pr, pd, pd - p1, pd - pr))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def main_d2(a):
    from pcgcv1_amd import eval as rd, metrics, synthetic
    from pcgcv1_amd.models import model_voxception as model
    from pcgcv1_amd.process import postprocess_points
    pts = synthetic.make_cloud(1300)
    normals = metrics.estimate_normals(pts, 10, 20)
    res = 1023
    d1k, d2k = "mseF,PSNR (p2point)", "mseF,PSNR (p2plane)"
    lines = ["checkpoint      bpp(count)  bpp(d2)   D2@rho=1   rho_d2  D2@rho_d2  D2 d2@rho=1   d2-rho1  d2-rho_d2 |  D1@rho=1  D1@rho_d2  D1 d2@rho=1"]
    for al in ALPHAS:
        ckpt = os.path.join(ROOT, "checkpoints", "hyper", "a%sb3.00" % al)

        def both(cubes_d, nums, pos, rho):
            rec = postprocess_points(cubes_d, nums, pos, 1.0, 64, rho)
            rec = np.unique(np.rint(rec).astype(np.int32), axis=0)
            return metrics.pc_error(pts, rec, normals, res)
        cubes_d, pos, nums, n, bpps = rd.rate_point(pts, model, ckpt, 1.0, 64, 64)
        cache = {}

        def measure(rho):
            if rho not in cache:
                cache[rho] = both(cubes_d, nums, pos, rho)
            return cache[rho]
        rho_d2 = rd.select_optimal_rho(d2k, rd.RHOS_D2, measure)
        m1, mr = measure(1.0), measure(rho_d2)
        cubes_e, pos_e, nums_e, _, bpps_e = rd.rate_point(pts, model, ckpt, 1.0, 64, 64, pointnums="d2", normals=normals)
        me = both(cubes_e, nums_e, pos_e, 1.0)
        lines.append("a%-8sb3.00  %9.5f  %9.5f  %9.4f  %6.2f  %9.4f  %11.4f  %+8.4f  %+8.4f | %9.4f  %9.4f  %11.4f" % (
            al, bpps[0], bpps_e[0], m1[d2k], rho_d2, mr[d2k], me[d2k], me[d2k] - m1[d2k], me[d2k] - mr[d2k], m1[d1k], mr[d1k], me[d1k]))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
