"""Time recolouring and the colour distortion (csrc/color.hip) on the synthetic bench cloud's 205 cubes against its
reconstruction under the a6 checkpoint, next to pcgc_d1_mse and the pcgc_d2_* calls on the same pair (the same shell search
and tie walk, csrc/voxel_grid.h; the source carries seeded normals).

    python tools/bench_recolor.py [--reps 50] [--warmup 5] [--out FILE]

Device events around each library call (the calls only enqueue kernels), after warm-up; median and min of --reps runs.
Needs an MI355X: there is no host path to time.  Run under `rocprofv3 --kernel-trace --stats -d DIR -o run -- python
tools/bench_recolor.py --reps 3 --warmup 1` for per-kernel times."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ckpt", default=os.path.join(ROOT, "checkpoints", "hyper", "a6.00b3.00"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from pcgcv1_amd import _lib, metrics, synthetic
    from pcgcv1_amd import recolor as rc
    from pcgcv1_amd.models import model_voxception as model
    from pcgcv1_amd.process import postprocess_points, preprocess_points
    from pcgcv1_amd.transform import compress_hyper
    dev = _lib.require_gpu()
    lib = _lib.hip()
    pts = synthetic.make_cloud(1300).astype(np.int32)
    col = np.random.default_rng(1300).integers(0, 256, (len(pts), 3)).astype(np.uint8)
    cubes, pos, nums = preprocess_points(pts, 1.0, 64, 64)
    logits = compress_hyper(cubes, model, a.ckpt, decompress=True)[8]
    rec = np.unique(np.rint(postprocess_points(logits, nums, pos, 1.0, 64, 1.0, None)).astype(np.int32), axis=0)
    res = int(max(pts.max(), rec.max())) + 1
    cells, _ = rc.target_cells(rec, res)
    tkeys = (cells[:, 0].astype(np.int64) * res + cells[:, 1]) * res + cells[:, 2]
    s_d, c_d = torch.from_numpy(pts).to(dev), torch.from_numpy(col).to(dev)
    t_d, k_d = torch.from_numpy(cells).to(dev), torch.from_numpy(tkeys).to(dev)
    tc_d = torch.empty((len(cells), 3), dtype=torch.uint8, device=dev)
    cnt_d = torch.empty(len(cells), dtype=torch.int32, device=dev)
    out = torch.empty(6, dtype=torch.float64, device=dev)
    ws = torch.empty(int(max(lib.pcgc_recolor_workspace_bytes(res, len(pts), len(cells)),
                             lib.pcgc_color_mse_workspace_bytes(res, max(len(pts), len(cells))),
                             lib.pcgc_d1_workspace_bytes(res), lib.pcgc_d2_workspace_bytes(res, max(len(pts), len(cells))))),
                     dtype=torch.uint8, device=dev)
    # D2 takes both clouds in key order
    (ks_d, order), (kt_d, order_t) = metrics._sorted_keys(s_d, res), metrics._sorted_keys(t_d, res)
    ss_d, ts_d = s_d[order].contiguous(), t_d[order_t].contiguous()
    ns_d = torch.from_numpy(np.random.default_rng(1301).normal(size=(len(pts), 3)).astype(np.float32)).to(dev)
    nt_d = torch.empty((len(cells), 3), dtype=torch.float32, device=dev)
    st = _lib.stream()

    def recolor():
        _lib.check(lib.pcgc_recolor(_lib.dptr(s_d), _lib.dptr(c_d), len(pts), _lib.dptr(k_d), len(cells), res, _lib.dptr(tc_d),
                                    _lib.dptr(cnt_d), _lib.dptr(ws), ws.numel(), st), "pcgc_recolor")

    def color_mse_ab():
        _lib.check(lib.pcgc_color_mse(_lib.dptr(s_d), _lib.dptr(c_d), len(pts), _lib.dptr(t_d), _lib.dptr(tc_d), len(cells), res,
                                      _lib.dptr(out), _lib.dptr(ws), ws.numel(), st), "pcgc_color_mse")

    def color_mse_ba():
        _lib.check(lib.pcgc_color_mse(_lib.dptr(t_d), _lib.dptr(tc_d), len(cells), _lib.dptr(s_d), _lib.dptr(c_d), len(pts), res,
                                      _lib.dptr(out[3:]), _lib.dptr(ws), ws.numel(), st), "pcgc_color_mse")

    def d1_ab():
        _lib.check(lib.pcgc_d1_mse(_lib.dptr(s_d), len(pts), _lib.dptr(t_d), len(cells), res, _lib.dptr(out), _lib.dptr(ws), ws.numel(), st),
                   "pcgc_d1_mse")

    def d1_ba():
        _lib.check(lib.pcgc_d1_mse(_lib.dptr(t_d), len(cells), _lib.dptr(s_d), len(pts), res, _lib.dptr(out), _lib.dptr(ws), ws.numel(), st),
                   "pcgc_d1_mse")

    def d2_transfer():
        _lib.check(lib.pcgc_d2_transfer_normals(_lib.dptr(ss_d), len(pts), _lib.dptr(ns_d), _lib.dptr(kt_d), len(cells), res,
                                                _lib.dptr(nt_d), _lib.dptr(ws), ws.numel(), st), "pcgc_d2_transfer_normals")

    def d2_ab():
        _lib.check(lib.pcgc_d2_mse(_lib.dptr(ss_d), len(pts), _lib.dptr(kt_d), len(cells), _lib.dptr(nt_d), res, _lib.dptr(out),
                                   _lib.dptr(ws), ws.numel(), st), "pcgc_d2_mse")

    def d2_ba():
        _lib.check(lib.pcgc_d2_mse(_lib.dptr(ts_d), len(cells), _lib.dptr(ks_d), len(pts), _lib.dptr(ns_d), res, _lib.dptr(out),
                                   _lib.dptr(ws), ws.numel(), st), "pcgc_d2_mse")

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return {"median_ms": round(float(np.median(ts)), 3), "min_ms": round(float(np.min(ts)), 3), "reps": a.reps}

    r = {"source_points": int(len(pts)), "target_points": int(len(cells)), "res": res,
         "workspace_MB": round(lib.pcgc_recolor_workspace_bytes(res, len(pts), len(cells)) / 2 ** 20, 1)}
    r["pcgc_d1_mse A->B"] = timed(d1_ab)
    r["pcgc_d1_mse B->A"] = timed(d1_ba)
    r["pcgc_d2_transfer_normals A->B"] = timed(d2_transfer)
    r["pcgc_d2_mse A->B"] = timed(d2_ab)
    r["pcgc_d2_mse B->A"] = timed(d2_ba)
    r["pcgc_recolor"] = timed(recolor)
    r["pcgc_color_mse A->B"] = timed(color_mse_ab)
    r["pcgc_color_mse B->A"] = timed(color_mse_ba)
    torch.cuda.synchronize()
    r["targets_without_backward_set"] = int((cnt_d == 0).sum())
    r["c_mse"] = [float(v) for v in out.cpu().numpy()]
    line = json.dumps(r)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
