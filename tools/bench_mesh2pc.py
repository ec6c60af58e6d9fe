"""Timing of the mesh -> point cloud kernels (csrc/mesh.hip), hip events around the device work after warm-up.

    python tools/bench_mesh2pc.py [--reps 20]

  sample+voxelize: pcgc_mesh_sample + pcgc_mesh_voxelize of 400 000 points (resolution 255) from a torus of about 1 M
                   triangles (the host's area running sum is timed apart)
  normals:         pcgc_estimate_normals(radius 10, max_nn 20) on synthetic.make_cloud() (about 0.85 M points, res 1024);
                   for comparison the same neighbour rule's nearest cousin on the host: scipy cKDTree query(k=20,
                   distance_upper_bound=10) on 16 workers + covariance + np.linalg.eigh
Prints one JSON line per case."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np      # noqa: E402
import torch            # noqa: E402

from pcgcv1_amd import _lib, synthetic   # noqa: E402
from pcgcv1_amd.dataprocess import mesh2pc_open3d as m2p   # noqa: E402


def torus(nu, nv, R=3.0, r=1.0):
    u, w = np.meshgrid(np.arange(nu) * 2 * np.pi / nu, np.arange(nv) * 2 * np.pi / nv, indexing="ij")
    v = np.stack([(R + r * np.cos(w)) * np.cos(u), (R + r * np.cos(w)) * np.sin(u), r * np.sin(w)], -1).reshape(-1, 3)
    idx = np.arange(nu * nv).reshape(nu, nv)
    a, b = idx, np.roll(idx, -1, 0)
    c, d = np.roll(b, -1, 1), np.roll(a, -1, 1)
    t = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])
    return v, t.astype(np.int32)


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(np.min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu_workers", type=int, default=16)
    a = ap.parse_args()
    dev = _lib.require_gpu()
    lib = _lib.hip()
    s = _lib.stream

    # ---- sampling + voxelisation
    v, t = torus(1000, 500)
    t0 = time.perf_counter()
    cdf = m2p.triangle_area_cdf(v, t)
    cdf_ms = (time.perf_counter() - t0) * 1e3
    n, res = 400000, 255
    v_d, t_d, c_d = (torch.from_numpy(x).to(dev) for x in (v, t, cdf))
    rot = torch.from_numpy(m2p.get_rotate_matrix(1)).to(dev)
    pts = torch.empty((n, 3), dtype=torch.float64, device=dev)
    out = torch.empty((n, 3), dtype=torch.int32, device=dev)
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    ws = torch.empty(int(lib.pcgc_mesh_voxelize_workspace_bytes(res)), dtype=torch.uint8, device=dev)

    def sample():
        _lib.check(lib.pcgc_mesh_sample(_lib.dptr(v_d), len(v), _lib.dptr(t_d), len(t), _lib.dptr(c_d), n, 12345, _lib.dptr(rot),
                                        _lib.dptr(pts), s()), "pcgc_mesh_sample")

    def vox():
        _lib.check(lib.pcgc_mesh_voxelize(_lib.dptr(pts), n, res, _lib.dptr(out), n, _lib.dptr(cnt), _lib.dptr(ws), ws.numel(), s()),
                   "pcgc_mesh_voxelize")
    s_med, s_min = timed(sample, a.reps)
    v_med, v_min = timed(vox, a.reps)
    b_med, b_min = timed(lambda: (sample(), vox()), a.reps)
    print(json.dumps({"case": "sample+voxelize", "triangles": len(t), "n_points": n, "resolution": res,
                      "unique_points": int(cnt.item()), "area_cdf_host_ms": round(cdf_ms, 3),
                      "sample_ms": round(s_med, 4), "voxelize_ms": round(v_med, 4), "both_ms": round(b_med, 4),
                      "both_min_ms": round(b_min, 4)}))

    # ---- normals
    p = synthetic.make_cloud()
    N, res = len(p), 1024                                   # the grid make_cloud voxelised it on
    p_d = torch.from_numpy(p).to(dev)
    nrm = torch.empty((N, 3), dtype=torch.float32, device=dev)
    ws = torch.empty(int(lib.pcgc_normals_workspace_bytes(res, N, 10.0)), dtype=torch.uint8, device=dev)

    def normals():
        _lib.check(lib.pcgc_estimate_normals(_lib.dptr(p_d), N, res, 10.0, 20, _lib.dptr(nrm), None, None, _lib.dptr(ws), ws.numel(),
                                             s()), "pcgc_estimate_normals")
    n_med, n_min = timed(normals, a.reps)
    row = {"case": "estimate_normals", "points": N, "res": res, "radius": 10, "max_nn": 20, "gpu_ms": round(n_med, 4),
           "gpu_min_ms": round(n_min, 4)}
    try:
        from scipy.spatial import cKDTree
        t0 = time.perf_counter()
        pf = p.astype(np.float64)
        tree = cKDTree(pf)
        d, idx = tree.query(pf, k=20, distance_upper_bound=10.0 + 1e-9, workers=a.cpu_workers)
        ok = np.isfinite(d)
        nb = pf[np.where(ok, idx, 0)] * ok[..., None]
        k = ok.sum(1)[:, None]
        mean = nb.sum(1) / k
        cov = np.einsum("nki,nkj->nij", nb, nb) / k[..., None] - mean[:, :, None] * mean[:, None, :]
        np.linalg.eigh(cov)
        row["scipy_ckdtree_k20_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        row["scipy_workers"] = a.cpu_workers
    except ImportError:
        row["scipy_ckdtree_k20_ms"] = None
    print(json.dumps(row))


if __name__ == "__main__":
    main()
