"""Training / test data from meshes, with the reference's interface (dataprocess/mesh2pc_open3d.py): every .off / .obj
under --input_rootdir is sampled uniformly by area (n_points), rotated at random, voxelised to a resolution^3 grid,
deduplicated, given normals and written as `<idx>_<name>.ply` with `x y z nx ny nz`.

Open3D is not part of this image; its three steps are restated here with explicit rules (include/pcgc.h):
  sample_points_uniformly -> pcgc_mesh_sample (device; seeded splitmix64 draws, Open3D's barycentric formula)
  voxelisation + np.unique -> pcgc_mesh_voxelize (device; the reference's min / max / np.round arithmetic)
  estimate_normals(KDTreeSearchParamHybrid(10, 20)) -> pcgc_estimate_normals (device; metrics.estimate_normals)
The mesh text is parsed by libpcgc_host.so (pcgc_parse_mesh), the area weights summed there in order (pcgc_mesh_area_cdf).
Bit parity with Open3D's sampler, neighbour order or eigenvector sign is not possible without Open3D; the output is
deterministic for a given --seed.

    python -m pcgcv1_amd.dataprocess.mesh2pc_open3d --input_rootdir ModelNet40/ --output_rootdir testdata/ModelNet40/ --seed 0
"""
import os
import random

import numpy as np

from .. import _lib
from . import inout_points as iop


def traverse_path_recursively(rootdir):
    """mesh2pc_open3d.py:10-23: every file below rootdir (sorted here, so that a seed picks the same files everywhere)."""
    out = []
    for d, dirs, files in os.walk(rootdir):
        dirs.sort()
        out += [os.path.join(d, f) for f in sorted(files)]
    return out


def read_triangle_mesh(filename):
    """.off / .obj -> (vertices float64 [V,3], triangles int32 [T,3]); polygons fan-triangulated (pcgc_parse_mesh)."""
    ext = os.path.splitext(filename)[1].lower()
    if ext not in (".off", ".obj"):
        raise ValueError("%s: only .off and .obj meshes are read" % filename)
    with open(filename, "rb") as f:
        text = np.frombuffer(f.read(), np.uint8)
    return parse_mesh(text, 0 if ext == ".off" else 1)


def parse_mesh(text, fmt):
    """mesh text (bytes / str / uint8 array) in format 0 = OFF, 1 = OBJ -> (vertices, triangles)."""
    if isinstance(text, str):
        text = text.encode()
    if isinstance(text, (bytes, bytearray)):
        text = np.frombuffer(bytes(text), np.uint8)
    host = _lib.host()
    nv, nt = np.zeros(1, np.int64), np.zeros(1, np.int64)
    cap = int(np.count_nonzero(text == 10)) + 2             # one vertex / triangle per line covers triangle meshes
    v, t = np.empty((cap, 3), np.float64), np.empty((cap, 3), np.int32)
    args = (_lib.nptr(text) if text.size else None, text.size, fmt)
    rc = host.pcgc_parse_mesh(*args, _lib.nptr(v), cap, _lib.nptr(t), cap, _lib.nptr(nv), _lib.nptr(nt))
    if rc == -2:                                             # polygons: more triangles than lines
        v, t = np.empty((int(nv[0]), 3), np.float64), np.empty((int(nt[0]), 3), np.int32)
        rc = host.pcgc_parse_mesh(*args, _lib.nptr(v), len(v), _lib.nptr(t), len(t), _lib.nptr(nv), _lib.nptr(nt))
    if rc in (-3, -4):
        raise ValueError(host.pcgc_host_last_error().decode())
    _lib.check_host(rc, "pcgc_parse_mesh")
    return v[:int(nv[0])].copy(), t[:int(nt[0])].copy()


def triangle_area_cdf(vertices, triangles):
    """Inclusive running sum of the triangle areas, float64, in order (np.cumsum of 0.5 |e x f|)."""
    v = np.ascontiguousarray(vertices, np.float64)
    t = np.ascontiguousarray(triangles, np.int32)
    cdf = np.empty(len(t), np.float64)
    rc = _lib.host().pcgc_mesh_area_cdf(_lib.nptr(v), len(v), _lib.nptr(t), len(t), _lib.nptr(cdf))
    if rc == -3:
        raise ValueError(_lib.host().pcgc_host_last_error().decode())
    _lib.check_host(rc, "pcgc_mesh_area_cdf")
    return cdf


def get_rotate_matrix(rng=None):
    """mesh2pc_open3d.py:49-54 from a seeded generator: the +-1 flip of m[0,0], then m @ Q of QR(randn(3,3)).
    rng: a numpy Generator, or a seed for np.random.default_rng."""
    if not isinstance(rng, np.random.Generator):
        rng = np.random.default_rng(rng)
    m = np.eye(3, dtype="float32")
    m[0, 0] *= rng.integers(0, 2) * 2 - 1
    return np.dot(m, np.linalg.qr(rng.standard_normal((3, 3)))[0])


def sample_points_uniformly(vertices, triangles, n_points, seed, rotation=None, cdf=None, device=False):
    """n_points area-weighted samples of the mesh (pcgc_mesh_sample), optionally times `rotation` as row vectors.
    -> float64 [n_points,3] numpy, or the device tensor with device=True."""
    import torch
    dev = _lib.require_gpu()
    if cdf is None:
        cdf = triangle_area_cdf(vertices, triangles)
    v_d = torch.from_numpy(np.ascontiguousarray(vertices, np.float64)).to(dev)
    t_d = torch.from_numpy(np.ascontiguousarray(triangles, np.int32)).to(dev)
    c_d = torch.from_numpy(np.ascontiguousarray(cdf, np.float64)).to(dev)
    r_d = None if rotation is None else torch.from_numpy(np.ascontiguousarray(rotation, np.float64).reshape(3, 3)).to(dev)
    out = torch.empty((int(n_points), 3), dtype=torch.float64, device=dev)
    _lib.check(_lib.hip().pcgc_mesh_sample(_lib.dptr(v_d), v_d.shape[0], _lib.dptr(t_d), t_d.shape[0], _lib.dptr(c_d), int(n_points),
                                           int(seed) & 0xFFFFFFFFFFFFFFFF, _lib.dptr(r_d), _lib.dptr(out), _lib.stream()),
               "pcgc_mesh_sample")
    return out if device else out.cpu().numpy()


def voxelize(points, resolution, device=False):
    """mesh2pc_open3d.py:67-73: shift by the smallest coordinate, scale the largest to `resolution`, np.round, np.unique
    (pcgc_mesh_voxelize).  points: float64 [n,3] numpy or device tensor -> int32 [N,3] in lexicographic order."""
    import torch
    dev = _lib.require_gpu()
    lib = _lib.hip()
    p_d = points if torch.is_tensor(points) else torch.from_numpy(np.ascontiguousarray(points, np.float64))
    p_d = p_d.to(device=dev, dtype=torch.float64).reshape(-1, 3).contiguous()
    n = int(p_d.shape[0])
    if n == 0:
        raise ValueError("voxelize: no points")
    ws = torch.empty(int(lib.pcgc_mesh_voxelize_workspace_bytes(int(resolution))), dtype=torch.uint8, device=dev)
    out = torch.empty((n, 3), dtype=torch.int32, device=dev)
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    _lib.check(lib.pcgc_mesh_voxelize(_lib.dptr(p_d), n, int(resolution), _lib.dptr(out), n, _lib.dptr(cnt), _lib.dptr(ws),
                                      ws.numel(), _lib.stream()), "pcgc_mesh_voxelize")
    out = out[:int(cnt.item())]
    return out if device else out.cpu().numpy()


def mesh2pc(mesh_filedir, pc_filedir, n_points=400000, resolution=255, seed=None, rotate=True):
    """mesh2pc_open3d.py:55-85 -> (points int32 [N,3], normals float32 [N,3]), also written to pc_filedir.
    seed: one np.random.default_rng seed for the sampler's stream and the rotation (None: fresh entropy)."""
    from .. import metrics
    rng = np.random.default_rng(seed)
    sample_seed = int(rng.integers(0, 2 ** 63))
    m = get_rotate_matrix(rng) if rotate else None
    v, t = read_triangle_mesh(mesh_filedir)
    p = sample_points_uniformly(v, t, int(n_points), sample_seed, m, device=True)
    pts_d = voxelize(p, resolution, device=True)
    normals = metrics.estimate_normals(pts_d, radius=10, max_nn=20)
    points = pts_d.cpu().numpy()
    if pc_filedir:
        iop.write_ply_normals(pc_filedir, points, normals)
    return points, normals


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)       # mesh2pc_open3d.py:88-98
    ap.add_argument("--input_rootdir", type=str, default="ModelNet40", dest="input_rootdir")
    ap.add_argument("--output_rootdir", type=str, default="testdata/ModelNet40/", dest="output_rootdir")
    ap.add_argument("--n_testdata", type=int, default=32, dest="n_testdata")
    ap.add_argument("--n_points", type=int, default=400000, dest="n_points")
    ap.add_argument("--resolution", type=int, default=255, dest="resolution")
    ap.add_argument("--seed", type=int, default=None, dest="seed", help="file choice, sampling and rotations (None: random)")
    ap.add_argument("--rotate", type=int, choices=(0, 1), default=1, dest="rotate")
    a = ap.parse_args(argv)
    files = [f for f in traverse_path_recursively(a.input_rootdir) if os.path.splitext(f)[1] in (".off", ".obj")]
    rnd = random.Random(a.seed)
    files = rnd.sample(files, min(a.n_testdata, len(files)))
    os.makedirs(a.output_rootdir, exist_ok=True)
    for idx, mesh_filedir in enumerate(files):
        name = os.path.basename(mesh_filedir).split(".")[0]
        pc_filedir = os.path.join(a.output_rootdir, "%d_%s.ply" % (idx, name))
        seed = None if a.seed is None else a.seed * 1000003 + idx
        points, _ = mesh2pc(mesh_filedir, pc_filedir, a.n_points, a.resolution, seed, bool(a.rotate))
        print(pc_filedir, len(points))


if __name__ == "__main__":
    main()
