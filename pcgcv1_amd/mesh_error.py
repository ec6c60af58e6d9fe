"""How far a cloud lies from a triangle mesh, on the GPU (metrics.mesh_error; csrc/meshdist.hip): the exact
distance from every point to the nearest triangle, its rms and its maximum.

    python -m pcgcv1_amd.mesh_error --cloud X.ply --mesh X.obj [--max_dist D] [--samples N --seed S] [--frame X.frame]
                                    [--render X.png --vmax 2 --size W H]

The cloud is in voxel units.  The mesh is any .obj or .off the project reads, in voxel units as `surface` writes it without a
frame; with --frame it is taken to be in the scan's units (as `surface --frame` writes it) and brought back to voxel units first,
and the figures are printed in both.  --samples adds the opposite direction, samples of the mesh against the cloud.  --render
draws the cloud coloured by its distance to the mesh, --vmax voxels and beyond, and the far points of --max_dist, in red.
"""
import argparse
import os

import numpy as np


def unapply_frame(points, frame):
    """the inverse of ingest.apply_frame: the scan's units -> grid coordinates, float64 [N,3], as sub then div"""
    x = np.asarray(points, np.float64).reshape(-1, 3)
    return (x - frame.origin) / np.float64(frame.step)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="measure a voxelised cloud (.ply) against a triangle mesh (.obj / .off) on the GPU",
                                 formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    ap.add_argument("--cloud", required=True, help="the cloud (.ply), in voxel units")
    ap.add_argument("--mesh", required=True, help="the mesh (.obj or .off)")
    ap.add_argument("--max_dist", type=float, default=None, metavar="D", help="points farther than D voxels from the mesh are counted as far and enter no mean")
    ap.add_argument("--samples", type=int, default=0, metavar="N", help="also measure N area-weighted samples of the mesh against the cloud")
    ap.add_argument("--seed", type=int, default=0, help="the seed of --samples")
    ap.add_argument("--frame", default="", metavar="X.frame", help="the mesh is in the scan's units of this frame (pcgcv1_amd/ingest.py)")
    ap.add_argument("--render", default="", metavar="X.png", help="write the cloud coloured by its distance to the mesh")
    ap.add_argument("--vmax", type=float, default=2.0, help="--render: the distance in voxels that is drawn red")
    ap.add_argument("--size", type=int, nargs=2, default=(1024, 1024), metavar=("W", "H"), help="--render: pixels")
    args = ap.parse_args(argv)
    try:                                                                  # before any file is read
        from .metrics import check_max_dist
        check_max_dist(args.max_dist)
        if args.samples < 0:
            raise ValueError("mesh_error: --samples %d is not a count" % args.samples)
        if os.path.splitext(args.mesh)[1].lower() not in (".obj", ".off"):
            raise ValueError("%s: a mesh is read from .obj or .off" % args.mesh)
        if args.render and os.path.splitext(args.render)[1].lower() != ".png":
            raise ValueError("%s: --render writes a .png" % args.render)
        if not (np.isfinite(args.vmax) and args.vmax > 0):
            raise ValueError("mesh_error: --vmax %r must be finite and positive" % (args.vmax,))
        if min(args.size) < 1:
            raise ValueError("mesh_error: --size %d %d must be positive" % tuple(args.size))
    except ValueError as e:
        ap.error(str(e))
    return args


def figure_lines(figures, step=None):
    """the printed figures, one per line; step: the frame's, for a second distance in the scan's units"""
    def both(voxels):
        return "%.6g voxels" % voxels + ("" if step is None else " = %.6g in scan units" % (voxels * step))
    near = figures["points"] - figures["far"]
    lines = ["points: %d, of them far: %d" % (figures["points"], figures["far"]),
             "cloud to mesh: rms %s, max %s over %d points" % (both(figures["rms (p2mesh)"]), both(float(np.sqrt(figures["h. (p2mesh)"]))), near),
             "mse (p2mesh): %.9g, h. (p2mesh): %.9g (squared voxels)" % (figures["mse (p2mesh)"], figures["h. (p2mesh)"])]
    if "mse (mesh2p)" in figures:
        lines += ["mesh to cloud: rms %s, max %s" % (both(float(np.sqrt(figures["mse (mesh2p)"]))), both(float(np.sqrt(figures["h. (mesh2p)"])))),
                  "mse (mesh2p): %.9g, h. (mesh2p): %.9g, h. (sym): %.9g (squared voxels)" % (
                      figures["mse (mesh2p)"], figures["h. (mesh2p)"], figures["h. (sym)"])]
    lines.append("search: cell edge %d, %d pairs" % (figures["edge"], figures["pairs"]))
    return lines


def main(argv=None):
    args = parse_args(argv)
    from . import metrics
    from .dataprocess.inout_points import load_ply_colors
    from .dataprocess.mesh2pc_open3d import read_triangle_mesh
    frame = None
    if args.frame:
        from .ingest import read_frame
        frame = read_frame(args.frame)
    points, _ = load_ply_colors(args.cloud, as_float=True)
    vertices, triangles = read_triangle_mesh(args.mesh)
    if frame is not None:
        vertices = unapply_frame(vertices, frame)
    try:
        figures, (best, _) = metrics.mesh_error(points, vertices, triangles, args.max_dist, args.samples, args.seed, per_point=True)
    except ValueError as e:
        raise SystemExit(str(e))
    print("\n".join(figure_lines(figures, None if frame is None else frame.step)))
    if args.render:
        from . import render
        distance = np.where(np.isfinite(best), np.sqrt(np.where(np.isfinite(best), best, 0.0)), args.vmax)      # far: the top of the map
        image = render.render(points, render.error_colors(distance, args.vmax), size=tuple(args.size))
        render.write_png(args.render, image)
        print("{}: {} x {} png of {} points".format(args.render, image.shape[1], image.shape[0], len(points)))


if __name__ == "__main__":
    main()
