"""Recolouring: carry the colours of the original cloud onto decoded geometry.

    python -m pcgcv1_amd.recolor --source ORIGINAL.ply --target X_rec.ply --output X_rec_color.ply

The geometry files hold no colours.  This is the encoder-side / evaluation step that follows the geometry codec — the
original's colours are transferred onto the reconstruction, which the attribute coder (colorcodec.py, `test.py compress
--colors raht`) then compresses and `metrics.color_metrics` can measure.  The rule (DESIGN.md "Colours"; include/pcgc.h, pcgc_recolor), in integers:

    N_T(s) = all target points at the minimal distance from the source point s (ties kept);  B(t) = { s : t in N_T(s) }
    colour(t) = (2 sum_{B(t)} c_s + |B(t)|) // (2 |B(t)|) per channel, the mean rounded half up,
                over N_S(t), t's own nearest source points, where no source point chose t.

Both searches run on the GPU (csrc/color.hip); there is no host path.
"""
import numpy as np

from . import _lib


def target_cells(target_points, resolution):
    """-> (cells int32 [M,3] unique in key order, index of every target point's cell): a target is searched at np.rint of its
    coordinates clipped to [0, resolution), so points off the integer grid (a rate point with scale != 1) that fall into
    one cell share one colour"""
    t = np.asarray(target_points)
    t = t.reshape(-1, t.shape[-1])[:, :3]
    cells = np.clip(np.rint(t.astype(np.float64)), 0, resolution - 1).astype(np.int64)
    keys = (cells[:, 0] * resolution + cells[:, 1]) * resolution + cells[:, 2]
    ukeys, inv = np.unique(keys, return_inverse=True)
    ucells = np.stack([ukeys // (resolution * resolution), (ukeys // resolution) % resolution, ukeys % resolution], -1)
    return ucells.astype(np.int32), inv.reshape(-1)


def recolor(source_points, source_colors, target_points, resolution=None, return_counts=False):
    """source_points int [N_S,3] (unique voxels >= 0), source_colors uint8 [N_S,3], target_points [N_T,3] -> uint8 [N_T,3] in
    the order of target_points.  resolution: edge of the grid (default: the largest coordinate of either cloud + 1).
    return_counts=True also returns |B(t)| per target point (int32; 0 = coloured from its own nearest source points)."""
    import torch
    from .metrics import GRID_MAX_RES, check_grid_range
    src = np.ascontiguousarray(np.asarray(source_points)[:, :3], np.int32)
    col = np.asarray(source_colors)
    tgt = np.asarray(target_points)
    if col.shape != (len(src), 3) or col.dtype != np.uint8:
        raise ValueError("recolor: source_colors must be uint8 [%d, 3] (got %s %s)" % (len(src), col.dtype, col.shape))
    if len(src) == 0:
        raise ValueError("recolor: the source cloud is empty")
    if len(tgt) == 0:
        return (np.zeros((0, 3), np.uint8), np.zeros(0, np.int32)) if return_counts else np.zeros((0, 3), np.uint8)
    if resolution is None:
        resolution = int(max(int(src.max()), int(np.rint(np.max(tgt))))) + 1
    res = int(resolution)
    # the grid's limit by name first (a target beyond it shows in the default resolution), then the caller's own resolution
    check_grid_range("recolor", src, [0, res - 1])
    if int(src.max()) >= res:
        raise ValueError("recolor: source coordinates must lie within [0, resolution = %d), resolution <= %d" % (res, GRID_MAX_RES))
    skeys = (src[:, 0].astype(np.int64) * res + src[:, 1]) * res + src[:, 2]
    if len(np.unique(skeys)) != len(skeys):
        raise ValueError("recolor: the source cloud holds duplicate points (pass unique voxels)")
    cells, inv = target_cells(tgt, res)
    tkeys = (cells[:, 0].astype(np.int64) * res + cells[:, 1]) * res + cells[:, 2]           # ascending: np.unique's order
    dev = _lib.require_gpu()
    lib = _lib.hip()
    s_d = torch.from_numpy(src).to(dev)
    c_d = torch.from_numpy(np.ascontiguousarray(col)).to(dev)
    k_d = torch.from_numpy(tkeys).to(dev)
    out = torch.empty((len(tkeys), 3), dtype=torch.uint8, device=dev)
    cnt = torch.empty(len(tkeys), dtype=torch.int32, device=dev)
    ws = torch.empty(int(lib.pcgc_recolor_workspace_bytes(res, len(src), len(tkeys))), dtype=torch.uint8, device=dev)
    _lib.check(lib.pcgc_recolor(_lib.dptr(s_d), _lib.dptr(c_d), len(src), _lib.dptr(k_d), len(tkeys), res, _lib.dptr(out),
                                _lib.dptr(cnt), _lib.dptr(ws), ws.numel(), _lib.stream()), "pcgc_recolor")
    colors = out.cpu().numpy()[inv]
    return (colors, cnt.cpu().numpy()[inv]) if return_counts else colors


def recolored_metrics(points, colors, rec):
    """The colour figures of a reconstruction recoloured from the original: `rec` is reduced to its grid cells (recolor's
    rint-and-share rule), those are recoloured from (points, colors) and measured with metrics.color_metrics."""
    from . import metrics
    res = int(max(int(np.max(points)), int(np.rint(np.max(rec))))) + 1
    cells, _ = target_cells(rec, res)
    return metrics.color_metrics(points, colors, cells, recolor(points, colors, cells, res))


def load_source(filename):
    """(points, colors) of a coloured ply; a file without colour properties is an error that names it"""
    from .dataprocess.inout_points import load_ply_colors
    points, colors = load_ply_colors(filename)
    if colors is None:
        raise SystemExit("%s has no colour properties (red green blue): nothing to transfer" % filename)
    return points, colors


def _load_target(filename):
    """positions as written (a scale != 1 reconstruction holds float text): float64 when any is fractional, else int64"""
    from .dataprocess.inout_points import load_ply_colors
    pts = load_ply_colors(filename, as_float=True)[0]
    return pts if (pts != np.rint(pts)).any() else pts.astype(np.int64)


def main(argv=None):
    import argparse
    from .dataprocess.inout_points import write_ply_colors
    ap = argparse.ArgumentParser(description="Transfer the colours of the original cloud onto decoded geometry (an encoder-side / "
                                             "evaluation tool: the codec's bitstream holds no colours).")
    ap.add_argument("--source", required=True, help="the original, coloured ply (integer voxels, red green blue)")
    ap.add_argument("--target", required=True, help="the decoded geometry (X_rec.ply)")
    ap.add_argument("--output", required=True, help="coloured ply to write: the target's positions with the transferred colours")
    ap.add_argument("--resolution", type=int, default=None, help="edge of the voxel grid (default: largest coordinate + 1)")
    a = ap.parse_args(argv)
    points, colors = load_source(a.source)
    target = _load_target(a.target)
    out, counts = recolor(points, colors, target, a.resolution, return_counts=True)
    write_ply_colors(a.output, target, out)
    print("recoloured %d points from %d (%d from their own nearest source points) -> %s" % (
        len(target), len(points), int((counts == 0).sum()), a.output))


if __name__ == "__main__":
    main()
