"""Brute-force numpy statements of the recolouring rule and of pc_error's colour distortion ("Colours").

Both build the full N x M matrix of squared distances, so they are for clouds of a few thousand points: the device
kernels (csrc/color.hip) are compared against them bit for bit (recolor) or to float64 rounding (color_metrics), and
color_metrics itself is pinned to the pc_error binary's printed values in tests/golden/pc_error_color.npz.
"""
import numpy as np

COLOR_KEYS = ["c[%d],    %s" % (i, d) for d in "12F" for i in range(3)] + ["c[%d],PSNR%s" % (i, d) for d in "12F" for i in range(3)]


def _tied(a, b):
    """bool [len(a), len(b)]: b[j] is one of the nearest points of b to a[i] (every point at the minimal squared distance)"""
    a = np.asarray(a, np.int64)
    b = np.asarray(b, np.int64)
    d = sum((a[:, None, k] - b[None, :, k]) ** 2 for k in range(3))
    return d == d.min(1, keepdims=True)


def _rounded_mean(tie, colors):
    """per row of `tie`: (2 * sum + n) // (2 * n) per channel over the columns that are set: the mean rounded half up"""
    n = tie.sum(1).astype(np.int64)
    s = tie.astype(np.int64) @ np.asarray(colors, np.int64)
    return (2 * s + n[:, None]) // (2 * n[:, None])


def recolor(source_points, source_colors, target_points):
    """-> (colours uint8 [N_T, 3], |B(t)| int32 [N_T]).  B(t) = the source points that have t among their nearest target
    points; colour(t) = rounded mean over B(t), or over t's own nearest source points where B(t) is empty."""
    back = _tied(source_points, target_points).T               # [N_T, N_S]
    count = back.sum(1)
    fwd = _tied(target_points, source_points)
    use = np.where((count > 0)[:, None], back, fwd)
    return _rounded_mean(use, source_colors).astype(np.uint8), count.astype(np.int32)


def recolor_off_grid(source_points, source_colors, target_points, resolution):
    """Targets off the integer grid are searched at np.rint of their coordinates clipped to [0, resolution); targets that
    land in one cell share its colour."""
    cells = np.clip(np.rint(np.asarray(target_points, np.float64)), 0, resolution - 1).astype(np.int64)
    uniq, inv = np.unique(cells, axis=0, return_inverse=True)
    return recolor(source_points, source_colors, uniq)[0][inv.reshape(-1)]


def yuv_bt709(rgb):
    c = np.asarray(rgb, np.float64) / 255.0
    r, g, b = c[:, 0], c[:, 1], c[:, 2]
    return np.stack([0.2126 * r + 0.7152 * g + 0.0722 * b,
                     -0.1146 * r - 0.3854 * g + 0.5 * b + 0.5,
                     0.5 * r - 0.4542 * g - 0.0458 * b + 0.5], -1)


def color_mse(points_a, colors_a, points_b, colors_b):
    """one direction: per channel, mean over A of (yuv(a) - yuv(rounded mean colour of a's nearest points of B))^2"""
    near = _rounded_mean(_tied(points_a, points_b), colors_b)
    return ((yuv_bt709(colors_a) - yuv_bt709(near)) ** 2).mean(0)


def color_metrics(points_a, colors_a, points_b, colors_b):
    m1 = color_mse(points_a, colors_a, points_b, colors_b)
    m2 = color_mse(points_b, colors_b, points_a, colors_a)
    out = {}
    for d, m in (("1", m1), ("2", m2), ("F", np.maximum(m1, m2))):
        for i in range(3):
            out["c[%d],    %s" % (i, d)] = float(m[i])
            out["c[%d],PSNR%s" % (i, d)] = float("inf") if m[i] == 0 else float(-10.0 * np.log10(m[i]))
    return out
