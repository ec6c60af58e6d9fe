"""The component rule (include/pcgc.h, pcgc_clean_components; pcgcv1_amd/clean.py) in numpy, by brute force: all
pairs at Chebyshev distance <= G, scipy's connected components of that graph, label = the smallest key, the sizes and the two
filters' masks.  O(n^2): for a few thousand voxels.  Also the snake, a component whose diameter is its size.  Not collected by
pytest."""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

import _clean_ref as clean_ref

DEFAULT_GAP = 1


def keys(points, bits):
    p = np.asarray(points, np.int64).reshape(-1, 3)
    res = np.int64(1) << bits
    return (p[:, 0] * res + p[:, 1]) * res + p[:, 2]


def components(points, bits, gap=DEFAULT_GAP, rows=256):
    """points int [n,3], distinct, inside the grid -> (label int64 [n], size int32 [n], n_components int)"""
    p = np.asarray(points, np.int64).reshape(-1, 3)
    n = len(p)
    src, dst = [], []
    for a in range(0, n, rows):
        d = np.abs(p[a:a + rows, None, :] - p[None, :, :]).max(-1)
        i, j = np.nonzero(d <= gap)
        src.append(i + a)
        dst.append(j)
    src, dst = np.concatenate(src), np.concatenate(dst)
    graph = coo_matrix((np.ones(len(src), np.int8), (src, dst)), shape=(n, n))
    n_components, comp = connected_components(graph, directed=False)
    smallest = np.full(n_components, np.iinfo(np.int64).max)
    np.minimum.at(smallest, comp, keys(p, bits))
    return smallest[comp], np.bincount(comp)[comp].astype(np.int32), int(n_components)


def parse_spec(text):
    f = text.split(":")
    if f[0] == "component":
        return ("component", int(f[1]), int(f[2]) if len(f) > 2 else DEFAULT_GAP)
    if f[0] == "largest":
        return ("largest", int(f[1]) if len(f) > 1 else DEFAULT_GAP)
    return clean_ref.parse_spec(text)


def keep_mask(points, bits, spec):
    kind = parse_spec(spec)
    if kind[0] == "component":
        return components(points, bits, kind[2])[1] >= kind[1]
    if kind[0] == "largest":
        label, size, _ = components(points, bits, kind[1])
        return label == label[size == size.max()].min()
    return clean_ref.keep_mask(points, spec)


def keep_mask_all(points, bits, specs):
    """the filters in order, each on what the one before kept -> bool [n]"""
    points = np.asarray(points)
    alive = np.arange(len(points))
    for spec in specs:
        alive = alive[keep_mask(points[alive], bits, spec)]
    mask = np.zeros(len(points), bool)
    mask[alive] = True
    return mask


def voxelize_scan_clean(points, colors=None, normals=None, bits=None, voxel_size=None, clean=()):
    """_clean_ref.voxelize_scan_clean with the component filters among the specs: the same refit around this module's masks.
    A label orders as the voxels do on any grid that holds them, so the bits of the largest coordinate serve."""
    saved = clean_ref.keep_mask_all
    clean_ref.keep_mask_all = lambda vox, specs: keep_mask_all(vox, max(1, int(np.max(vox)).bit_length()), specs)
    try:
        return clean_ref.voxelize_scan_clean(points, colors, normals, bits, voxel_size, clean)
    finally:
        clean_ref.keep_mask_all = saved


def snake(bits):
    """one path through the grid, consecutive cells one step apart: full x-rows at every even y of every even z-plane in
    alternating direction, joined by one cell at the odd y (z) in between -> int32 [n,3] in walk order"""
    res, cells = 1 << bits, []
    for zi, z in enumerate(range(0, res, 2)):
        layer = []
        for yi, y in enumerate(range(0, res, 2)):
            xs = list(range(res)) if yi % 2 == 0 else list(range(res - 1, -1, -1))
            layer += [(x, y, z) for x in xs]
            if y + 2 < res:
                layer.append((xs[-1], y + 1, z))
        if zi % 2:
            layer = layer[::-1]
        cells += layer
        if z + 2 < res:
            cells.append(layer[-1][:2] + (z + 1,))
    return np.array(cells, np.int32)


def surface():
    """the surface fixture of tests/test_gpu_clean.py, by the same recipe: bits = 6, 3159 voxels of a sparsely sampled sphere that
    the grid's faces cut, a filled 5^3 block, 30 scattered voxels and four corners"""
    rng = np.random.default_rng(21)
    d = rng.normal(size=(6000, 3))
    p = np.rint((30, 36, 28) + 33.0 * d / np.linalg.norm(d, axis=1, keepdims=True))
    p = np.clip(p, 0, 63)
    p = np.unique(p, axis=0)
    p = p[rng.permutation(len(p))[:3000]]
    block = np.stack(np.meshgrid(*[np.arange(30, 35)] * 3, indexing="ij"), -1).reshape(-1, 3)
    p = np.unique(np.r_[p, block, rng.integers(0, 64, (30, 3)), [[0, 0, 0], [63, 63, 63], [0, 63, 31], [32, 0, 63]]], axis=0).astype(np.int32)
    return p[rng.permutation(len(p))]
