"""The colour codec's rule in numpy: YCoCg-R, the region-adaptive hierarchical transform (RAHT) over the Morton order of a
voxelised cloud, the uniform quantiser and the reconstruction.  This file is the definition; csrc/raht.hip
and pcgcv1_amd/colorcodec.py must give the same bits.

Row order of every per-coefficient array: row j belongs to leaf j, the j-th point in ascending Morton order.  Row 0 is the
DC (subband 3d, weight M); row j > 0 is the `hi` of the one merge in which the node that STARTS at leaf j is the right-hand
sibling (a node is named by its first leaf), its subband is that merge's level and its weight the merged weight w1 + w2.
"""
import numpy as np


def depth_of(points):
    """smallest d with 2^d > the largest coordinate"""
    return int(np.max(points)).bit_length()


def morton_keys(points, d):
    """3d bits, bit triple b from the top = x_b y_b z_b, x most significant"""
    p = np.asarray(points).astype(np.int64)
    key = np.zeros(len(p), np.int64)
    for b in range(d):
        key |= (((p[:, 0] >> b) & 1) << (3 * b + 2)) | (((p[:, 1] >> b) & 1) << (3 * b + 1)) | (((p[:, 2] >> b) & 1) << (3 * b))
    return key


def rgb_to_ycocg(rgb):
    c = np.asarray(rgb).astype(np.int32)
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    co = r - b
    t = b + (co >> 1)
    cg = g - t
    y = t + (cg >> 1)
    return np.stack([y, co, cg], -1)


def ycocg_to_rgb(ycc):
    c = np.asarray(ycc).astype(np.int32)
    y, co, cg = c[..., 0], c[..., 1], c[..., 2]
    t = y - (cg >> 1)
    g = cg + t
    b = t - (co >> 1)
    r = b + co
    return np.stack([r, g, b], -1)


def _walk(keys, nlev):
    """the merges of every level for ascending unique keys: per level (slot of node 1, slot of node 2, w1, w2); a node's slot
    is its first leaf"""
    key = keys.copy()
    start = np.arange(len(key), dtype=np.int64)
    w = np.ones(len(key), np.int64)
    merges = []
    for _ in range(nlev):
        parent = key >> 1
        first = np.flatnonzero(parent[1:] == parent[:-1])            # node 1 of each pair: low bit 0, the smaller key
        second = first + 1
        assert ((key[first] & 1) == 0).all() and ((key[second] & 1) == 1).all()
        merges.append((start[first], start[second], w[first].copy(), w[second].copy()))
        w[first] += w[second]
        keep = np.ones(len(key), bool)
        keep[second] = False
        key, start, w = parent[keep], start[keep], w[keep]
    assert len(key) == 1
    return merges


def forward(points, attrs, d=None):
    """points int [M,3] unique, attrs [M,3] -> (coef float64 [M,3], subband int32 [M], weight int64 [M]), rows in Morton order"""
    points = np.asarray(points)
    d = depth_of(points) if d is None else d
    keys = morton_keys(points, d)
    perm = np.argsort(keys, kind="stable")
    keys = keys[perm]
    assert len(keys) == 1 or (np.diff(keys) > 0).all(), "duplicate points"
    a = np.asarray(attrs)[perm].astype(np.float64)
    m = len(keys)
    subband = np.full(m, 3 * d, np.int32)
    weight = np.full(m, m, np.int64)
    for l, (s1, s2, w1, w2) in enumerate(_walk(keys, 3 * d)):
        r1, r2, rw = np.sqrt(w1.astype(np.float64))[:, None], np.sqrt(w2.astype(np.float64))[:, None], np.sqrt((w1 + w2).astype(np.float64))[:, None]
        a1, a2 = a[s1], a[s2]
        lo = (r1 * a1 + r2 * a2) / rw
        hi = (r1 * a2 - r2 * a1) / rw
        a[s1], a[s2] = lo, hi
        subband[s2] = l
        weight[s2] = w1 + w2
    return a, subband, weight


def inverse(points, coef, d=None):
    """coef [M,3] in Morton order (forward's rows) -> attributes float64 [M,3] in the order of `points`"""
    points = np.asarray(points)
    d = depth_of(points) if d is None else d
    keys = morton_keys(points, d)
    perm = np.argsort(keys, kind="stable")
    a = np.asarray(coef).astype(np.float64).copy()
    for s1, s2, w1, w2 in reversed(_walk(keys[perm], 3 * d)):
        r1, r2, rw = np.sqrt(w1.astype(np.float64))[:, None], np.sqrt(w2.astype(np.float64))[:, None], np.sqrt((w1 + w2).astype(np.float64))[:, None]
        lo, hi = a[s1], a[s2]
        a1 = (r1 * lo - r2 * hi) / rw
        a2 = (r2 * lo + r1 * hi) / rw
        a[s1], a[s2] = a1, a2
    out = np.empty_like(a)
    out[perm] = a
    return out


def quantize(coef, step):
    return np.rint(np.asarray(coef, np.float64) / np.float64(step)).astype(np.int32)


def dequantize(q, step):
    return q.astype(np.float64) * np.float64(step)


def colors_from_attrs(a):
    """step 6: rint, clip to the channel's range, inverse YCoCg-R, clip to [0, 255]"""
    ycc = np.rint(a)
    ycc = np.stack([np.clip(ycc[:, 0], 0, 255), np.clip(ycc[:, 1], -255, 255), np.clip(ycc[:, 2], -255, 255)], -1).astype(np.int32)
    return np.clip(ycocg_to_rgb(ycc), 0, 255).astype(np.uint8)


def codec(points, colors, step, d=None):
    """the whole lossy path -> (decoded uint8 [M,3] in the order of `points`, q int32 [M,3] Morton order, subband, the
    reconstructed YCoCg attributes before rounding, float64 [M,3] in the order of `points`)"""
    coef, subband, _ = forward(points, rgb_to_ycocg(colors), d)
    q = quantize(coef, step)
    a = inverse(points, dequantize(q, step), d)
    return colors_from_attrs(a), q, subband, a


def empirical_bits(q, subband):
    """sum over the subbands (level, channel) of n * H0(q): the zeroth-order entropy yardstick of the rate test"""
    bits = 0.0
    for l in np.unique(subband):
        for c in range(3):
            _, n = np.unique(q[subband == l, c], return_counts=True)
            p = n / n.sum()
            bits += float(-(n * np.log2(p)).sum())
    return bits


def subband_order(subband):
    """the leaves grouped by subband, ascending subband, ascending leaf within one: the order in which the file holds q"""
    return np.argsort(subband, kind="stable")
