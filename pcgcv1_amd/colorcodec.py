"""Colour codec for decoded geometry: RAHT + uniform quantiser + static range coding -> <name>.colors.

    data = encode_colors(points, colors, qstep)          # points int [M,3] unique voxels, colors uint8 [M,3]
    colors = decode_colors(points, data)                 # uint8 [M,3] in the order of `points`

The rule (tests/_raht_ref.py is its definition in numpy): YCoCg-R, the region-adaptive hierarchical transform
over the Morton order of the voxels, q = rint(coef / qstep), range coding of q per subband (level, channel) with a two-sided
geometric table that is rebuilt from 16 bits in integer arithmetic.  The transform, the quantiser and the symbols run on the
GPU (csrc/raht.hip); the range coder is the host's (coder_ops).  There is no host path for the transform.

The file, little endian:

    0   4  magic "PCRA"                        16  8  color_qstep, float64
    4   1  version (1)                         24  4  crc32c of bytes 36 .. end
    5   1  d (coordinates < 2^d)               28  4  E, the number of escaped values
    6   2  L, the number of coded levels       32  4  crc32c of the geometry's leaves per subband (3d + 1 int64, little endian)
    8   8  M, the number of points             36  12 L  per coded level: amax u16, ratio[Y, Co, Cg] u16 (Q16), stream bytes u32
    then the L range-coder streams (level l: its leaves in Morton order x 3 channels, one table per channel), the E escapes
    (position delta as a varint, value as a zigzag varint, positions k * 3 + c ascending) and the raw tail: q of every leaf of
    the levels >= L and of the DC, zigzag varints.  L follows from the geometry: the lowest level above which (itself
    included) at most RAW_LEAVES leaves remain, where tables would cost more than they save.
"""
import struct

import numpy as np

from . import _lib

MAGIC = b"PCRA"
VERSION = 1
HEADER_BYTES = 36
LEVEL_BYTES = 12
RAW_LEAVES = 48            # the top of the tree, at most this many leaves (DC included), is stored raw
AMAX_CAP = 2047            # largest |q| with a symbol of its own; larger values take the escape symbol
MAX_COORD = 4095           # 12-bit clouds, as recolor


# ---------------------------------------------------------------------------------------------------------------- colour space
def rgb_to_ycocg(rgb):
    """uint8 [..., 3] -> int32 [..., 3] (Y in [0,255], Co and Cg in [-255,255]); reversible (YCoCg-R)"""
    c = np.asarray(rgb).astype(np.int32)
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    co = r - b
    t = b + (co >> 1)
    cg = g - t
    return np.stack([t + (cg >> 1), co, cg], -1)


def ycocg_to_rgb(ycc):
    """the inverse of rgb_to_ycocg, int32 [..., 3] (no clipping)"""
    c = np.asarray(ycc).astype(np.int32)
    y, co, cg = c[..., 0], c[..., 1], c[..., 2]
    t = y - (cg >> 1)
    b = t - (co >> 1)
    return np.stack([b + co, cg + t, b], -1)


# ---------------------------------------------------------------------------------------------------------------- tables
def build_tables(amax, ratios):
    """Quantised CDFs int32 [len(ratios), 2 amax + 3] of the two-sided geometric pmf over q in [-amax, amax] plus the escape
    symbol 2 amax + 1, each from one Q16 ratio r (weight of |q| = k: 2^30 (r / 2^16)^k by repeated multiply-and-shift; the
    escape gets both tails).  Integers only, so every machine builds the same table; every symbol is at least 1 / 2^16 wide."""
    amax = int(amax)
    r = np.asarray(ratios, np.int64).reshape(-1)
    if not (0 <= amax <= AMAX_CAP) or (r < 1).any() or (r > 65535).any():
        raise ValueError("colour tables: amax %d or a ratio outside [1, 65535]" % amax)
    t = np.empty((len(r), amax + 1), np.int64)
    t[:, 0] = 1 << 30
    for k in range(1, amax + 1):
        t[:, k] = (t[:, k - 1] * r) >> 16
    esc = (2 * t[:, amax] * r) // (65536 - r)
    w = np.concatenate([t[:, :0:-1], t, esc[:, None]], 1)                 # q = -amax .. amax, escape
    n = w.shape[1]
    freq = 1 + (w * (65536 - n)) // w.sum(1, keepdims=True)
    freq[:, amax] += 65536 - freq.sum(1)
    cdf = np.zeros((len(r), n + 1), np.int64)
    cdf[:, 1:] = np.cumsum(freq, 1)
    return cdf.astype(np.int32)


def choose_ratio(abs_hist):
    """Q16 ratio of the geometric table for a subband with abs_hist[k] values of magnitude k: the moment fit
    E|q| = 2 r / (1 - r^2).  The encoder's choice only: the decoder reads the 16 bits."""
    n = float(abs_hist.sum())
    mean = float((abs_hist * np.arange(len(abs_hist))).sum()) / n if n else 0.0
    r = (np.sqrt(1.0 + mean * mean) - 1.0) / mean if mean > 0 else 0.0
    return int(min(65535, max(1, int(round(r * 65536)))))


# ---------------------------------------------------------------------------------------------------------------- container
def coded_levels(level_counts):
    """L: the levels 0 .. L-1 are range coded, the leaves of the levels >= L (DC included) are stored raw"""
    counts = [int(c) for c in level_counts]
    above, l = counts[-1], len(counts) - 1
    while l > 0 and above + counts[l - 1] <= RAW_LEAVES:
        l -= 1
        above += counts[l]
    return l


def _zigzag(v):
    v = np.asarray(v, np.int64)
    return (v << 1) ^ (v >> 63)


def _put_varints(values):
    out = bytearray()
    for v in np.asarray(values, np.int64).reshape(-1).tolist():
        while v >= 0x80:
            out.append((v & 0x7F) | 0x80)
            v >>= 7
        out.append(v)
    return bytes(out)


def _get_varints(buf, at, n, what):
    out = np.empty(n, np.int64)
    for i in range(n):
        v, shift = 0, 0
        while True:
            if at >= len(buf) or shift > 63:
                raise ValueError(".colors: truncated or corrupt %s" % what)
            b = buf[at]
            at += 1
            v |= (b & 0x7F) << shift
            shift += 7
            if b < 0x80:
                break
        out[i] = v
    return out, at


def _unzigzag(u):
    return (u >> 1) ^ -(u & 1)


def _crc(payload):
    buf = np.frombuffer(payload, np.uint8)
    return int(_lib.host().pcgc_crc32c(0, _lib.nptr(buf) if buf.size else None, buf.size))


def _geometry_crc(counts):
    return _crc(np.asarray(counts, "<i8").tobytes())


def pack(d, m, qstep, level_counts, amax, symbols, tail, esc_pos=(), esc_val=()):
    """The file's bytes.  level_counts [3d + 1] leaves per subband; amax [L] alphabet half-widths of the coded levels; symbols
    int16 [K,3] of the K leaves of the coded levels in subband order (q + amax, or 2 amax + 1 = escape); tail int [M - K, 3]
    = q of the raw leaves; esc_pos / esc_val: positions k * 3 + c (ascending) and values of the escaped q."""
    from . import coder_ops
    counts = [int(c) for c in level_counts]
    n_coded = coded_levels(counts)
    k_raw = sum(counts[:n_coded])
    symbols = np.ascontiguousarray(symbols, np.int16).reshape(-1, 3)
    tail = np.asarray(tail, np.int64).reshape(-1, 3)
    if len(counts) != 3 * d + 1 or sum(counts) != m or len(symbols) != k_raw or len(tail) != m - k_raw or len(amax) != n_coded:
        raise ValueError("colour container: the symbols do not fit the level counts")
    table, streams = [], []
    at = 0
    for l in range(n_coded):
        s = symbols[at:at + counts[l]]
        at += counts[l]
        a = int(amax[l])
        ratios = [choose_ratio(np.bincount(np.abs(s[:, c].astype(np.int64) - a).clip(max=a + 1), minlength=a + 2)) for c in range(3)]
        stream = coder_ops.range_encode(s, build_tables(a, ratios)[None]) if len(s) else b""
        table.append(struct.pack("<HHHHI", a, ratios[0], ratios[1], ratios[2], len(stream)))
        streams.append(stream)
    esc_pos = np.asarray(esc_pos, np.int64).reshape(-1)
    esc = np.stack([np.diff(esc_pos, prepend=0), _zigzag(esc_val)], -1) if len(esc_pos) else np.zeros((0, 2), np.int64)
    payload = b"".join(table) + b"".join(streams) + _put_varints(esc) + _put_varints(_zigzag(tail))
    head = MAGIC + struct.pack("<BBHQdIII", VERSION, d, n_coded, m, float(qstep), _crc(payload), len(esc_pos), _geometry_crc(counts))
    return head + payload


def unpack(data, d, m, level_counts):
    """-> (qstep, amax int32 [L], symbols int16 [K,3], patch int32 [P,2]): patch rows (k * 3 + c, q) hold the escaped values and
    the raw tail.  d, m and level_counts are the decoded geometry's; every disagreement is a ValueError that says which."""
    from . import coder_ops
    data = bytes(data)
    if len(data) < HEADER_BYTES:
        raise ValueError(".colors: %d bytes, shorter than its %d-byte header (truncated file)" % (len(data), HEADER_BYTES))
    if data[:4] != MAGIC:
        raise ValueError(".colors: wrong magic %r (want %r): not a colour stream" % (data[:4], MAGIC))
    version, fd, n_coded, fm, qstep, crc, n_esc, gcrc = struct.unpack("<BBHQdIII", data[4:HEADER_BYTES])
    if version != VERSION:
        raise ValueError(".colors: version %d, this decoder reads version %d" % (version, VERSION))
    if fd != d or fm != m:
        raise ValueError(".colors was coded for other geometry: it holds d = %d, M = %d, the decoded points have d = %d, M = %d"
                         % (fd, fm, d, m))
    counts = [int(c) for c in level_counts]
    if n_coded != coded_levels(counts):
        raise ValueError(".colors was coded for other geometry: %d coded levels, the decoded points give %d" % (n_coded, coded_levels(counts)))
    if gcrc != _geometry_crc(counts):
        raise ValueError(".colors was coded for other geometry: same d and M, but the octree of the decoded points has other level sizes")
    if not (qstep > 0 and np.isfinite(qstep)):
        raise ValueError(".colors: color_qstep %r is not a positive number" % (qstep,))
    payload = data[HEADER_BYTES:]
    if len(payload) < LEVEL_BYTES * n_coded:
        raise ValueError(".colors: truncated in the level table")
    if _crc(payload) != crc:
        raise ValueError(".colors: checksum mismatch (truncated or corrupt payload)")
    rows = [struct.unpack("<HHHHI", payload[LEVEL_BYTES * l:LEVEL_BYTES * (l + 1)]) for l in range(n_coded)]
    at = LEVEL_BYTES * n_coded
    k_raw = sum(counts[:n_coded])
    symbols = np.empty((k_raw, 3), np.int16)
    k = 0
    for l, (a, r0, r1, r2, nbytes) in enumerate(rows):
        if at + nbytes > len(payload) or (counts[l] == 0) != (nbytes == 0):
            raise ValueError(".colors: the stream of level %d does not fit the file" % l)
        if counts[l]:
            symbols[k:k + counts[l]] = coder_ops.range_decode(payload[at:at + nbytes], (counts[l], 3), build_tables(a, [r0, r1, r2])[None])
        at += nbytes
        k += counts[l]
    esc, at = _get_varints(payload, at, 2 * n_esc, "escape list")
    esc = esc.reshape(-1, 2)
    tail, at = _get_varints(payload, at, 3 * (m - k_raw), "raw tail")
    if at != len(payload):
        raise ValueError(".colors: %d bytes after the raw tail" % (len(payload) - at))
    esc_pos = np.cumsum(esc[:, 0])
    if len(esc_pos) and esc_pos[-1] >= 3 * k_raw:
        raise ValueError(".colors: an escape position lies outside the coded levels")
    patch = np.concatenate([np.stack([esc_pos, _unzigzag(esc[:, 1])], -1),
                            np.stack([np.arange(3 * k_raw, 3 * m, dtype=np.int64), _unzigzag(tail)], -1)]).astype(np.int32)
    return float(qstep), np.array([r[0] for r in rows], np.int32), symbols, patch


def header_bytes(data):
    """bytes of the header and the level table (what the rate test does not count as payload)"""
    return HEADER_BYTES + LEVEL_BYTES * struct.unpack("<H", bytes(data[6:8]))[0]


def write_colors_file(filename, data):
    with open(filename, "wb") as f:
        f.write(data)
    return len(data)


def read_colors_file(filename):
    with open(filename, "rb") as f:
        return f.read()


# ---------------------------------------------------------------------------------------------------------------- device side
class Plan:
    """The tree of one geometry on the device: the sort, and per leaf subband / left sibling / right weight / subband order."""

    def __init__(self, points):
        import torch
        self.dev = dev = _lib.require_gpu()
        lib = _lib.hip()
        p = np.asarray(points)
        if p.ndim != 2 or p.shape[1] < 3 or p.dtype.kind not in "iu":
            raise ValueError("colour codec: points must be an integer array [M, 3] (got %s %s): voxelised clouds only" % (p.dtype, p.shape))
        if len(p) == 0:
            raise ValueError("colour codec: the cloud is empty")
        p = np.ascontiguousarray(p[:, :3])
        if int(p.min()) < 0 or int(p.max()) > MAX_COORD:
            raise ValueError("colour codec: coordinates must lie within [0, %d] (got %d .. %d)" % (MAX_COORD, int(p.min()), int(p.max())))
        self.m = m = len(p)
        self.d = d = int(p.max()).bit_length()
        p_d = torch.from_numpy(p.astype(np.int32)).to(dev)
        keys = torch.empty(m, dtype=torch.int64, device=dev)
        _lib.check(lib.pcgc_raht_keys(_lib.dptr(p_d), m, _lib.dptr(keys), _lib.stream()), "pcgc_raht_keys")
        self.keys, self.point_of_leaf = torch.sort(keys)
        if m > 1 and bool((self.keys[1:] == self.keys[:-1]).any()):
            raise ValueError("colour codec: the cloud holds duplicate points (pass unique voxels)")
        self.subband, self.left, self.w_right, self.order = (torch.empty(m, dtype=torch.int32, device=dev) for _ in range(4))
        self.ws = torch.empty(int(lib.pcgc_raht_workspace_bytes(m)), dtype=torch.uint8, device=dev)
        self.level_counts = np.zeros(3 * d + 1, np.int64)
        _lib.check(lib.pcgc_raht_structure(_lib.dptr(self.keys), m, d, _lib.dptr(self.subband), _lib.dptr(self.left), _lib.dptr(self.w_right),
                                           _lib.dptr(self.order), _lib.nptr(self.level_counts), _lib.dptr(self.ws), self.ws.numel(),
                                           _lib.stream()), "pcgc_raht_structure")
        self.launches = 0

    def transform(self, attr, inverse=False, fuse_top=True):
        """in place on attr float64 [M,3] (device, leaf order)"""
        import ctypes
        lib = _lib.hip()
        n = ctypes.c_int(0)
        fn = lib.pcgc_raht_inverse if inverse else lib.pcgc_raht_forward
        _lib.check(fn(_lib.dptr(attr), self.m, self.d, _lib.dptr(self.left), _lib.dptr(self.w_right), _lib.dptr(self.subband),
                      _lib.dptr(self.order), _lib.nptr(self.level_counts), 1 if fuse_top else 0, ctypes.byref(n), _lib.dptr(self.ws),
                      self.ws.numel(), _lib.stream()), "pcgc_raht_inverse" if inverse else "pcgc_raht_forward")
        self.launches = n.value
        return attr


def _clock(timings, key, t0):
    """stage times for tools/bench_colorcodec.py: device-synchronised, only when a dict is passed"""
    if timings is None:
        return t0
    import time
    import torch
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    timings[key] = timings.get(key, 0.0) + (t1 - t0)
    return t1


def _start(timings):
    if timings is None:
        return 0.0
    import time
    import torch
    torch.cuda.synchronize()
    return time.perf_counter()


def raht_forward(points, attrs, fuse_top=True):
    """points int [M,3] unique voxels, attrs [M,3] -> (coef float64 [M,3], subband int32 [M], weight int64 [M]); row j belongs to
    the j-th point in Morton order: row 0 is the DC, row j > 0 the coefficient of the merge whose right-hand node starts there"""
    import torch
    plan = Plan(points)
    a = np.asarray(attrs)
    if a.shape != (plan.m, 3):
        raise ValueError("raht_forward: attrs must be [%d, 3] (got %s)" % (plan.m, a.shape))
    attr = torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(plan.dev)[plan.point_of_leaf].contiguous()
    plan.transform(attr, fuse_top=fuse_top)
    leaf = torch.arange(plan.m, device=plan.dev, dtype=torch.int64)
    weight = leaf - plan.left.to(torch.int64) + plan.w_right.to(torch.int64)
    return attr.cpu().numpy(), plan.subband.cpu().numpy(), weight.cpu().numpy()


def raht_inverse(points, coef, fuse_top=True):
    """coef [M,3] in raht_forward's row order -> attributes float64 [M,3] in the order of `points`"""
    import torch
    plan = Plan(points)
    c = np.asarray(coef)
    if c.shape != (plan.m, 3):
        raise ValueError("raht_inverse: coef must be [%d, 3] (got %s)" % (plan.m, c.shape))
    attr = torch.from_numpy(np.ascontiguousarray(c, np.float64)).to(plan.dev)
    plan.transform(attr, inverse=True, fuse_top=fuse_top)
    out = torch.empty_like(attr)
    out[plan.point_of_leaf] = attr
    return out.cpu().numpy()


def _check_step(qstep):
    q = float(qstep)
    if not (q > 0 and np.isfinite(q)):
        raise ValueError("colour codec: color_qstep must be a positive number (got %r)" % (qstep,))
    return q


def encode_colors(points, colors, qstep, fuse_top=True, timings=None):
    """points int [M,3] unique voxels in [0, 4095], colors uint8 [M,3], qstep > 0 -> the bytes of <name>.colors"""
    import torch
    lib = _lib.hip()
    qstep = _check_step(qstep)
    col = np.asarray(colors)
    n = len(np.asarray(points))
    if col.shape != (n, 3) or col.dtype != np.uint8:
        raise ValueError("colour codec: colors must be uint8 [%d, 3] (got %s %s)" % (n, col.dtype, col.shape))
    t = _start(timings)
    plan = Plan(points)
    t = _clock(timings, "sort + structure", t)
    m, dev, s = plan.m, plan.dev, _lib.stream()
    rgb = torch.from_numpy(np.ascontiguousarray(col)).to(dev)
    attr = torch.empty((m, 3), dtype=torch.float64, device=dev)
    _lib.check(lib.pcgc_raht_load_colors(_lib.dptr(rgb), _lib.dptr(plan.point_of_leaf), m, _lib.dptr(attr), s), "pcgc_raht_load_colors")
    plan.transform(attr, fuse_top=fuse_top)
    t = _clock(timings, "transform", t)
    q = torch.empty((m, 3), dtype=torch.int32, device=dev)
    maxabs_d = torch.empty(64, dtype=torch.int32, device=dev)
    _lib.check(lib.pcgc_raht_quantize(_lib.dptr(attr), _lib.dptr(plan.order), _lib.dptr(plan.subband), m, qstep, _lib.dptr(q),
                                      _lib.dptr(maxabs_d), s), "pcgc_raht_quantize")
    maxabs = maxabs_d.cpu().numpy()
    n_coded = coded_levels(plan.level_counts)
    k_raw = int(plan.level_counts[:n_coded].sum())
    amax = np.minimum(maxabs[:n_coded], AMAX_CAP).astype(np.int32)
    amax_d = torch.zeros(64, dtype=torch.int32, device=dev)
    amax_d[:n_coded] = torch.from_numpy(amax).to(dev)
    sym = torch.empty((k_raw, 3), dtype=torch.int16, device=dev)
    _lib.check(lib.pcgc_raht_symbols(_lib.dptr(q), _lib.dptr(plan.order), _lib.dptr(plan.subband), k_raw, _lib.dptr(amax_d), _lib.dptr(sym), s),
               "pcgc_raht_symbols")
    symbols = sym.cpu().numpy()
    tail = q[k_raw:].cpu().numpy()
    esc_pos, esc_val = np.zeros(0, np.int64), np.zeros(0, np.int64)
    if (maxabs[:n_coded] > AMAX_CAP).any():              # rare: only then can a symbol be the escape
        esc_of_row = np.repeat(2 * amax.astype(np.int64) + 1, plan.level_counts[:n_coded])
        esc_pos = np.flatnonzero((symbols == esc_of_row[:, None].astype(np.int16)).reshape(-1))
        esc_val = q.reshape(-1)[torch.from_numpy(esc_pos).to(dev)].cpu().numpy()
    t = _clock(timings, "quantise + symbols", t)
    data = pack(plan.d, m, qstep, plan.level_counts, amax, symbols, tail, esc_pos, esc_val)
    _clock(timings, "host coding", t)
    if timings is not None:
        timings["launches"] = plan.launches
    return data


def decode_colors(points, data, fuse_top=True, timings=None):
    """points: the decoded geometry the stream was coded for, data: the bytes of <name>.colors -> uint8 [M,3] in the order of
    `points`.  A stream coded for other geometry, a truncated or a corrupt one raises ValueError."""
    import torch
    lib = _lib.hip()
    t = _start(timings)
    plan = Plan(points)
    t = _clock(timings, "sort + structure", t)
    m, dev, s = plan.m, plan.dev, _lib.stream()
    qstep, amax, symbols, patch = unpack(data, plan.d, m, plan.level_counts)
    t = _clock(timings, "host coding", t)
    amax_d = torch.zeros(64, dtype=torch.int32, device=dev)
    amax_d[:len(amax)] = torch.from_numpy(amax).to(dev)
    sym = torch.from_numpy(symbols).to(dev)
    patch_d = torch.from_numpy(np.ascontiguousarray(patch)).to(dev)
    attr = torch.empty((m, 3), dtype=torch.float64, device=dev)
    _lib.check(lib.pcgc_raht_dequantize(_lib.dptr(sym) if len(symbols) else None, len(symbols), _lib.dptr(patch_d), len(patch),
                                        _lib.dptr(plan.order), _lib.dptr(plan.subband), _lib.dptr(amax_d), m, qstep, _lib.dptr(attr), s),
               "pcgc_raht_dequantize")
    t = _clock(timings, "quantise + symbols", t)
    plan.transform(attr, inverse=True, fuse_top=fuse_top)
    out = torch.empty((m, 3), dtype=torch.uint8, device=dev)
    _lib.check(lib.pcgc_raht_store_colors(_lib.dptr(attr), _lib.dptr(plan.point_of_leaf), m, _lib.dptr(out), s), "pcgc_raht_store_colors")
    colors = out.cpu().numpy()
    _clock(timings, "transform", t)
    if timings is not None:
        timings["launches"] = plan.launches
    return colors
