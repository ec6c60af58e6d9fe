"""Colour codec for decoded geometry: RAHT + uniform quantiser + static entropy coding -> <name>.colors.

    data = encode_colors(points, colors, qstep)          # points int [M,3] unique voxels, colors uint8 [M,3]
    data = encode_colors(points, colors, qstep, coder="rans")            # stream version 2: the entropy coder runs on the GPU too
    colors = decode_colors(points, data)                 # uint8 [M,3] in the order of `points`; either version
    data, report = encode_colors_target(points, colors, psnr=38)         # the step chosen on the grid 2^(j/8): at least 38 dB luma
    data, report = encode_colors_target(points, colors, bpp=0.6)         # ... or at most 0.6 bits per point; an ordinary file either way

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

Version 2 (coder="rans"; tests/_rans_ref.py is its definition in numpy, csrc/rans.hip codes it): the same header with version = 2,
the same q, tables, escapes and raw tail; only the entropy coder of the large levels differs.  A level of at least
RANS_MIN_SYMBOLS symbols (3 x its leaves) is cut into chunks of 64 RANS_STEPS symbols (the last one shorter) and every chunk is
coded on its own with 64 interleaved rANS lanes (state uint32, lower bound 2^16, 16-bit words; symbol j of a chunk belongs to
lane j % 64 and step j / 64, its table is the level's table of channel (first + j) % 3).  A chunk's bytes are its min(n, 64) final
states (uint32, lane ascending) and then its words in the order the decoder takes them (steps ascending, lanes ascending
within a step).  A smaller level keeps version 1's range stream: a chunk carries up to 256 bytes of states, more than the top
levels' whole payload.

    36  14 L  per coded level: amax u16, ratio[Y, Co, Cg] u16 (Q16), coder u16 (0 = range, 1 = rANS), stream bytes u32
    then, for the rANS levels in level order, one u32 per chunk: the chunk's bytes (ceil(3 leaves / (64 RANS_STEPS)) chunks per
    level; they add up to the level's stream bytes), then the L streams, the escapes and the raw tail as in version 1.

In the code the two versions are one format: a version 1 file is a file whose levels are all range coded.  _FORMATS says what a
version decides (the level row, and whether it names a coder and a chunk table follows); _write lays out and _read checks and
reads either version (pack / assemble_v2 and unpack / unpack_v2 are their callers); _encode_coef and decode_colors code every
level with the coder level_coders gives it, from the same device-side sums, tables and escapes.
"""
import itertools
import struct

import numpy as np

from . import _lib

MAGIC = b"PCRA"
VERSION = 1
VERSION_RANS = 2           # the stream version coder="rans" writes
HEADER_BYTES = 36
CODER_RANGE, CODER_RANS = 0, 1
# all that a stream version decides: the layout of a level row and whether the rows name a coder (then rANS levels exist and
# their chunk table follows the rows; without the field every level is range coded)
_FORMATS = {VERSION: (struct.Struct("<HHHHI"), False), VERSION_RANS: (struct.Struct("<HHHHHI"), True)}
_VERSION_OF = {"range": VERSION, "rans": VERSION_RANS}
LEVEL_BYTES, LEVEL_BYTES_RANS = _FORMATS[VERSION][0].size, _FORMATS[VERSION_RANS][0].size          # 12, 14
RANS_LANES = 64
# format constants of version 2, confirmed from profiles/colorcodec_rans_rd.txt (bytes of the alternatives on both clouds) and
# profiles/colorcodec_rans_bench.txt (times at S = 512 ... 4096); DESIGN.md 7d gives the reasoning
RANS_STEPS = 2048          # S: a chunk holds up to 64 S symbols
RANS_MIN_SYMBOLS = 16384   # T: a level with fewer symbols keeps the range coder
RANS_LOW = 1 << 16         # L: the lower bound of a lane's state, and its value before the first and after the last symbol
RAW_LEAVES = 48            # the top of the tree, at most this many leaves (DC included), is stored raw
AMAX_CAP = 2047            # largest |q| with a symbol of its own; larger values take the escape symbol
MAX_COORD = 4095           # 12-bit clouds, as recolor
SUBBANDS = 37              # subbands of a 12-bit cloud, the DC included: 3 * 12 + 1 (kBins in the kernels)
LEVEL_SLOTS = 64           # entries of the per-level int32 device buffers (amax, max |q|): SUBBANDS and room to spare


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


def ratios_of_sums(abs_sums, n):
    """Q16 ratios of the geometric tables for subbands of n values (broadcast) whose magnitudes add up to abs_sums int [...]
    (pcgc_raht_abs_sums) -> int64 [...]: the moment fit E|q| = 2 r / (1 - r^2).  The encoder's choice only: the decoder reads
    the 16 bits."""
    a = np.asarray(abs_sums, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = np.where(np.asarray(n) > 0, a / np.asarray(n, np.float64), 0.0)
        r = np.where(mean > 0, (np.sqrt(1.0 + mean * mean) - 1.0) / mean, 0.0)
    return np.clip(np.rint(r * 65536), 1, 65535).astype(np.int64)


def ratio_of_sum(abs_sum, n):
    """ratios_of_sums for one subband -> int"""
    return int(ratios_of_sums(abs_sum, n))


def choose_ratio(abs_hist):
    """ratio_of_sum for a subband with abs_hist[k] values of magnitude k"""
    return ratio_of_sum(int((abs_hist * np.arange(len(abs_hist))).sum()), int(abs_hist.sum()))


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


def _row_base(counts, n_coded):
    """int64 [n_coded + 1]: the first row of every coded level in the [K,3] symbol array, and K"""
    return np.concatenate([[0], np.cumsum(counts[:n_coded], dtype=np.int64)]).astype(np.int64)


def rans_chunk_count(n_symbols, steps=None):
    """chunks of a level of n_symbols symbols"""
    per = RANS_LANES * (RANS_STEPS if steps is None else steps)
    return -(-int(n_symbols) // per)


def level_coders(level_counts, version=VERSION_RANS):
    """the coder of every coded level: rANS from RANS_MIN_SYMBOLS symbols on where the version has it, else the range coder"""
    counts = [int(c) for c in level_counts]
    rans = _FORMATS[version][1]
    return [CODER_RANS if rans and 3 * c >= RANS_MIN_SYMBOLS else CODER_RANGE for c in counts[:coded_levels(counts)]]


def _write(version, d, m, qstep, level_counts, amax, ratios, streams, chunk_sizes, tail, esc_pos, esc_val, what="streams"):
    """The file's bytes, either version.  level_counts [3d + 1] leaves per subband; per coded level amax[l], ratios[l] [3], streams[l]
    = its bytes from the coder level_coders names and chunk_sizes[l] = the bytes of each of its chunks (rANS levels; anything
    empty otherwise); tail int [M - K, 3] = q of the raw leaves; esc_pos / esc_val: positions k * 3 + c (ascending) and values of
    the escaped q."""
    row, names_coder = _FORMATS[version]
    counts = [int(c) for c in level_counts]
    n_coded = coded_levels(counts)
    kinds = level_coders(counts, version)
    tail = np.asarray(tail, np.int64).reshape(-1, 3)
    if len(counts) != 3 * d + 1 or sum(counts) != m or len(tail) != m - sum(counts[:n_coded]) or not (
            len(amax) == len(ratios) == len(streams) == len(chunk_sizes) == n_coded):
        raise ValueError("colour container: the %s do not fit the level counts" % what)
    table, chunk_table = [], []
    for l in range(n_coded):
        if kinds[l] == CODER_RANS:
            sizes = np.asarray(chunk_sizes[l], np.int64).reshape(-1)
            if len(sizes) != rans_chunk_count(3 * counts[l]) or int(sizes.sum()) != len(streams[l]):
                raise ValueError("colour container: the chunks of level %d do not fit its stream" % l)
            chunk_table.append(sizes.astype("<u4").tobytes())
        table.append(row.pack(int(amax[l]), *(int(r) for r in ratios[l]), *([kinds[l]] if names_coder else []), len(streams[l])))
    esc_pos = np.asarray(esc_pos, np.int64).reshape(-1)
    esc = np.stack([np.diff(esc_pos, prepend=0), _zigzag(esc_val)], -1) if len(esc_pos) else np.zeros((0, 2), np.int64)
    payload = b"".join(table) + b"".join(chunk_table) + b"".join(bytes(x) for x in streams) + _put_varints(esc) + _put_varints(_zigzag(tail))
    head = MAGIC + struct.pack("<BBHQdIII", version, d, n_coded, m, float(qstep), _crc(payload), len(esc_pos), _geometry_crc(counts))
    return head + payload


def pack(d, m, qstep, level_counts, amax, symbols, tail, esc_pos=(), esc_val=()):
    """The bytes of a version 1 file from symbols: _write's arguments, but symbols int16 [K,3] of the K leaves of the coded levels
    in subband order (q + amax, or 2 amax + 1 = escape) for the streams; the tables are fitted to them here."""
    from . import coder_ops
    counts = [int(c) for c in level_counts]
    n_coded = coded_levels(counts)
    base = _row_base(counts, n_coded)
    symbols = np.ascontiguousarray(symbols, np.int16).reshape(-1, 3)
    if len(symbols) != base[-1] or len(amax) != n_coded:
        raise ValueError("colour container: the symbols do not fit the level counts")
    level = [symbols[base[l]:base[l + 1]] for l in range(n_coded)]
    sums = [np.minimum(np.abs(s.astype(np.int64) - int(a)), int(a) + 1).sum(0) for s, a in zip(level, amax)]       # the escape counts as amax + 1
    ratios = ratios_of_sums(np.reshape(sums, (n_coded, 3)), np.reshape(counts[:n_coded], (n_coded, 1)))
    streams = [coder_ops.range_encode(s, build_tables(a, r)[None]) if len(s) else b"" for s, a, r in zip(level, amax, ratios)]
    return _write(VERSION, d, m, qstep, counts, amax, ratios, streams, [()] * n_coded, tail, esc_pos, esc_val, what="symbols")


def assemble_v2(d, m, qstep, level_counts, amax, ratios, streams, chunk_sizes, tail, esc_pos=(), esc_val=()):
    """The bytes of a version 2 file from coded streams: streams[l] = the bytes of level l (range or rANS, level_coders says
    which), chunk_sizes[l] = the bytes of each of its chunks (rANS levels; anything empty otherwise)."""
    return _write(VERSION_RANS, d, m, qstep, level_counts, amax, ratios, streams, chunk_sizes, tail, esc_pos, esc_val)


def _read_patch(payload, at, n_esc, k_raw, m):
    """the escape list and the raw tail, from payload[at:] to its end -> patch int32 [P,2]"""
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
    return patch


def _read(data, d, m, level_counts, want_version=None):
    """The host's half of reading a file of either version (want_version: that one alone): every check that needs no symbol, and
    the range-coded levels.  -> (qstep, amax int32 [L], ratios int32 [L,3], kinds [L], streams [L] (bytes; b"" for a range level),
    chunk_sizes [L] (int64 arrays), symbols int16 [K,3] with the rows of the range-coded levels filled in and the others 0, patch
    int32 [P,2]: rows (k * 3 + c, q) of the escaped values and the raw tail).  d, m and level_counts are the decoded geometry's;
    every disagreement is a ValueError that says which."""
    from . import coder_ops
    data = bytes(data)
    if len(data) < HEADER_BYTES:
        raise ValueError(".colors: %d bytes, shorter than its %d-byte header (truncated file)" % (len(data), HEADER_BYTES))
    if data[:4] != MAGIC:
        raise ValueError(".colors: wrong magic %r (want %r): not a colour stream" % (data[:4], MAGIC))
    version, fd, n_coded, fm, qstep, crc, n_esc, gcrc = struct.unpack("<BBHQdIII", data[4:HEADER_BYTES])
    if (version not in _FORMATS) if want_version is None else (version != want_version):
        raise ValueError(".colors: version %d, this decoder reads version %d" % (version, want_version or VERSION))
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
    row, names_coder = _FORMATS[version]
    payload = data[HEADER_BYTES:]
    if len(payload) < row.size * n_coded:
        raise ValueError(".colors: truncated in the level table")
    if _crc(payload) != crc:
        raise ValueError(".colors: checksum mismatch (truncated or corrupt payload)")
    rows = [row.unpack_from(payload, row.size * l) for l in range(n_coded)]
    kinds = level_coders(counts, version)
    at = row.size * n_coded
    chunk_sizes = []
    for l, (a, r0, r1, r2, *kind, nbytes) in enumerate(rows):
        if names_coder and kind[0] != kinds[l]:
            raise ValueError(".colors: level %d (%d symbols) names coder %d, the format gives it coder %d" % (l, 3 * counts[l], kind[0], kinds[l]))
        if a > AMAX_CAP or min(r0, r1, r2) < 1:
            raise ValueError(".colors: the table of level %d (amax %d, ratios %d %d %d) is outside the format" % (l, a, r0, r1, r2))
        sizes = np.zeros(0, np.int64)
        if kinds[l] == CODER_RANS:
            n_chunks = rans_chunk_count(3 * counts[l])
            if at + 4 * n_chunks > len(payload):
                raise ValueError(".colors: truncated in the chunk table of level %d" % l)
            sizes = np.frombuffer(payload, "<u4", n_chunks, at).astype(np.int64)
            at += 4 * n_chunks
            per = RANS_LANES * RANS_STEPS
            n_of = np.minimum(per, 3 * counts[l] - per * np.arange(n_chunks, dtype=np.int64))
            states = 4 * np.minimum(n_of, RANS_LANES)
            if (sizes & 1).any():
                raise ValueError(".colors: a chunk of level %d has an odd number of word bytes" % l)
            if (sizes < states).any() or (sizes > states + 2 * n_of).any():
                raise ValueError(".colors: a chunk of level %d cannot hold its states and at most one word per symbol" % l)
            if int(sizes.sum()) != nbytes:
                raise ValueError(".colors: the chunks of level %d hold %d bytes, its stream %d" % (l, int(sizes.sum()), nbytes))
        chunk_sizes.append(sizes)
    base = _row_base(counts, n_coded)
    symbols = np.zeros((int(base[-1]), 3), np.int16)
    streams = []
    for l, (a, r0, r1, r2, *_, nbytes) in enumerate(rows):
        if at + nbytes > len(payload) or (counts[l] == 0 and nbytes != 0):   # a level of zeros alone may take no bytes
            raise ValueError(".colors: the stream of level %d does not fit the file (byte counts overrun the payload)" % l)
        if kinds[l] == CODER_RANS:
            streams.append(payload[at:at + nbytes])
        else:
            streams.append(b"")
            if counts[l]:
                symbols[base[l]:base[l + 1]] = coder_ops.range_decode(payload[at:at + nbytes], (counts[l], 3), build_tables(a, [r0, r1, r2])[None])
        at += nbytes
    patch = _read_patch(payload, at, n_esc, int(base[-1]), m)
    return (float(qstep), np.array([r[0] for r in rows], np.int32), np.array([r[1:4] for r in rows], np.int32).reshape(-1, 3), kinds, streams,
            chunk_sizes, symbols, patch)


def unpack(data, d, m, level_counts):
    """a version 1 file -> (qstep, amax int32 [L], symbols int16 [K,3], patch int32 [P,2]) of _read"""
    qstep, amax, _, _, _, _, symbols, patch = _read(data, d, m, level_counts, VERSION)
    return qstep, amax, symbols, patch


def unpack_v2(data, d, m, level_counts):
    """a version 2 file -> all that _read returns; the rANS levels' rows of symbols are left for the kernel"""
    return _read(data, d, m, level_counts, VERSION_RANS)


def header_bytes(data):
    """bytes of the header and the level table (what the rate test does not count as payload); version 2's chunk table is payload"""
    row = _FORMATS.get(bytes(data[4:5])[0], _FORMATS[VERSION])[0]
    return HEADER_BYTES + row.size * struct.unpack("<H", bytes(data[6:8]))[0]


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


# ---------------------------------------------------------------------------------------------------------------- rANS on the device
class _RansJob:
    """The chunks of some runs of symbols (run i: counts[i] symbols from index bases[i] of one flat int16 array, tables cdfs[i] int32
    [3, symbols + 1]) and their tables on the device, for pcgc_rans_encode / pcgc_rans_decode."""

    def __init__(self, bases, counts, cdfs, steps, dev):
        import torch
        per = RANS_LANES * int(steps)
        if steps < 1 or steps > 1 << 20:
            raise ValueError("rANS: steps_per_chunk %r outside [1, 2^20]" % (steps,))
        self.steps, self.dev = int(steps), dev
        self.per_run = [-(-int(n) // per) for n in counts]
        rows = []
        for i, (b, n) in enumerate(zip(bases, counts)):
            first = np.arange(self.per_run[i], dtype=np.int64) * per
            rows.append(np.stack([np.full_like(first, i), int(b) + first, np.minimum(per, int(n) - first)], -1))
        self.chunks = np.concatenate(rows) if rows else np.zeros((0, 3), np.int64)
        self.n_chunks = len(self.chunks)
        cdfs = [np.ascontiguousarray(c, np.int32) for c in cdfs]
        for c in cdfs:
            if c.ndim != 2 or c.shape[0] != 3 or not (3 <= c.shape[1] <= 2 * AMAX_CAP + 3) or (c[:, 0] != 0).any() or (
                    c[:, -1] != 65536).any() or (np.diff(c, axis=1) < 1).any():
                raise ValueError("rANS: a table is not three 16-bit CDFs of 2 .. %d symbols with every frequency >= 1" % (2 * AMAX_CAP + 2))
        self.n_runs = len(cdfs)
        if self.n_chunks:
            self.max_entries = max(c.shape[1] for c in cdfs)
            off = np.cumsum([0] + [c.size for c in cdfs]).astype(np.int64)
            self.cdf_total = int(off[-1])
            self.cdfs_d = torch.from_numpy(np.concatenate([c.reshape(-1) for c in cdfs])).to(dev)
            self.off_d = torch.from_numpy(off).to(dev)
            self.chunks_d = torch.from_numpy(np.ascontiguousarray(self.chunks)).to(dev)

    def split(self, per_chunk):
        """per-chunk values -> one array per run"""
        return np.split(np.asarray(per_chunk), np.cumsum(self.per_run)[:-1]) if self.per_run else []

    def encode(self, sym_d, timings=None):
        """sym_d int16 device tensor (flat) -> (the chunks' bytes back to back, int64 [n_chunks] bytes of each).  Two copies come
        back: the chunk offsets (8 bytes per chunk), which tell how many bytes there are, and then those bytes."""
        import torch
        if not self.n_chunks:
            return b"", np.zeros(0, np.int64)
        lib = _lib.hip()
        n = sym_d.numel()
        coded = int(self.chunks[:, 2].sum())                             # the worst case: every symbol a word, every chunk 64 states
        out = torch.empty(2 * coded + 4 * RANS_LANES * self.n_chunks, dtype=torch.uint8, device=self.dev)
        t = _start(timings)
        offsets = torch.empty(self.n_chunks + 1, dtype=torch.int64, device=self.dev)
        ws = torch.empty(int(lib.pcgc_rans_workspace_bytes(self.n_chunks, self.steps)), dtype=torch.uint8, device=self.dev)
        _lib.check(lib.pcgc_rans_encode(_lib.dptr(sym_d), n, _lib.dptr(self.chunks_d), self.n_chunks, _lib.dptr(self.cdfs_d), _lib.dptr(self.off_d),
                                        self.n_runs, self.cdf_total, self.max_entries, self.steps, _lib.dptr(out), out.numel(), _lib.dptr(offsets),
                                        _lib.dptr(ws), ws.numel(), _lib.stream()), "pcgc_rans_encode")
        t = _clock(timings, "sub: rANS encode kernels", t)
        off = offsets.cpu().numpy()
        sizes = np.diff(off)
        if (sizes < 4).any():
            raise _lib.PcgcError("pcgc_rans_encode refused chunk %d" % int(np.flatnonzero(sizes < 4)[0]))
        payload = out[:int(off[-1])].cpu().numpy().tobytes()
        _clock(timings, "sub: read-back of offsets and bytes", t)
        return payload, sizes

    def decode(self, payload, sizes, sym_d, timings=None):
        """writes the symbols into sym_d (int16 device tensor, flat) -> status int32 [n_chunks]"""
        import torch
        if not self.n_chunks:
            return np.zeros(0, np.int32)
        lib = _lib.hip()
        off = np.concatenate([[0], np.cumsum(np.asarray(sizes, np.int64))]).astype(np.int64)
        if len(off) != self.n_chunks + 1 or int(off[-1]) != len(payload) or len(payload) == 0:
            raise ValueError("rANS: %d chunk sizes adding up to %d bytes for %d chunks in %d bytes" % (len(off) - 1, int(off[-1]), self.n_chunks, len(payload)))
        t = _start(timings)
        pay_d = torch.from_numpy(np.frombuffer(bytearray(payload), np.uint8)).to(self.dev)
        off_d = torch.from_numpy(off).to(self.dev)
        status = torch.empty(self.n_chunks, dtype=torch.int32, device=self.dev)
        t = _clock(timings, "sub: upload of the rANS bytes", t)
        _lib.check(lib.pcgc_rans_decode(_lib.dptr(pay_d), pay_d.numel(), _lib.dptr(off_d), _lib.dptr(self.chunks_d), self.n_chunks,
                                        _lib.dptr(self.cdfs_d), _lib.dptr(self.off_d), self.n_runs, self.cdf_total, self.max_entries, self.steps,
                                        _lib.dptr(sym_d), sym_d.numel(), _lib.dptr(status), _lib.stream()), "pcgc_rans_decode")
        _clock(timings, "sub: rANS decode kernel", t)
        return status.cpu().numpy()


def _rans_runs(level_counts):
    counts = [int(c) for c in level_counts]
    if any(c < 0 for c in counts) or any(c % 3 for c in counts[:-1]):
        raise ValueError("rANS: level_counts are symbols per level, every level but the last a multiple of 3 (whole [count, 3] rows)")
    return np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64) if counts else np.zeros(0, np.int64), counts


def rans_encode(symbols, level_counts, cdfs, steps_per_chunk=None):
    """The rANS kernels on their own.  symbols: int16, flat, sum(level_counts) of them, level after level; level_counts[l] symbols
    belong to level l and are coded with cdfs[l] (int32 [3, A_l + 1], as build_tables gives; symbol i takes the table of channel
    (index within its level) % 3); every level is cut into chunks of 64 steps_per_chunk symbols.
    -> (bytes of all chunks back to back, int64 [chunks] bytes of each chunk)"""
    import torch
    dev = _lib.require_gpu()
    bases, counts = _rans_runs(level_counts)
    sym = np.ascontiguousarray(symbols, np.int16).reshape(-1)
    if len(sym) != sum(counts) or len(cdfs) != len(counts):
        raise ValueError("rANS: %d symbols and %d tables for level counts %r" % (len(sym), len(cdfs), counts))
    for b, n, c in zip(bases, counts, cdfs):
        if n and (int(sym[b:b + n].min()) < 0 or int(sym[b:b + n].max()) > np.shape(c)[1] - 2):
            raise ValueError("rANS: a symbol outside its level's alphabet of %d" % (np.shape(c)[1] - 1))
    job = _RansJob(bases, counts, cdfs, RANS_STEPS if steps_per_chunk is None else steps_per_chunk, dev)
    return job.encode(torch.from_numpy(sym).to(dev))


def rans_decode(payload, chunk_sizes, level_counts, cdfs, steps_per_chunk=None):
    """the inverse of rans_encode -> (symbols int16 [sum(level_counts)], status int32 [chunks]: 0 = the chunk ended with every
    state at 2^16 and every word taken).  The sizes are checked against the level counts here, before the kernel runs."""
    import torch
    dev = _lib.require_gpu()
    bases, counts = _rans_runs(level_counts)
    job = _RansJob(bases, counts, cdfs, RANS_STEPS if steps_per_chunk is None else steps_per_chunk, dev)
    sizes = np.asarray(chunk_sizes, np.int64).reshape(-1)
    states = 4 * np.minimum(job.chunks[:, 2], RANS_LANES)
    if len(sizes) != job.n_chunks or (sizes & 1).any() or (sizes < states).any() or (sizes > states + 2 * job.chunks[:, 2]).any():
        raise ValueError("rANS: the chunk sizes do not fit the level counts")
    sym_d = torch.zeros(sum(counts), dtype=torch.int16, device=dev)
    status = job.decode(bytes(payload), sizes, sym_d)
    return sym_d.cpu().numpy(), status


def _check_step(qstep):
    q = float(qstep)
    if not (q > 0 and np.isfinite(q)):
        raise ValueError("colour codec: color_qstep must be a positive number (got %r)" % (qstep,))
    return q


class _Coefficients:
    """The encoder's front end, for encode_colors and the rate control alike: the colours checked, the tree (plan), the colours
    (rgb) and their transform coefficients (coef float64 [M,3], leaf order) on the device."""

    def __init__(self, points, colors, timings=None, fuse_top=True):
        import torch
        col = np.asarray(colors)
        n = len(np.asarray(points))
        if col.shape != (n, 3) or col.dtype != np.uint8:
            raise ValueError("colour codec: colors must be uint8 [%d, 3] (got %s %s)" % (n, col.dtype, col.shape))
        t = _start(timings)
        self.plan = plan = Plan(points)
        t = _clock(timings, "sort + structure", t)
        self.rgb = torch.from_numpy(np.ascontiguousarray(col)).to(plan.dev)
        self.coef = torch.empty((plan.m, 3), dtype=torch.float64, device=plan.dev)
        _lib.check(_lib.hip().pcgc_raht_load_colors(_lib.dptr(self.rgb), _lib.dptr(plan.point_of_leaf), plan.m, _lib.dptr(self.coef), _lib.stream()),
                   "pcgc_raht_load_colors")
        plan.transform(self.coef, fuse_top=fuse_top)
        _clock(timings, "transform", t)
        self.timings = timings


def _range_runs(kinds, base):
    """rows [lo, hi) of the symbol array for every run of neighbouring range-coded levels that holds symbols, one copy between
    host and device each: the whole array in version 1, usually the top of the tree alone in version 2"""
    runs = []
    for kind, levels in itertools.groupby(range(len(kinds)), kinds.__getitem__):
        levels = list(levels)
        lo, hi = int(base[levels[0]]), int(base[levels[-1] + 1])
        if kind == CODER_RANGE and hi > lo:
            runs.append((lo, hi))
    return runs


def _coder_version(coder):
    if coder not in _VERSION_OF:
        raise ValueError("colour codec: coder must be 'range' or 'rans' (got %r)" % (coder,))
    return _VERSION_OF[coder]


def encode_colors(points, colors, qstep, fuse_top=True, timings=None, coder="range"):
    """points int [M,3] unique voxels in [0, 4095], colors uint8 [M,3], qstep > 0 -> the bytes of <name>.colors.  coder: "range" =
    stream version 1 (the host's range coder), "rans" = version 2 (the large levels coded by csrc/rans.hip)"""
    qstep = _check_step(qstep)
    _coder_version(coder)
    front = _Coefficients(points, colors, timings, fuse_top)
    return _encode_coef(front.plan, front.coef, qstep, coder, timings)


def _encode_coef(plan, attr, qstep, coder, timings):
    """encode_colors from the coefficients on: quantiser, symbols, entropy coding, container (attr is left as it is, so the
    rate control codes the same coefficients at one step after another).  Nothing per symbol leaves the device except the symbols
    of the range-coded levels (all of them for coder="range"), the escapes (rare) and the raw tail; the tables come from
    per-subband sums, the rANS levels' bytes from the rANS kernels."""
    import torch
    from . import coder_ops
    lib = _lib.hip()
    m, dev, s = plan.m, plan.dev, _lib.stream()
    version = _coder_version(coder)
    counts = [int(c) for c in plan.level_counts]
    t = _start(timings)
    q = torch.empty((m, 3), dtype=torch.int32, device=dev)
    maxabs_d = torch.empty(LEVEL_SLOTS, dtype=torch.int32, device=dev)
    _lib.check(lib.pcgc_raht_quantize(_lib.dptr(attr), _lib.dptr(plan.order), _lib.dptr(plan.subband), m, qstep, _lib.dptr(q),
                                      _lib.dptr(maxabs_d), s), "pcgc_raht_quantize")
    maxabs = maxabs_d.cpu().numpy()
    n_coded = coded_levels(counts)
    base = _row_base(counts, n_coded)
    k_raw = int(base[-1])
    amax = np.minimum(maxabs[:n_coded], AMAX_CAP).astype(np.int32)
    amax_d = torch.zeros(LEVEL_SLOTS, dtype=torch.int32, device=dev)
    amax_d[:n_coded] = torch.from_numpy(amax).to(dev)
    sym = torch.empty((k_raw, 3), dtype=torch.int16, device=dev)
    _lib.check(lib.pcgc_raht_symbols(_lib.dptr(q), _lib.dptr(plan.order), _lib.dptr(plan.subband), k_raw, _lib.dptr(amax_d), _lib.dptr(sym), s),
               "pcgc_raht_symbols")
    ts = _start(timings)
    sums_d = torch.empty(SUBBANDS * 3, dtype=torch.int64, device=dev)      # one per (subband, channel), as pcgc.h says
    _lib.check(lib.pcgc_raht_abs_sums(_lib.dptr(q), _lib.dptr(plan.order), _lib.dptr(plan.subband), k_raw, _lib.dptr(amax_d), _lib.dptr(sums_d), s),
               "pcgc_raht_abs_sums")
    _clock(timings, "sub: abs sums kernel", ts)
    tail = q[k_raw:].cpu().numpy()
    esc_pos, esc_val = np.zeros(0, np.int64), np.zeros(0, np.int64)
    if (maxabs[:n_coded] > AMAX_CAP).any():              # rare: an escape is a |q| above AMAX_CAP in a level whose amax is the cap
        flat = q[:k_raw].reshape(-1)
        pos_d = torch.nonzero(flat.abs() > AMAX_CAP).reshape(-1)
        esc_pos, esc_val = pos_d.cpu().numpy(), flat[pos_d].cpu().numpy()
    t = _clock(timings, "quantise + symbols", t)
    ts = _start(timings)
    kinds = level_coders(counts, version)
    ratios = ratios_of_sums(sums_d.cpu().numpy().reshape(SUBBANDS, 3)[:n_coded], np.reshape(counts[:n_coded], (n_coded, 1)))
    cdfs = [build_tables(int(amax[l]), ratios[l]) for l in range(n_coded)]
    on_gpu = [l for l in range(n_coded) if kinds[l] == CODER_RANS]
    streams, chunk_sizes = [b""] * n_coded, [np.zeros(0, np.int64)] * n_coded
    job = _RansJob([3 * base[l] for l in on_gpu], [3 * counts[l] for l in on_gpu], [cdfs[l] for l in on_gpu], RANS_STEPS, dev)
    ts = _clock(timings, "sub: tables (host) and their upload", ts)
    payload, sizes = job.encode(sym.reshape(-1), timings)
    ts = _start(timings)
    at = 0
    for l, sz in zip(on_gpu, job.split(sizes)):
        chunk_sizes[l] = sz
        streams[l] = payload[at:at + int(sz.sum())]
        at += int(sz.sum())
    symbols = torch.empty((k_raw, 3), dtype=torch.int16)  # the host coder's: only the rows of the range-coded levels are filled
    for lo, hi in _range_runs(kinds, base):
        symbols[lo:hi].copy_(sym[lo:hi])
    symbols = symbols.numpy()
    for l in range(n_coded):
        if kinds[l] == CODER_RANGE and counts[l]:
            streams[l] = coder_ops.range_encode(symbols[base[l]:base[l + 1]], cdfs[l][None])
    data = _write(version, plan.d, m, qstep, counts, amax, ratios, streams, chunk_sizes, tail, esc_pos, esc_val)
    _clock(timings, "sub: range-coded levels (host range coder), varints, crc", ts)
    _clock(timings, "host coding", t)
    if timings is not None:
        timings["launches"] = plan.launches
    return data


def decode_colors(points, data, fuse_top=True, timings=None):
    """points: the decoded geometry the stream was coded for, data: the bytes of <name>.colors (either version) -> uint8 [M,3] in
    the order of `points`.  A stream coded for other geometry, a truncated or a corrupt one raises ValueError; everything about
    the file is checked on the host before a kernel reads it."""
    import torch
    lib = _lib.hip()
    t = _start(timings)
    plan = Plan(points)
    t = _clock(timings, "sort + structure", t)
    m, dev, s = plan.m, plan.dev, _lib.stream()
    counts = [int(c) for c in plan.level_counts]
    ts = _start(timings)
    qstep, amax, ratios, kinds, streams, chunk_sizes, symbols, patch = _read(data, plan.d, m, counts)
    ts = _clock(timings, "sub: host checks, range-coded levels (host range coder), varints, crc", ts)
    n_coded = len(amax)
    base = _row_base(counts, n_coded)
    sym = torch.empty((len(symbols), 3), dtype=torch.int16, device=dev)
    for lo, hi in _range_runs(kinds, base):
        sym[lo:hi].copy_(torch.from_numpy(symbols[lo:hi]))
    on_gpu = [l for l in range(n_coded) if kinds[l] == CODER_RANS]
    job = _RansJob([3 * base[l] for l in on_gpu], [3 * counts[l] for l in on_gpu],
                   [build_tables(int(amax[l]), ratios[l]) for l in on_gpu], RANS_STEPS, dev)
    _clock(timings, "sub: tables (host) and their upload", ts)
    if job.n_chunks:
        status = job.decode(b"".join(streams[l] for l in on_gpu), np.concatenate([chunk_sizes[l] for l in on_gpu]), sym.reshape(-1), timings)
        if status.any():
            c = int(np.flatnonzero(status)[0])
            raise ValueError(".colors: corrupt rANS chunk %d of level %d (status %d: %s)" % (
                c, on_gpu[int(job.chunks[c, 0])], int(status[c]),
                "its states do not return to 2^16" if status[c] & 1 else "words left over or missing" if status[c] & 2 else "refused"))
    t = _clock(timings, "host coding", t)
    amax_d = torch.zeros(LEVEL_SLOTS, dtype=torch.int32, device=dev)
    amax_d[:n_coded] = torch.from_numpy(amax).to(dev)
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


# ---------------------------------------------------------------------------------------------------------------- rate control
# Targets are searched over a fixed grid of steps, so that the result is a discrete, reproducible choice: notch j stands for the
# step 2^(j / 8), 0.25 .. 128 in 73 notches of about 9 %.  The chosen step goes into the header as every step does.
QSTEP_GRID_MIN = -16
QSTEP_GRID_MAX = 56
SWEEP_MAX_STEPS = 32       # candidate steps one pcgc_raht_rate_sweep launch prices
RAW_VALUE_BYTES = 3        # the estimate's price of one value of the raw tail (a zigzag varint of the top of the tree)
# BT.709 of rgb (include/pcgc.h, pcgc_color_mse): the rows give Y, U, V
_BT709 = np.array([[0.2126, 0.7152, 0.0722], [-0.1146, -0.3854, 0.5], [0.5, -0.4542, -0.0458]], np.float64)


def grid_step(j):
    """the quantiser step of notch j"""
    return 2.0 ** (j / 8.0)


def parse_target(text):
    """'psnr:38' / 'bpp:0.6' -> ("psnr", 38.0) / ("bpp", 0.6); anything else is a ValueError that says what is wanted"""
    kind, sep, number = str(text).partition(":")
    try:
        value = float(number)
    except ValueError:
        value = float("nan")
    if not sep or kind not in ("psnr", "bpp") or not np.isfinite(value) or (kind == "bpp" and value <= 0):
        raise ValueError("--color_target=%s: want psnr:<dB> (luma PSNR of the decoded colours, at least) or bpp:<bits per point> "
                         "(size of the colour file, at most; positive)" % (text,))
    return kind, value


def yuv_mse(sums6, m):
    """sse6's six sums over m points -> the mean squared errors of BT.709 Y, U and V of rgb / 255 (float64 [3]): with d the rgb
    difference and w a row of the matrix, (w . d)^2 = sum_i w_i^2 d_i^2 + 2 sum_{i<k} w_i w_k d_i d_k"""
    s = np.asarray(sums6, np.int64).astype(np.float64)
    w = _BT709
    sq = w[:, 0] ** 2 * s[0] + w[:, 1] ** 2 * s[1] + w[:, 2] ** 2 * s[2]
    mixed = w[:, 0] * w[:, 1] * s[3] + w[:, 0] * w[:, 2] * s[4] + w[:, 1] * w[:, 2] * s[5]
    return (sq + 2.0 * mixed) / (255.0 * 255.0 * float(m))


def psnr_ceiling(m):
    """The highest finite luma PSNR that m uint8 points can have, in dB: the BT.709 weights of Y are whole multiples of 0.0002
    (1063, 3576 and 361 of them, with no common factor), so a luma error that is not 0 is at least 0.0002 of a level, and the
    smallest squared error that is not 0 is that of one such point.  Above it there is only the infinite PSNR of no luma error at all."""
    return float(10.0 * np.log10(255.0 * 255.0 * float(m) / (0.0002 * 0.0002)))


def psnr_of_mse(mse):
    """dB at peak 1 (the mse is of values / 255); an mse that is not positive (rounding of an exact 0 included) is infinite"""
    return float("inf") if not mse > 0 else float(-10.0 * np.log10(mse))


def estimate_bits(abs_sums, n):
    """Bits of a subband of n values whose magnitudes add up to abs_sums, under the two-sided geometric table the encoder would
    choose for it (ratio r): a value q costs -log2((1 - r) / (1 + r)) - |q| log2(r), linear in |q|, so the sum suffices.  The
    table's 16-bit quantisation and the escapes are not priced.  Arrays broadcast; an empty subband costs nothing."""
    a = np.asarray(abs_sums, np.float64)
    n = np.asarray(n, np.float64)
    r = ratios_of_sums(abs_sums, n) / 65536.0
    return np.where(n > 0, n * -np.log2((1.0 - r) / (1.0 + r)) + a * -np.log2(r), 0.0)


def estimate_bytes(level_counts, abs_sums, coder="range"):
    """The size of the file encode_colors would write, from a sweep's sums: abs_sums int64 [K, SUBBANDS, 3] -> float64 [K].  Header,
    level rows, per coded level the bytes of estimate_bits over its three channels (rounded up), RAW_VALUE_BYTES per value of
    the raw tail and, for coder="rans", a rANS level's chunk table entries and final states."""
    version = _coder_version(coder)
    counts = np.asarray(level_counts, np.int64)
    n_coded = coded_levels(counts)
    sums = np.asarray(abs_sums, np.int64).reshape(-1, SUBBANDS, 3)[:, :n_coded]
    bits = estimate_bits(sums, counts[None, :n_coded, None]).sum(-1)                      # [K, L]
    fixed = HEADER_BYTES + _FORMATS[version][0].size * n_coded
    fixed += RAW_VALUE_BYTES * 3 * int(counts.sum() - counts[:n_coded].sum())
    per = RANS_LANES * RANS_STEPS
    for l, kind in enumerate(level_coders(counts, version)):
        if kind == CODER_RANS:
            n = 3 * int(counts[l])
            chunks = rans_chunk_count(n)
            fixed += 4 * chunks + 4 * (RANS_LANES * (chunks - 1) + min(RANS_LANES, n - per * (chunks - 1)))
    return fixed + np.ceil(bits / 8.0).sum(-1)


class _Search(_Coefficients):
    """What both targets share: the encoder's front end, and the three device-side tools that work on its coefficients — the
    sweep, the closed-loop probe and the real encode."""

    def __init__(self, points, colors, timings=None):
        import torch
        super().__init__(points, colors, timings)
        self.n_coded = coded_levels(self.plan.level_counts)
        self.k_raw = int(self.plan.level_counts[:self.n_coded].sum())
        self.work = torch.empty_like(self.coef)
        self.out = torch.empty((self.plan.m, 3), dtype=torch.uint8, device=self.plan.dev)
        self.sums6 = torch.empty(6, dtype=torch.int64, device=self.plan.dev)
        self.probes = self.real_encodes = 0

    def sweep(self, steps):
        """-> (abs_sums int64 [K, SUBBANDS, 3], max_abs int32 [K, SUBBANDS]) of the K steps, SWEEP_MAX_STEPS per launch"""
        import torch
        lib, plan = _lib.hip(), self.plan
        steps = np.ascontiguousarray(steps, np.float64).reshape(-1)
        if len(steps) == 0 or not (np.isfinite(steps) & (steps > 0)).all():
            raise ValueError("colour codec: the sweep wants at least one step, all positive numbers (got %r)" % (steps,))
        t = _start(self.timings)
        sums = torch.empty((len(steps), SUBBANDS, 3), dtype=torch.int64, device=plan.dev)
        tops = torch.empty((len(steps), SUBBANDS), dtype=torch.int32, device=plan.dev)
        for k0 in range(0, len(steps), SWEEP_MAX_STEPS):
            part = np.ascontiguousarray(steps[k0:k0 + SWEEP_MAX_STEPS])
            _lib.check(lib.pcgc_raht_rate_sweep(_lib.dptr(self.coef), _lib.dptr(plan.order), _lib.dptr(plan.subband), plan.m, self.k_raw,
                                                _lib.nptr(part), len(part), _lib.dptr(sums[k0:k0 + len(part)]), _lib.dptr(tops[k0:k0 + len(part)]),
                                                _lib.stream()), "pcgc_raht_rate_sweep")
        res = sums.cpu().numpy(), tops.cpu().numpy()
        _clock(self.timings, "rate control: sweep", t)
        return res

    def probe(self, qstep):
        """the closed loop at one step, on the device: the colours a decoder would write -> uint8 [M,3] device tensor (reused by
        the next probe), in the order of the points"""
        lib, plan, s = _lib.hip(), self.plan, _lib.stream()
        _lib.check(lib.pcgc_raht_requantize(_lib.dptr(self.coef), plan.m, _check_step(qstep), _lib.dptr(self.work), s), "pcgc_raht_requantize")
        plan.transform(self.work, inverse=True)
        _lib.check(lib.pcgc_raht_store_colors(_lib.dptr(self.work), _lib.dptr(plan.point_of_leaf), plan.m, _lib.dptr(self.out), s),
                   "pcgc_raht_store_colors")
        return self.out

    def psnr_y(self, qstep):
        """luma PSNR of the closed loop at one step: 48 bytes come back"""
        t = _start(self.timings)
        out = self.probe(qstep)
        _lib.check(_lib.hip().pcgc_color_sse6(_lib.dptr(out), _lib.dptr(self.rgb), self.plan.m, _lib.dptr(self.sums6), _lib.stream()), "pcgc_color_sse6")
        y = psnr_of_mse(yuv_mse(self.sums6.cpu().numpy(), self.plan.m)[0])
        self.probes += 1
        _clock(self.timings, "rate control: probes", t)
        return y

    def encode(self, qstep, coder):
        t = _start(self.timings)
        data = _encode_coef(self.plan, self.coef, _check_step(qstep), coder, None)
        self.real_encodes += 1
        _clock(self.timings, "rate control: real encodes", t)
        return data


def rate_sweep(points, colors, steps):
    """pcgc_raht_rate_sweep on its own: for every step, what a real encode at that step would hand its tables — abs_sums int64
    [K, SUBBANDS, 3] (per subband and channel, the sum of min(|q|, 2048) over the coded levels) and max_abs int32 [K, SUBBANDS]"""
    return _Search(points, colors).sweep(steps)


def probe_colors(points, colors, qstep):
    """the closed loop of the PSNR search on its own: uint8 [M,3], what decode_colors gives for encode_colors at that step"""
    return _Search(points, colors).probe(qstep).cpu().numpy()


def sse6(rgb_a, rgb_b):
    """two uint8 [M,3] colourings of the same points -> int64 [6]: the sums of dr^2, dg^2, db^2, dr dg, dr db, dg db (yuv_mse turns
    them into the squared error of Y, U and V)"""
    import torch
    dev = _lib.require_gpu()
    a, b = np.asarray(rgb_a), np.asarray(rgb_b)
    if a.ndim != 2 or a.shape[1] != 3 or a.shape != b.shape or a.dtype != np.uint8 or b.dtype != np.uint8 or len(a) == 0:
        raise ValueError("sse6: two uint8 arrays [M, 3] of one shape, M > 0 (got %s %s and %s %s)" % (a.dtype, a.shape, b.dtype, b.shape))
    a_d, b_d = torch.from_numpy(np.ascontiguousarray(a)).to(dev), torch.from_numpy(np.ascontiguousarray(b)).to(dev)
    out = torch.empty(6, dtype=torch.int64, device=dev)
    _lib.check(_lib.hip().pcgc_color_sse6(_lib.dptr(a_d), _lib.dptr(b_d), len(a), _lib.dptr(out), _lib.stream()), "pcgc_color_sse6")
    return out.cpu().numpy()


def encode_colors_target(points, colors, psnr=None, bpp=None, coder="range", timings=None):
    """encode_colors with the step chosen on the grid 2^(j / 8), QSTEP_GRID_MIN <= j <= QSTEP_GRID_MAX -> (data, report).
    psnr: the luma (BT.709 Y, peak 255) PSNR in dB of the decoded colours against `colors`, at least: the result has
    psnr_y(j) >= psnr and j == QSTEP_GRID_MAX or psnr_y(j + 1) < psnr.  bpp: 8 len(data) / len(points), the whole file, at most:
    len(data(j)) <= budget and j == QSTEP_GRID_MIN or len(data(j - 1)) > budget.  A target the grid cannot reach is a ValueError
    that names what it can; so is a psnr above psnr_ceiling(M), which no file of M points with any luma error at all can have
    (on uint8 colours the finest step decodes without error, so it never falls short: the ceiling is what is out of reach).
    report: j, qstep, psnr_y, bytes, bpp, probes, real_encodes (and est_bytes, j_est with bpp)."""
    if (psnr is None) == (bpp is None):
        raise ValueError("colour codec: give exactly one target, psnr (dB) or bpp (bits per point)")
    _coder_version(coder)
    target = float(psnr if bpp is None else bpp)
    if np.isnan(target) or (bpp is not None and not (target > 0)):
        raise ValueError("colour codec: the target must be a number, a bpp positive (got %r)" % (target,))
    search = _Search(points, colors, timings)
    report = {}
    if bpp is None:
        seen = {}

        def reached(j):
            if j not in seen:
                seen[j] = search.psnr_y(grid_step(j))
            return seen[j] >= target

        lo, hi = QSTEP_GRID_MIN, QSTEP_GRID_MAX
        if not reached(lo):
            raise ValueError("colour codec: a luma PSNR of %g dB is out of reach: the finest step, %g, gives %.4f dB" % (target, grid_step(lo), seen[lo]))
        if target > psnr_ceiling(search.plan.m):         # met by a file without luma error alone: not a PSNR to search for
            raise ValueError("colour codec: a luma PSNR of %g dB is out of reach: no decoded file of %d points has a finite PSNR above %.4f dB "
                             "(the finest step, %g, gives %s dB)" % (target, search.plan.m, psnr_ceiling(search.plan.m), grid_step(lo),
                                                                     "%.4f" % seen[lo] if np.isfinite(seen[lo]) else "no luma error at all, inf"))
        if reached(hi):
            lo = hi
        while hi - lo > 1:                               # reached(lo) and not reached(hi)
            mid = (lo + hi) // 2
            if reached(mid):
                lo = mid
            else:
                hi = mid
        j = lo
        data = search.encode(grid_step(j), coder)
        y = seen[j]
    else:
        budget = int(np.floor(target * search.plan.m / 8.0 + 1e-6))
        steps = [grid_step(j) for j in range(QSTEP_GRID_MIN, QSTEP_GRID_MAX + 1)]
        est = estimate_bytes(search.plan.level_counts, search.sweep(steps)[0], coder)
        fits = np.flatnonzero(est <= budget)
        j = j_est = QSTEP_GRID_MIN + int(fits[0]) if len(fits) else QSTEP_GRID_MAX
        data = search.encode(grid_step(j), coder)
        if len(data) <= budget:
            while j > QSTEP_GRID_MIN:
                finer = search.encode(grid_step(j - 1), coder)
                if len(finer) > budget:
                    break
                j, data = j - 1, finer
        else:
            while len(data) > budget:
                if j == QSTEP_GRID_MAX:
                    raise ValueError("colour codec: %g bits per point (%d bytes) is out of reach: the coarsest step, %g, takes %d bytes"
                                     % (target, budget, grid_step(j), len(data)))
                j += 1
                data = search.encode(grid_step(j), coder)
        y = search.psnr_y(grid_step(j))
        report.update(est_bytes=float(est[j - QSTEP_GRID_MIN]), j_est=j_est)
    report.update(j=j, qstep=grid_step(j), psnr_y=y, bytes=len(data), bpp=8.0 * len(data) / search.plan.m, probes=search.probes,
                  real_encodes=search.real_encodes)
    if timings is not None:
        timings["launches"] = search.plan.launches
    return data, report
