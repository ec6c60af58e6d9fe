"""The entropy coder of colour stream version 2 in numpy: chunked, 64-way interleaved rANS.  This file is the definition
(DESIGN.md 7d); csrc/rans.hip and pcgcv1_amd/colorcodec.py must give the same bytes.

Coder: state uint32, lower bound L = 2^16, 16-bit little-endian renormalisation words, 16-bit tables (colorcodec.build_tables:
totals 65536, every frequency >= 1).  Encoding symbol (start, freq): if x >= freq << 16, emit x & 0xFFFF and x >>= 16; then
x = ((x // freq) << 16) + (x % freq) + start.  Decoding: slot = x & 0xFFFF, s with cdf[s] <= slot < cdf[s + 1],
x = freq * (x >> 16) + slot - start; if x < L, x = (x << 16) | next word.

Chunk: n symbols, 1 <= n <= 64 steps; symbol j belongs to lane j % 64 and step j // 64; its table is the level's table of channel
(first + j) % 3, first = the chunk's first index in the level's flat [count, 3] symbol array.  The encoder starts every lane at L,
walks the steps from last to first and within a step the lanes from highest to lowest.  The chunk's bytes: the min(n, 64) final
states (uint32, lane ascending), then the words in the reverse of emission order, which is the order the decoder (steps
ascending, lanes ascending within a step, every renormalising lane takes the next word) reads them in.  A chunk is valid only if
at the end every state is L again and every word has been taken.

Level: ceil(3 count / (64 S)) chunks of 64 S symbols, the last one shorter; a level with fewer than T symbols keeps version 1's
range stream.  S and T are the format's constants (colorcodec.RANS_STEPS, RANS_MIN_SYMBOLS).

The loops below run over the steps; every step is one numpy expression over all lanes of all chunks of the level."""
import struct

import numpy as np

from pcgcv1_amd import colorcodec as cc

L = 1 << 16
LANES = 64
S = 2048
T = 16384


def chunk_sizes_of(n, steps):
    """symbols per chunk of a level of n symbols"""
    per = LANES * steps
    return [min(per, n - f) for f in range(0, n, per)]


def _grid(n, steps):
    """index of the symbol at [chunk, step, lane] in the level's flat array, and which of them exist"""
    per = LANES * steps
    n_chunks = -(-n // per)
    used = steps if n_chunks > 1 else -(-n // LANES)                      # a lone short chunk: the steps past its end hold nothing
    idx = np.arange(n_chunks * used * LANES, dtype=np.int64).reshape(n_chunks, used, LANES)
    return idx, idx < n


def encode_level(symbols, cdf, steps=S):
    """symbols: the level's flat array (row major [count, 3]); cdf int32 [3, A + 1] -> one bytes object per chunk"""
    sym = np.asarray(symbols, np.int64).reshape(-1)
    n = len(sym)
    if n == 0:
        return []
    cdf = np.asarray(cdf, np.int64)
    assert sym.min() >= 0 and sym.max() <= cdf.shape[1] - 2
    idx, valid = _grid(n, steps)
    s = np.where(valid, sym[np.minimum(idx, n - 1)], 0)
    start = cdf[idx % 3, s]
    freq = np.where(valid, cdf[idx % 3, s + 1] - start, 1)
    x = np.full((idx.shape[0], LANES), L, np.uint64)
    words = np.zeros(idx.shape, np.uint16)
    emitted = np.zeros(idx.shape, bool)
    for t in range(idx.shape[1] - 1, -1, -1):
        f, b, v = freq[:, t].astype(np.uint64), start[:, t].astype(np.uint64), valid[:, t]
        emit = v & (x >= (f << np.uint64(16)))
        words[:, t] = np.where(emit, x & np.uint64(0xFFFF), 0)
        emitted[:, t] = emit
        x = np.where(emit, x >> np.uint64(16), x)
        x = np.where(v, ((x // f) << np.uint64(16)) + (x % f) + b, x)
    assert (x < (1 << 32)).all()
    out = []
    for c, n_c in enumerate(chunk_sizes_of(n, steps)):
        # row-major over [step, lane] = steps ascending, lanes ascending: the reverse of the order of emission
        out.append(x[c, :min(n_c, LANES)].astype("<u4").tobytes() + words[c][emitted[c]].astype("<u2").tobytes())
    return out


def decode_level(chunks, n, cdf, steps=S):
    """chunks: one bytes object per chunk of a level of n symbols -> (symbols int16 [n], status int32 [chunks]); status 0 = valid,
    bit 0 = a state did not return to L, bit 1 = words left over or missing, 4 = the bytes cannot hold the chunk's states"""
    cdf = np.asarray(cdf, np.int64)
    sizes = chunk_sizes_of(n, steps)
    assert len(chunks) == len(sizes)
    if n == 0:
        return np.zeros(0, np.int16), np.zeros(0, np.int32)
    idx, valid = _grid(n, steps)
    n_chunks = len(sizes)
    status = np.zeros(n_chunks, np.int32)
    x = np.full((n_chunks, LANES), L, np.uint64)
    n_words = np.zeros(n_chunks, np.int64)
    stream = np.zeros((n_chunks, LANES * steps + LANES), np.uint64)          # words past a chunk's end read as 0
    for c, (data, n_c) in enumerate(zip(chunks, sizes)):
        ns = min(n_c, LANES)
        if len(data) < 4 * ns or len(data) % 2 or len(data) > 4 * ns + 2 * n_c:
            status[c] = 4
            continue
        x[c, :ns] = np.frombuffer(data, "<u4", ns)
        w = np.frombuffer(data, "<u2", offset=4 * ns)
        n_words[c] = len(w)
        stream[c, :len(w)] = w
    rd = np.zeros(n_chunks, np.int64)
    out = np.zeros(idx.shape, np.int64)
    rows = np.arange(n_chunks)[:, None]
    for t in range(idx.shape[1]):
        v, ch = valid[:, t], idx[:, t] % 3
        slot = (x & np.uint64(0xFFFF)).astype(np.int64)
        s = np.zeros(slot.shape, np.int64)
        for k in range(3):
            s = np.where(ch == k, np.searchsorted(cdf[k], slot, side="right") - 1, s)
        s = np.clip(s, 0, cdf.shape[1] - 2)
        start, freq = cdf[ch, s], cdf[ch, s + 1] - cdf[ch, s]
        nx = (freq.astype(np.uint64) * (x >> np.uint64(16)) + (slot - start).astype(np.uint64)) & np.uint64(0xFFFFFFFF)
        x = np.where(v, nx, x)
        out[:, t] = np.where(v, s, 0)
        need = v & (x < L)
        pos = rd[:, None] + np.cumsum(need, 1) - need
        word = np.where(pos < n_words[:, None], stream[rows, np.minimum(pos, stream.shape[1] - 1)], 0)
        x = np.where(need, ((x << np.uint64(16)) | word) & np.uint64(0xFFFFFFFF), x)
        rd += need.sum(1)
    bad = (x != L).any(1).astype(np.int32) | (2 * (rd != n_words)).astype(np.int32)
    status = np.where(status == 0, bad, status)
    return out.reshape(-1)[:n].astype(np.int16), status


def encode(symbols, level_counts, cdfs, steps=S):
    """what colorcodec.rans_encode returns: level_counts symbols per level -> (all chunks back to back, bytes per chunk)"""
    sym = np.asarray(symbols).reshape(-1)
    chunks, at = [], 0
    for n, cdf in zip(level_counts, cdfs):
        chunks += encode_level(sym[at:at + n], cdf, steps)
        at += n
    return b"".join(chunks), np.array([len(c) for c in chunks], np.int64)


def decode(payload, chunk_bytes, level_counts, cdfs, steps=S):
    sym, status, at, k = [], [], 0, 0
    for n, cdf in zip(level_counts, cdfs):
        n_c = len(chunk_sizes_of(n, steps))
        parts = []
        for b in chunk_bytes[k:k + n_c]:
            parts.append(payload[at:at + int(b)])
            at += int(b)
        k += n_c
        s, st = decode_level(parts, n, cdf, steps)
        sym.append(s)
        status.append(st)
    return np.concatenate(sym) if sym else np.zeros(0, np.int16), np.concatenate(status) if status else np.zeros(0, np.int32)


# ---------------------------------------------------------------------------------------------------------------- the file
def pack_v2(d, m, qstep, level_counts, amax, symbols, tail, esc_pos=(), esc_val=()):
    """colorcodec.pack's arguments -> the bytes of the version 2 file.  The tables are chosen as version 1 chooses them (from the
    histogram of the symbols), the rows and the chunk table are laid out here, not by the code under test."""
    from pcgcv1_amd import coder_ops
    counts = [int(c) for c in level_counts]
    n_coded = cc.coded_levels(counts)
    symbols = np.ascontiguousarray(symbols, np.int16).reshape(-1, 3)
    tail = np.asarray(tail, np.int64).reshape(-1, 3)
    assert len(counts) == 3 * d + 1 and sum(counts) == m and len(symbols) == sum(counts[:n_coded]) and len(amax) == n_coded
    rows, chunk_table, streams = [], [], []
    at = 0
    for l in range(n_coded):
        s = symbols[at:at + counts[l]]
        at += counts[l]
        a = int(amax[l])
        ratios = [cc.choose_ratio(np.bincount(np.abs(s[:, c].astype(np.int64) - a).clip(max=a + 1), minlength=a + 2)) for c in range(3)]
        cdf = cc.build_tables(a, ratios)
        if 3 * counts[l] >= T:
            chunks = encode_level(s.reshape(-1), cdf, S)
            chunk_table += [struct.pack("<I", len(c)) for c in chunks]
            stream, kind = b"".join(chunks), 1
        else:
            stream, kind = (coder_ops.range_encode(s, cdf[None]) if len(s) else b""), 0
        rows.append(struct.pack("<HHHHHI", a, ratios[0], ratios[1], ratios[2], kind, len(stream)))
        streams.append(stream)
    esc_pos = np.asarray(esc_pos, np.int64).reshape(-1)
    esc = np.stack([np.diff(esc_pos, prepend=0), cc._zigzag(esc_val)], -1) if len(esc_pos) else np.zeros((0, 2), np.int64)
    payload = b"".join(rows) + b"".join(chunk_table) + b"".join(streams) + cc._put_varints(esc) + cc._put_varints(cc._zigzag(tail))
    head = b"PCRA" + struct.pack("<BBHQdIII", 2, d, n_coded, m, float(qstep), cc._crc(payload), len(esc_pos), cc._geometry_crc(counts))
    return head + payload


def unpack_v2(data, d, m, level_counts):
    """what colorcodec.unpack returns for a version 1 file: (qstep, amax, symbols int16 [K,3], patch).  Only the rANS chunks are
    decoded here, by the numpy rule.  The container itself is read by colorcodec.unpack_v2, the product's host half, so this is no
    independent reader of the layout: the independent statement of the layout is pack_v2 above, and the refusals of unpack_v2 are
    tested directly with hand-made bytes (tests/test_rans_host.py)."""
    counts = [int(c) for c in level_counts]
    qstep, amax, ratios, kinds, streams, chunk_sizes, symbols, patch = cc.unpack_v2(data, d, m, counts)
    at = 0
    for l in range(len(amax)):
        if kinds[l] == 1:
            parts, b = [], 0
            for size in chunk_sizes[l]:
                parts.append(streams[l][b:b + int(size)])
                b += int(size)
            sym, status = decode_level(parts, 3 * counts[l], cc.build_tables(int(amax[l]), ratios[l]), S)
            if status.any():
                raise ValueError(".colors: corrupt rANS chunk %d of level %d (status %d)" % (int(np.flatnonzero(status)[0]), l, int(status.max())))
            symbols[at:at + counts[l]] = sym.reshape(-1, 3)
        at += counts[l]
    return qstep, amax, symbols, patch
