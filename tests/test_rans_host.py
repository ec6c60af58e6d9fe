"""Colour stream version 2 on the host, no GPU: the numpy statement of the chunked 64-way interleaved rANS coder
(tests/_rans_ref.py) round trips and ends every chunk in its valid state, and the version 2 container (colorcodec.assemble_v2 /
unpack_v2, the reference's pack_v2 / unpack_v2) holds mixed range and rANS levels and names every structural error."""
import hashlib
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _rans_ref as rans                                                 # noqa: E402
from pcgcv1_amd import colorcodec as cc                                  # noqa: E402


def sizes_for(steps):
    per = 64 * steps
    return sorted({1, 2, 63, 64, 65, 127, 128, 129, per, per + 1, 2 * per + 5})


def alphabets():
    """name -> (cdf int32 [3, A + 1], symbol sampler(rng, n) -> int16 [n])"""
    def geometric(amax, scale, escapes):
        def draw(rng, n):
            q = np.rint(rng.laplace(0, scale, n)).astype(np.int64)
            s = np.where(np.abs(q) <= amax, q + amax, 2 * amax + 1)
            if escapes and n > 4:
                s[rng.integers(0, n, max(1, n // 50))] = 2 * amax + 1
            return s.astype(np.int16)
        return draw
    return {
        "two_symbols": (cc.build_tables(0, [30000, 1, 65535]), geometric(0, 0.4, False)),
        "amax3_ratio1": (cc.build_tables(3, [1, 1, 1]), geometric(3, 1.5, False)),            # every non-zero symbol has frequency 1
        "nearly_flat": (cc.build_tables(40, [65535, 65535, 65000]), geometric(40, 30.0, False)),
        "amax2047_escapes": (cc.build_tables(cc.AMAX_CAP, [64000, 65300, 50000]), geometric(cc.AMAX_CAP, 700.0, True)),
    }


ALPHABETS = alphabets()


def test_alphabets_are_what_they_claim():
    freq = np.diff(ALPHABETS["amax3_ratio1"][0], axis=1)
    assert (freq[:, [0, 1, 2, 4, 5, 6, 7]] == 1).all() and (freq[:, 3] == 65536 - 7).all()
    assert ALPHABETS["two_symbols"][0].shape == (3, 3) and ALPHABETS["amax2047_escapes"][0].shape == (3, 4097)
    flat = np.diff(ALPHABETS["nearly_flat"][0], axis=1)                  # ratio 65535: flat over the values, the escape holds both heavy tails
    assert (np.delete(flat[0], [40, 81]) == flat[0, 0]).all() and flat[0, 81] > 60000


@pytest.mark.parametrize("steps", (1, 2, 3))
@pytest.mark.parametrize("name", sorted(ALPHABETS))
def test_reference_round_trip_and_final_state(name, steps):
    cdf, draw = ALPHABETS[name]
    rng = np.random.default_rng(steps)
    for n in sizes_for(steps):
        sym = draw(rng, n)
        if name == "amax2047_escapes" and n > 4:
            assert (sym == 2 * cc.AMAX_CAP + 1).any()
        chunks = rans.encode_level(sym, cdf, steps)
        want = rans.chunk_sizes_of(n, steps)
        assert len(chunks) == len(want) == -(-n // (64 * steps))
        for c, n_c in zip(chunks, want):
            assert len(c) % 2 == 0 and 4 * min(n_c, 64) <= len(c) <= 4 * min(n_c, 64) + 2 * n_c          # at most one word per symbol
        back, status = rans.decode_level(chunks, n, cdf, steps)
        assert not status.any(), (name, steps, n, status)                 # every state back at L, every word consumed
        assert back.dtype == np.int16 and np.array_equal(back, sym), (name, steps, n)
        # a word too many or a word too few: the chunk is no longer valid (the end state is a consistency check, no checksum:
        # damaged bits may decode to other symbols and still end at L; the file's crc32c is what guards the bytes)
        if n >= 64:
            assert rans.decode_level([chunks[0] + b"\x00\x00"] + chunks[1:], n, cdf, steps)[1][0] & 2
            if len(chunks[0]) > 4 * 64:
                assert rans.decode_level([chunks[0][:-2]] + chunks[1:], n, cdf, steps)[1][0] != 0
        assert rans.decode_level([chunks[0][:3]] + chunks[1:], n, cdf, steps)[1][0] == 4
    payload, sizes = rans.encode(np.concatenate([draw(rng, 300), draw(rng, 66)]), [300, 66], [cdf, cdf], steps)
    assert len(sizes) == -(-300 // (64 * steps)) + -(-66 // (64 * steps)) and sizes.sum() == len(payload)
    assert not rans.decode(payload, sizes, [300, 66], [cdf, cdf], steps)[1].any()


def test_all_zero_chunk_under_a_peaked_table_emits_no_word():
    cdf = cc.build_tables(3, [1, 1, 1])
    for n, steps in ((64 * 3, 3), (100, 2), (1, 1)):
        chunks = rans.encode_level(np.full(n, 3, np.int16), cdf, steps)     # q = 0 is symbol amax
        assert len(chunks) == 1 and len(chunks[0]) == 4 * min(n, 64)        # the states only
        back, status = rans.decode_level(chunks, n, cdf, steps)
        assert not status.any() and (back == 3).all()


def test_channel_follows_the_index_in_the_level():
    """symbol j of a chunk takes the table of channel (first + j) % 3: three very different tables, several chunks"""
    cdf = cc.build_tables(5, [1, 30000, 65535])
    rng = np.random.default_rng(0)
    sym = np.stack([np.full(200, 5), rng.integers(3, 8, 200), rng.integers(0, 12, 200)], -1).astype(np.int16).reshape(-1)
    chunks = rans.encode_level(sym, cdf, 1)
    assert len(chunks) == 10
    back, status = rans.decode_level(chunks, len(sym), cdf, 1)
    assert not status.any() and np.array_equal(back, sym)
    rolled = cdf[[1, 2, 0]]
    back2, status2 = rans.decode_level(chunks, len(sym), rolled, 1)
    assert status2.any() or not np.array_equal(back2, sym)


def _fabricated(seed=0):
    """level counts with two chunks in one level, an empty level, the threshold T straddled exactly, range-coded small levels and
    a raw top; symbols with escapes"""
    hi = -(-rans.T // 3)                                                  # the fewest leaves whose 3 symbols each reach T
    per = 64 * rans.S
    counts = [per // 3 + 2000, 0, hi, hi - 1, 900, 300, 120, 60, 20, 10, 5, 3, 1]          # 3 d + 1 = 13: d = 4
    assert 3 * counts[2] >= rans.T > 3 * counts[3] and 3 * counts[0] > per
    d, m = 4, sum(counts)
    n_coded = cc.coded_levels(counts)
    assert n_coded == 8
    rng = np.random.default_rng(seed)
    k = sum(counts[:n_coded])
    lev = np.repeat(np.arange(n_coded), counts[:n_coded])
    q = np.rint(rng.laplace(0, 2.0, (m, 3)) * np.array([4.0, 1.0, 0.3])).astype(np.int64)
    amax = np.array([min(6, np.abs(q[:k][lev == l]).max(initial=0)) for l in range(n_coded)], np.int32)
    a = amax[lev][:, None]
    inside = np.abs(q[:k]) <= a
    sym = np.where(inside, q[:k] + a, 2 * a + 1).astype(np.int16)
    pos = np.flatnonzero(~inside.reshape(-1))
    assert len(pos) > 100
    return d, m, counts, amax, sym, q, k, pos


def test_container_v2_round_trip_and_refusals():
    d, m, counts, amax, sym, q, k, pos = _fabricated()
    data = rans.pack_v2(d, m, 2.0, counts, amax, sym, q[k:], pos, q[:k].reshape(-1)[pos])
    assert data[:4] == b"PCRA" and data[4] == 2 and struct.unpack("<d", data[16:24])[0] == 2.0
    assert cc.level_coders(counts) == [1, 0, 1, 0, 0, 0, 0, 0]
    assert cc.header_bytes(data) == cc.HEADER_BYTES + cc.LEVEL_BYTES_RANS * 8
    qstep, amax2, ratios, kinds, streams, chunk_sizes, part, patch = cc.unpack_v2(data, d, m, counts)
    assert qstep == 2.0 and np.array_equal(amax2, amax) and kinds == [1, 0, 1, 0, 0, 0, 0, 0]
    assert [len(c) for c in chunk_sizes] == [2, 0, 1, 0, 0, 0, 0, 0] and [len(s) > 0 for s in streams] == [True, False, True] + [False] * 5
    # the host half has decoded the range-coded levels and left the rANS rows for the kernel
    lo = counts[0] + counts[1] + counts[2]
    assert np.array_equal(part[lo:], sym[lo:]) and not part[:counts[0]].any()
    # the same bytes from the product's assembler, given the streams
    assert cc.assemble_v2(d, m, 2.0, counts, amax, ratios, [streams[l] if kinds[l] else _range_stream(data, counts, l) for l in range(8)],
                          chunk_sizes, q[k:], pos, q[:k].reshape(-1)[pos]) == data
    qstep, amax3, sym2, patch2 = rans.unpack_v2(data, d, m, counts)
    assert np.array_equal(sym2, sym) and np.array_equal(patch2, patch) and np.array_equal(amax3, amax)
    q2 = np.zeros_like(q)
    q2[:k] = sym2.astype(np.int64) - amax[np.repeat(np.arange(8), counts[:8])][:, None]
    q2.reshape(-1)[patch[:, 0]] = patch[:, 1]
    assert np.array_equal(q2, q)
    # tables: version 1 chooses the same (amax, ratios) for the same symbols
    v1 = cc.pack(d, m, 2.0, counts, amax, sym, q[k:], pos, q[:k].reshape(-1)[pos])
    for l in range(8):
        a, r0, r1, r2, _ = struct.unpack("<HHHHI", v1[36 + 12 * l:48 + 12 * l])
        assert (a, r0, r1, r2) == (amax[l],) + tuple(ratios[l])
    # a version 1 file still goes through the unchanged unpack, and each reader refuses the other's version by number
    assert np.array_equal(cc.unpack(v1, d, m, counts)[2], sym)
    with pytest.raises(ValueError, match="version 2, this decoder reads version 1"):
        cc.unpack(data, d, m, counts)
    with pytest.raises(ValueError, match="version 1, this decoder reads version 2"):
        cc.unpack_v2(v1, d, m, counts)
    with pytest.raises(ValueError, match="version 7"):
        cc.unpack_v2(data[:4] + b"\x07" + data[5:], d, m, counts)
    with pytest.raises(ValueError, match="magic"):
        cc.unpack_v2(b"XXXX" + data[4:], d, m, counts)
    with pytest.raises(ValueError, match="M = %d" % m):
        cc.unpack_v2(data, d, m + 1, counts)
    other = list(counts)
    other[4] -= 1
    other[5] += 1
    with pytest.raises(ValueError, match="other geometry"):
        cc.unpack_v2(data, d, m, other)
    for cut in (10, cc.HEADER_BYTES + 5, len(data) // 2, len(data) - 1):
        with pytest.raises(ValueError, match="truncated"):
            cc.unpack_v2(data[:cut], d, m, counts)
    flipped = bytearray(data)
    flipped[len(data) // 2] ^= 0x10
    with pytest.raises(ValueError, match="checksum"):
        cc.unpack_v2(bytes(flipped), d, m, counts)

    def resealed(payload):
        return data[:24] + struct.pack("<I", cc._crc(payload)) + data[28:36] + payload

    payload = data[36:]
    table = 14 * 8
    # the file ends inside the chunk table (checksum made to agree, so that the structure check is what refuses)
    with pytest.raises(ValueError, match="truncated in the chunk table of level 0"):
        cc.unpack_v2(resealed(payload[:table + 6]), d, m, counts)
    with pytest.raises(ValueError, match="truncated in the chunk table of level 2"):
        cc.unpack_v2(resealed(payload[:table + 10]), d, m, counts)
    first = struct.unpack("<I", payload[table:table + 4])[0]
    with pytest.raises(ValueError, match="odd number of word bytes"):
        cc.unpack_v2(resealed(payload[:table] + struct.pack("<I", first + 1) + payload[table + 4:]), d, m, counts)
    with pytest.raises(ValueError, match="chunks of level 0 hold"):
        cc.unpack_v2(resealed(payload[:table] + struct.pack("<I", first + 2) + payload[table + 4:]), d, m, counts)
    with pytest.raises(ValueError, match="cannot hold its states"):
        cc.unpack_v2(resealed(payload[:table] + struct.pack("<I", 8) + payload[table + 4:]), d, m, counts)
    # byte counts that overrun the payload: level 0's stream and its chunks claim more than the file holds
    row0 = struct.unpack("<HHHHHI", payload[:14])
    grown = struct.pack("<HHHHHI", *row0[:5], row0[5] + 2 * len(payload))
    second = struct.unpack("<I", payload[table + 4:table + 8])[0]
    with pytest.raises(ValueError, match="cannot hold its states|overrun the payload"):
        cc.unpack_v2(resealed(grown + payload[14:table + 4] + struct.pack("<I", second + 2 * len(payload)) + payload[table + 8:]), d, m, counts)
    row7 = struct.unpack("<HHHHHI", payload[14 * 7:14 * 8])
    with pytest.raises(ValueError, match="stream of level 7 does not fit the file .byte counts overrun the payload"):
        cc.unpack_v2(resealed(payload[:14 * 7] + struct.pack("<HHHHHI", *row7[:5], row7[5] + len(payload)) + payload[14 * 8:]), d, m, counts)
    # a level that names the coder the format does not give it
    swapped = struct.pack("<HHHHHI", *row0[:4], 0, row0[5])
    with pytest.raises(ValueError, match="names coder 0"):
        cc.unpack_v2(resealed(swapped + payload[14:]), d, m, counts)
    # a chunk whose words were damaged but whose structure is whole: the reference's decoder finds it
    at = table + 12 + 4 * 64 + 40
    damaged = resealed(payload[:at] + bytes([payload[at] ^ 0x55]) + payload[at + 1:])
    cc.unpack_v2(damaged, d, m, counts)
    with pytest.raises(ValueError, match="corrupt rANS chunk 0 of level 0"):
        rans.unpack_v2(damaged, d, m, counts)


def test_container_bytes_are_frozen():
    """Both files of _fabricated()'s input (58 032 points, 8 coded levels, two rANS levels, an empty level, escapes in levels
    with amax <= 6), by their sha256.  The digests were taken at the commit before the two writers became one (numpy 2.2.6),
    never from the code under test: no byte of a .colors file may move."""
    d, m, counts, amax, sym, q, k, pos = _fabricated()
    assert m == 58032 and cc.coded_levels(counts) == 8 and cc.level_coders(counts).count(1) == 2 and counts[1] == 0 and amax.max() <= 6
    args = (d, m, 2.0, counts, amax, sym, q[k:], pos, q[:k].reshape(-1)[pos])
    v1 = cc.pack(*args)
    assert len(v1) == 116269 and hashlib.sha256(v1).hexdigest() == "12b471ef6268b55c273636e5be6ce9e42e2646ba059fc5a1992359a317c8ead0"
    data = rans.pack_v2(*args)
    assert len(data) == 117003 and hashlib.sha256(data).hexdigest() == "67a782ad13bafa255c70448c58bc7e114a45b67a3059b110067c56993abf6a30"
    _, amax2, ratios, kinds, streams, chunk_sizes, _, _ = cc.unpack_v2(data, d, m, counts)
    again = cc.assemble_v2(d, m, 2.0, counts, amax2, ratios, [streams[l] if kinds[l] else _range_stream(data, counts, l) for l in range(8)],
                           chunk_sizes, q[k:], pos, q[:k].reshape(-1)[pos])
    assert hashlib.sha256(again).hexdigest() == "67a782ad13bafa255c70448c58bc7e114a45b67a3059b110067c56993abf6a30"


def _range_stream(data, counts, level):
    """the bytes of a range-coded level of a version 2 file"""
    payload = data[36:]
    rows = [struct.unpack("<HHHHHI", payload[14 * l:14 * l + 14]) for l in range(8)]
    at = 14 * 8 + 4 * sum(cc.rans_chunk_count(3 * counts[l]) for l in range(8) if rows[l][4] == 1)
    for l in range(level):
        at += rows[l][5]
    return payload[at:at + rows[level][5]]


def test_small_clouds_have_no_rans_level():
    """below T everything is version 1's coder under the version 2 header; a cloud that is all raw has no level at all"""
    counts = [700, 300, 0, 90, 30, 10, 1]
    d, m = 2, sum(counts)
    rng = np.random.default_rng(3)
    n_coded = cc.coded_levels(counts)
    k = sum(counts[:n_coded])
    q = rng.integers(-3, 4, (m, 3))
    amax = np.full(n_coded, 3, np.int32)
    sym = (q[:k] + 3).astype(np.int16)
    data = rans.pack_v2(d, m, 1.0, counts, amax, sym, q[k:])
    assert set(cc.level_coders(counts)) == {0} and data[4] == 2
    assert np.array_equal(rans.unpack_v2(data, d, m, counts)[2], sym)
    v1 = cc.pack(d, m, 1.0, counts, amax, sym, q[k:])
    assert len(data) == len(v1) + 2 * n_coded                             # the coder field of every row, nothing else
    tiny = rans.pack_v2(1, 3, 1.0, [1, 1, 0, 1], [], np.zeros((0, 3), np.int16), q[:3])
    assert len(tiny) == len(cc.pack(1, 3, 1.0, [1, 1, 0, 1], [], np.zeros((0, 3), np.int16), q[:3]))
    assert np.array_equal(rans.unpack_v2(tiny, 1, 3, [1, 1, 0, 1])[3][:, 1].reshape(-1, 3), q[:3])


def test_ratio_from_the_integer_sum_is_the_histograms_ratio():
    rng = np.random.default_rng(1)
    for a in (0, 1, 7, 300, cc.AMAX_CAP):
        for scale in (0.01, 0.5, 3.0, 200.0, 5000.0):
            mag = np.minimum(np.abs(np.rint(rng.laplace(0, scale, 5000)).astype(np.int64)), a + 1)
            assert cc.ratio_of_sum(int(mag.sum()), len(mag)) == cc.choose_ratio(np.bincount(mag, minlength=a + 2))
    assert cc.ratio_of_sum(0, 0) == cc.choose_ratio(np.zeros(5, np.int64)) == 1
