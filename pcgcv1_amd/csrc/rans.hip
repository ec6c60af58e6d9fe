// Chunked, 64-way interleaved rANS for the colour stream, version 2 (gfx950).  pcgcv1_amd/colorcodec.py holds the container,
// DESIGN.md §7d the rule; tests/_rans_ref.py is its definition in numpy and these kernels must give the same bytes.
//
// One wavefront codes one chunk; lane i owns rANS lane i, symbol j of the chunk belongs to lane j % 64 and step j / 64.  The
// three tables of the chunk's level (channel = global symbol index % 3) are staged in LDS once per chunk.  State uint32, lower
// bound 2^16, 16-bit renormalisation words, 16-bit precision: a symbol emits at most one word, so the words of a step are
// placed with one wave ballot and a lane prefix count.
//
// The encoder walks the steps from last to first and fills its slot's word area from the BACK: within a step the lanes'
// words lie in ascending lane order, the steps in ascending order, which is exactly the order in which the decoder (steps
// ascending, lanes ascending) takes them.  The decoder keeps a 128-word window of the stream in registers (two words per lane,
// a third in flight) and hands each renormalising lane its word with a lane shuffle, so no step waits for global memory; its
// symbol search starts from a 256-bucket hint table in LDS (slot >> 8 -> first candidate symbol) and finishes with a binary
// search between two neighbouring hints, one or two LDS reads for a peaked table.
//
// Every index that comes from the chunk descriptors, the offsets or the stream is checked against the buffers' sizes before
// it is used: a bad descriptor or a bad stream ends in a status, never in an access outside the chunk's own bytes.
#include <algorithm>
#include "common.h"
#include "workspace.h"

namespace pcgc {
namespace {

constexpr uint32_t kLow = 1u << 16;              // the state's lower bound L
constexpr int kLanes = 64;
constexpr int kStateBytes = kLanes * 4;          // a chunk's slot: 256 bytes of states, then 64 * steps words
constexpr int kMaxEntries = 2 * 2047 + 4;        // cdf entries per channel at AMAX_CAP: 2 amax + 2 symbols + 1
constexpr int kHint = 256;                       // hint buckets per channel (slot >> 8); + 1 closing entry
constexpr int kMaxSteps = 1 << 20;
constexpr int kBatch = 8;                        // steps whose symbols the encoder loads ahead

extern __shared__ __attribute__((aligned(16))) char smem[];

struct Chunk {
  int64_t first;      // index of the chunk's first symbol in the whole symbol array
  int n;              // symbols
  int entries;        // cdf entries per channel of its level (symbols + 1)
  int64_t table;      // offset of the level's three tables in cdfs
};

// the descriptor of chunk c, checked against everything the kernels index with it (wave-uniform)
__device__ __forceinline__ bool read_chunk(const int64_t* chunks, int64_t c, const int64_t* cdf_off, int n_levels, int64_t cdf_total,
                                           int64_t n_symbols, int steps, int max_entries, Chunk* out) {
  const int64_t level = chunks[c * 3], first = chunks[c * 3 + 1], n = chunks[c * 3 + 2];
  if (level < 0 || level >= n_levels || n < 1 || n > (int64_t)kLanes * steps || first < 0 || first > n_symbols - n) return false;
  const int64_t t0 = cdf_off[level], t1 = cdf_off[level + 1];
  if (t0 < 0 || t1 > cdf_total || t1 < t0 || (t1 - t0) % 3 != 0) return false;
  const int64_t entries = (t1 - t0) / 3;
  if (entries < 3 || entries > max_entries) return false;
  out->first = first;
  out->n = (int)n;
  out->entries = (int)entries;
  out->table = t0;
  return true;
}

__device__ __forceinline__ void stage_tables(const int32_t* cdfs, const Chunk& ch, int32_t* tab, int lane) {
  for (int i = lane; i < 3 * ch.entries; i += kLanes) tab[i] = cdfs[ch.table + i];
  __syncthreads();
}

// the symbol s of table t (entries e) with t[s] <= slot < t[s + 1], searched in [lo, hi): t[lo] <= slot < t[hi]
__device__ __forceinline__ int find_symbol(const int32_t* t, int lo, int hi, int slot) {
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (t[mid] <= slot) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ void __launch_bounds__(kLanes) encode_kernel(const int16_t* sym, int64_t n_symbols, const int64_t* chunks, const int32_t* cdfs,
                                                         const int64_t* cdf_off, int64_t cdf_total, int n_levels, int steps, int max_entries,
                                                         char* slots, int64_t slot_bytes, int32_t* chunk_bytes) {
  int32_t* tab = reinterpret_cast<int32_t*>(smem);
  const int lane = threadIdx.x;
  const int64_t c = blockIdx.x;
  Chunk ch;
  if (!read_chunk(chunks, c, cdf_off, n_levels, cdf_total, n_symbols, steps, max_entries, &ch)) {
    if (lane == 0) chunk_bytes[c] = -1;
    return;
  }
  stage_tables(cdfs, ch, tab, lane);
  char* slot = slots + c * slot_bytes;
  uint16_t* words = reinterpret_cast<uint16_t*>(slot + kStateBytes);          // 64 * steps of them; filled from the back
  int end = kLanes * steps;
  uint32_t x = kLow;
  const int nsteps = (ch.n + kLanes - 1) / kLanes;
  const int e = ch.entries;
  for (int t1 = nsteps; t1 > 0; t1 -= kBatch) {                               // steps t1 - 1 down to max(t1 - kBatch, 0)
    int s[kBatch];
#pragma unroll
    for (int b = 0; b < kBatch; ++b) {
      const int j = (t1 - 1 - b) * kLanes + lane;
      s[b] = (t1 - 1 - b >= 0 && j < ch.n) ? sym[ch.first + j] : -1;
    }
#pragma unroll
    for (int b = 0; b < kBatch; ++b) {
      if (t1 - 1 - b < 0) break;                                               // wave-uniform
      const int j = (t1 - 1 - b) * kLanes + lane;
      bool emit = false;
      uint32_t w = 0;
      if (j < ch.n) {
        const int k = min(max(s[b], 0), e - 2);                               // a symbol outside the alphabet cannot leave the table
        const int32_t* t = tab + (int)((ch.first + j) % 3) * e;
        const uint32_t start = (uint32_t)t[k];
        const uint32_t freq = (uint32_t)min(max(t[k + 1] - t[k], 1), 65535);
        if (x >= (freq << 16)) { emit = true; w = x & 0xFFFFu; x >>= 16; }
        x = ((x / freq) << 16) + (x % freq) + start;
      }
      const unsigned long long mask = __ballot(emit);
      end -= __popcll(mask);
      if (emit) words[end + __popcll(mask & ((1ull << lane) - 1ull))] = (uint16_t)w;
    }
  }
  const int ns = min(ch.n, kLanes);
  if (lane < ns) reinterpret_cast<uint32_t*>(slot)[lane] = x;
  if (lane == 0) chunk_bytes[c] = 4 * ns + 2 * (kLanes * steps - end);
}

// offsets[c] = bytes of the chunks before c (a refused chunk counts 0 bytes), offsets[n] = all of them.  One workgroup: the
// codec has tens of chunks (24 for the 828 k-point bench cloud at S = 2048) and a test a few hundred; each thread walks n / 256 of them, so
// the launch stays short up to some 10^5 chunks, far beyond any steps_per_chunk the codec would use.
__global__ void __launch_bounds__(256) scan_kernel(const int32_t* chunk_bytes, int64_t n, int64_t* offsets) {
  __shared__ int64_t part[256];
  const int64_t per = (n + 255) / 256;
  const int64_t c0 = std::min<int64_t>(n, (int64_t)threadIdx.x * per), c1 = std::min<int64_t>(n, c0 + per);
  int64_t s = 0;
  for (int64_t c = c0; c < c1; ++c) s += std::max(chunk_bytes[c], 0);
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t acc = 0;
    for (int i = 0; i < 256; ++i) { const int64_t v = part[i]; part[i] = acc; acc += v; }
    offsets[n] = acc;
  }
  __syncthreads();
  int64_t acc = part[threadIdx.x];
  for (int64_t c = c0; c < c1; ++c) { offsets[c] = acc; acc += std::max(chunk_bytes[c], 0); }
}

// the chunk's states and words, from its slot to out + offsets[c]
__global__ void __launch_bounds__(256) pack_kernel(const char* slots, int64_t slot_bytes, int steps, const int32_t* chunk_bytes,
                                                   const int64_t* chunks, const int64_t* offsets, uint16_t* out, int64_t out_bytes) {
  const int64_t c = blockIdx.x;
  const int bytes = chunk_bytes[c];
  const int64_t at = offsets[c];
  const int64_t n = chunks[c * 3 + 2];
  if (bytes <= 0 || n < 1 || at < 0 || at + bytes > out_bytes) return;
  const int half_states = 2 * (int)std::min<int64_t>(n, kLanes);                   // the states as 16-bit halves
  const int total = bytes / 2, nwords = total - half_states;
  if (nwords < 0 || nwords > kLanes * steps) return;
  const uint16_t* slot = reinterpret_cast<const uint16_t*>(slots + c * slot_bytes);
  const uint16_t* words = slot + kStateBytes / 2 + (kLanes * steps - nwords);
  uint16_t* dst = out + at / 2;
  for (int i = threadIdx.x; i < total; i += 256) dst[i] = i < half_states ? slot[i] : words[i - half_states];
}

__global__ void __launch_bounds__(kLanes) decode_kernel(const uint16_t* payload, int64_t payload_bytes, const int64_t* offsets,
                                                         const int64_t* chunks, const int32_t* cdfs, const int64_t* cdf_off, int64_t cdf_total,
                                                         int n_levels, int steps, int max_entries, int16_t* sym, int64_t n_symbols,
                                                         int32_t* status) {
  int32_t* tab = reinterpret_cast<int32_t*>(smem);
  const int lane = threadIdx.x;
  const int64_t c = blockIdx.x;
  Chunk ch;
  if (!read_chunk(chunks, c, cdf_off, n_levels, cdf_total, n_symbols, steps, max_entries, &ch)) {
    if (lane == 0) status[c] = 4;
    return;
  }
  const int ns = min(ch.n, kLanes);
  const int64_t b0 = offsets[c], b1 = offsets[c + 1];
  if (b0 < 0 || b1 > payload_bytes || ((b0 | b1) & 1) || b1 - b0 < 4 * ns || b1 - b0 > 4 * ns + 2 * (int64_t)ch.n) {
    if (lane == 0) status[c] = 4;                                             // the chunk's bytes cannot hold its states and at most n words
    return;
  }
  const int e = ch.entries;
  int32_t* hint = tab + 3 * e;                                                // [3][kHint + 1]
  stage_tables(cdfs, ch, tab, lane);
  for (int i = lane; i < 3 * (kHint + 1); i += kLanes) {
    const int chn = i / (kHint + 1), k = i % (kHint + 1);
    hint[i] = k == kHint ? e - 2 : find_symbol(tab + chn * e, 0, e - 1, k << 8);
  }
  __syncthreads();
  const uint16_t* st = payload + b0 / 2;
  const uint16_t* words = st + 2 * ns;
  const int nwords = (int)((b1 - b0) / 2) - 2 * ns;
  uint32_t x = lane < ns ? (uint32_t)st[2 * lane] | ((uint32_t)st[2 * lane + 1] << 16) : kLow;
  // the window: w0 = words[wb + lane], w1 = words[wb + 64 + lane], w2 = words[wb + 128 + lane] on its way; 0 past the chunk's end
  auto word_at = [&](int i) -> uint32_t { return i < nwords ? (uint32_t)words[i] : 0u; };
  int wb = 0, rd = 0;
  uint32_t w0 = word_at(lane), w1 = word_at(kLanes + lane), w2 = word_at(2 * kLanes + lane);
  const int nsteps = (ch.n + kLanes - 1) / kLanes;
  for (int t = 0; t < nsteps; ++t) {
    const int j = t * kLanes + lane;
    bool need = false;
    if (j < ch.n) {
      const int32_t* tb = tab + (int)((ch.first + j) % 3) * e;
      const int32_t* hb = hint + (int)((ch.first + j) % 3) * (kHint + 1);
      const int slot = (int)(x & 0xFFFFu);
      const int lo = min(max(hb[slot >> 8], 0), e - 2), hi = min(max(hb[(slot >> 8) + 1] + 1, lo + 1), e - 1);
      const int s = find_symbol(tb, lo, hi, slot);
      const uint32_t start = (uint32_t)tb[s], freq = (uint32_t)(tb[s + 1] - tb[s]);
      x = freq * (x >> 16) + (uint32_t)slot - start;
      sym[ch.first + j] = (int16_t)s;
      need = x < kLow;
    }
    const unsigned long long mask = __ballot(need);
    const int p = rd - wb + __popcll(mask & ((1ull << lane) - 1ull));          // < 128: rd - wb < 64
    const uint32_t v0 = __shfl(w0, p & 63), v1 = __shfl(w1, p & 63);
    if (need) x = (x << 16) | (p < kLanes ? v0 : v1);
    rd += __popcll(mask);
    if (rd - wb >= kLanes) {
      wb += kLanes;
      w0 = w1;
      w1 = w2;
      w2 = word_at(wb + 2 * kLanes + lane);
    }
  }
  const bool states_bad = __ballot(x != kLow) != 0ull;
  if (lane == 0) status[c] = (states_bad ? 1 : 0) | (rd != nwords ? 2 : 0);
}

// workspace of pcgc_rans_encode: one int32 byte count per chunk, then one slot per chunk (states + 64 * steps words)
struct RansBuffers { int32_t* chunk_bytes; char* slots; int64_t slot_bytes; size_t bytes; };

RansBuffers rans_layout(int64_t n_chunks, int steps_per_chunk, void* workspace) {
  Carver c(workspace);
  RansBuffers b;
  b.slot_bytes = kStateBytes + 2 * (int64_t)kLanes * steps_per_chunk;
  b.chunk_bytes = c.take<int32_t>((size_t)n_chunks);
  b.slots = c.take_unrounded<char>((size_t)n_chunks * b.slot_bytes);
  b.bytes = c.bytes();
  return b;
}

}  // namespace
}  // namespace pcgc

using namespace pcgc;

extern "C" {

size_t pcgc_rans_workspace_bytes(int64_t n_chunks, int steps_per_chunk) {
  if (n_chunks <= 0 || n_chunks > 0x7FFFFFFF || steps_per_chunk < 1 || steps_per_chunk > kMaxSteps) return 0;
  return rans_layout(n_chunks, steps_per_chunk, nullptr).bytes;
}

static bool tables_fit(int max_entries) { return max_entries >= 3 && max_entries <= kMaxEntries; }

int pcgc_rans_encode(const int16_t* symbols, int64_t n_symbols, const int64_t* chunks, int64_t n_chunks, const int32_t* cdfs,
                     const int64_t* cdf_offsets, int n_levels, int64_t cdf_total, int max_entries, int steps_per_chunk, void* out,
                     int64_t out_bytes, int64_t* offsets, void* workspace, size_t workspace_bytes, pcgc_stream_t stream) {
  PCGC_REQUIRE(symbols && chunks && cdfs && cdf_offsets && out && offsets && workspace && n_symbols > 0 && n_chunks > 0 &&
               n_chunks <= 0x7FFFFFFF && n_levels > 0 && cdf_total > 0 && out_bytes >= 0 && steps_per_chunk >= 1 &&
               steps_per_chunk <= kMaxSteps, "pcgc_rans_encode: bad arguments");
  PCGC_REQUIRE(tables_fit(max_entries), "pcgc_rans_encode: tables of %d entries (at most %d fit)", max_entries, kMaxEntries);
  const RansBuffers b = rans_layout(n_chunks, steps_per_chunk, workspace);
  PCGC_REQUIRE(workspace_bytes >= b.bytes, "pcgc_rans_encode: workspace too small");
  PCGC_REQUIRE(((uintptr_t)out & 1) == 0, "pcgc_rans_encode: the output buffer must be 2-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(encode_kernel, dim3((unsigned)n_chunks), dim3(kLanes), (size_t)3 * max_entries * sizeof(int32_t), s, symbols, n_symbols,
                     chunks, cdfs, cdf_offsets, cdf_total, n_levels, steps_per_chunk, max_entries, b.slots, b.slot_bytes, b.chunk_bytes);
  hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(256), 0, s, b.chunk_bytes, n_chunks, offsets);
  hipLaunchKernelGGL(pack_kernel, dim3((unsigned)n_chunks), dim3(256), 0, s, b.slots, b.slot_bytes, steps_per_chunk, b.chunk_bytes, chunks,
                     offsets, static_cast<uint16_t*>(out), out_bytes);
  return launch_ok("rans encode kernels");
}

int pcgc_rans_decode(const void* payload, int64_t payload_bytes, const int64_t* offsets, const int64_t* chunks, int64_t n_chunks,
                     const int32_t* cdfs, const int64_t* cdf_offsets, int n_levels, int64_t cdf_total, int max_entries,
                     int steps_per_chunk, int16_t* symbols, int64_t n_symbols, int32_t* status, pcgc_stream_t stream) {
  PCGC_REQUIRE(payload && offsets && chunks && cdfs && cdf_offsets && symbols && status && payload_bytes > 0 && n_symbols > 0 &&
               n_chunks > 0 && n_chunks <= 0x7FFFFFFF && n_levels > 0 && cdf_total > 0 && steps_per_chunk >= 1 &&
               steps_per_chunk <= kMaxSteps, "pcgc_rans_decode: bad arguments");
  PCGC_REQUIRE(tables_fit(max_entries), "pcgc_rans_decode: tables of %d entries (at most %d fit)", max_entries, kMaxEntries);
  PCGC_REQUIRE(((uintptr_t)payload & 1) == 0, "pcgc_rans_decode: the payload must be 2-byte aligned");
  const size_t lds = ((size_t)3 * max_entries + 3 * (kHint + 1)) * sizeof(int32_t);
  hipLaunchKernelGGL(decode_kernel, dim3((unsigned)n_chunks), dim3(kLanes), lds, (hipStream_t)stream, static_cast<const uint16_t*>(payload),
                     payload_bytes, offsets, chunks, cdfs, cdf_offsets, cdf_total, n_levels, steps_per_chunk, max_entries, symbols, n_symbols,
                     status);
  return launch_ok("rans decode kernel");
}

}  // extern "C"
