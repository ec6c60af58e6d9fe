// Stand-alone check of csrc/workspace.h (the carver every voxel-grid workspace is laid out with): g++ -std=c++17 -O1 -Wall -Werror,
// no GPU.  tests/test_workspace_host.py builds and runs it.  Exit status 0 = every layout holds.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../pcgcv1_amd/csrc/workspace.h"

using namespace pcgc;

static long g_failures = 0;
static char g_case[160];
#define CHECK(cond, ...)                                    \
  do {                                                      \
    if (!(cond)) {                                          \
      if (++g_failures <= 20) {                             \
        std::printf("FAIL %s: %s: ", g_case, #cond);        \
        std::printf(__VA_ARGS__);                           \
        std::printf("\n");                                  \
      }                                                     \
    }                                                       \
  } while (0)

struct Region { const char* at; size_t bytes; };

// A layout in the shape of the library's: three typed regions of the given counts, a nested layout of two more that takes the
// carver by value (as rank_layout does), and a last region that is rounded or not.
struct Layout {
  std::vector<Region> regions;
  size_t bytes;
};

static Carver nested(Carver c, size_t n, std::vector<Region>* out) {
  out->push_back({reinterpret_cast<const char*>(c.take<double>(n)), n * sizeof(double)});
  out->push_back({reinterpret_cast<const char*>(c.take<int64_t>(1)), sizeof(int64_t)});
  return c;
}

static Layout layout(size_t n4, size_t n1, size_t n24, size_t last, bool rounded, void* base) {
  struct Wide { double v[3]; };
  Layout l;
  Carver c(base);
  l.regions.push_back({reinterpret_cast<const char*>(c.take<int32_t>(n4)), n4 * 4});
  l.regions.push_back({reinterpret_cast<const char*>(c.take<int8_t>(n1)), n1});
  l.regions.push_back({reinterpret_cast<const char*>(c.take<Wide>(n24)), n24 * 24});
  Carver rest = nested(c, n4, &l.regions);
  const char* p = reinterpret_cast<const char*>(rounded ? rest.take<uint16_t>(last) : rest.take_unrounded<uint16_t>(last));
  l.regions.push_back({p, last * 2});
  l.bytes = rest.bytes();
  return l;
}

int main() {
  alignas(256) static char buffer[1 << 16];
  const size_t counts[] = {0, 1, 63, 64, 65, 127, 128, 129, 2500};
  long checked = 0;
  CHECK(align256(0) == 0 && align256(1) == 256 && align256(256) == 256 && align256(257) == 512, "align256");
  CHECK(align256(((size_t)1 << 40) + 1) == ((size_t)1 << 40) + 256, "align256 keeps 64 bits");
  for (size_t n4 : counts)
    for (size_t n1 : counts)
      for (size_t n24 : {(size_t)0, (size_t)11, (size_t)32})
        for (size_t last : {(size_t)0, (size_t)1, (size_t)128, (size_t)129})
          for (int rounded = 0; rounded < 2; ++rounded) {
            std::snprintf(g_case, sizeof g_case, "n4=%zu n1=%zu n24=%zu last=%zu rounded=%d", n4, n1, n24, last, rounded);
            const Layout sized = layout(n4, n1, n24, last, rounded != 0, nullptr), real = layout(n4, n1, n24, last, rounded != 0, buffer);
            ++checked;
            // a null base: null pointers, the same size
            CHECK(sized.bytes == real.bytes, "%zu != %zu", sized.bytes, real.bytes);
            for (const Region& r : sized.regions) CHECK(r.at == nullptr, "a pointer from a null base");
            CHECK(real.bytes <= sizeof buffer, "the check's own buffer is too small");
            // every region starts 256-aligned at the previous one's rounded end: back to back, so disjoint, in order
            size_t end = 0;
            for (size_t k = 0; k < real.regions.size(); ++k) {
              const Region& r = real.regions[k];
              const size_t at = (size_t)(r.at - buffer);
              CHECK(at % 256 == 0, "region %zu at %zu", k, at);
              CHECK(at == end, "region %zu at %zu, the one before it ended at %zu", k, at, end);      // a zero count: a valid position, no advance
              CHECK(at + r.bytes <= real.bytes, "region %zu ends at %zu past bytes() = %zu", k, at + r.bytes, real.bytes);
              end = at + align256(r.bytes);
            }
            // the size: the rounded end of the last region, or with the unrounded take its exact end
            const Region& tail = real.regions.back();
            const size_t tail_at = (size_t)(tail.at - buffer);
            CHECK(real.bytes == (rounded ? end : tail_at + tail.bytes), "bytes() = %zu", real.bytes);
            if (!rounded && last == 1) CHECK(real.bytes % 256 == 2, "the unrounded take rounded: %zu", real.bytes);
          }
  // the offsets of one layout written out by hand
  {
    std::snprintf(g_case, sizeof g_case, "by hand");
    const Layout l = layout(65, 1, 11, 129, false, buffer);
    const size_t want[] = {0, 512, 768, 1280, 2048, 2304};
    for (size_t k = 0; k < 6; ++k) CHECK((size_t)(l.regions[k].at - buffer) == want[k], "region %zu at %zu", k, (size_t)(l.regions[k].at - buffer));
    CHECK(l.bytes == 2304 + 258, "bytes() = %zu", l.bytes);
  }
  // Arena (net_plan.h's): offsets rounded to the asked alignment
  {
    std::snprintf(g_case, sizeof g_case, "arena");
    Arena a;
    CHECK(a.take(10, 16) == 0 && a.take(4, 4) == 12 && a.take(1, 256) == 256 && a.end == 257, "end = %zu", a.end);
  }
  std::printf("%ld layouts checked, %ld failures\n", checked, g_failures);
  return g_failures ? 1 : 0;
}
