// test_host_layout.cpp -- the region declarations of a one-problem host call (HostLayout, csrc/host_internal.h) without a device:
// every offset is a 256-byte multiple, the groups are contiguous in the order input, scratch, output, a zero-byte region takes no
// space, and the totals are the sum of the padded sizes.  The offsets index a real buffer of total() bytes, so that the sanitizers
// see every region written to its last byte.
#include <stdio.h>
#include <string.h>

#include <vector>

#define HOST_LAYOUT_ONLY
#include "../../refactored_orb_slam2_amd/csrc/host_internal.h"

static int failures = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);     \
      failures++;                                                    \
    }                                                                \
  } while (0)

static size_t pad(size_t b) { return (b + 255) / 256 * 256; }

struct Region {
  int group;
  size_t bytes, off;
};

// declares `sizes` group by group and checks the whole layout against the sums
static void run(const std::vector<size_t>& in, const std::vector<size_t>& scratch, const std::vector<size_t>& out) {
  HostLayout L;
  std::vector<Region> regions;
  size_t sum[3] = {0, 0, 0};
  for (size_t b : in) { regions.push_back({0, b, L.in(b)}); sum[0] += pad(b); }
  for (size_t b : scratch) { regions.push_back({1, b, L.scratch(b)}); sum[1] += pad(b); }
  for (size_t b : out) { regions.push_back({2, b, L.out(b)}); sum[2] += pad(b); }
  CHECK(L.in_end() == sum[0]);
  CHECK(L.out_begin() == sum[0] + sum[1]);
  CHECK(L.total() == sum[0] + sum[1] + sum[2]);
  CHECK(L.out_bytes() == sum[2]);
  const size_t lo[3] = {0, L.in_end(), L.out_begin()}, hi[3] = {L.in_end(), L.out_begin(), L.total()};
  std::vector<unsigned char> block(L.total() + 1, 0);   // + 1: an empty layout still has an address
  size_t next = 0;
  for (size_t i = 0; i < regions.size(); i++) {
    const Region& r = regions[i];
    CHECK(r.off % 256 == 0);
    CHECK(r.off == next);                                    // contiguous, in declaration order
    CHECK(r.off >= lo[r.group] && r.off + pad(r.bytes) <= hi[r.group]);
    next = r.off + pad(r.bytes);
    if (r.bytes == 0) CHECK(next == r.off);                  // a zero-byte region takes no space
    if (r.bytes) memset(block.data() + r.off, (int)(i + 1), r.bytes);
  }
  CHECK(next == L.total());
  for (size_t i = 0; i < regions.size(); i++)                // no region overwrote another
    for (size_t k = 0; k < regions[i].bytes; k++)
      if (block[regions[i].off + k] != (unsigned char)(i + 1)) { CHECK(!"regions overlap"); break; }
}

int main() {
  run({}, {}, {});
  run({1}, {}, {1});
  run({16, 0, 255, 256, 257}, {0, 0}, {4});
  run({65, 65 * 4}, {65 * 4, 65}, {256, 63 * 4, 0, 64 * 4});   // byte flags that end off a 4-byte boundary in front of int32 regions
  run({0, 0}, {1000}, {0});
  run({3}, {}, {});
  run({}, {7}, {});
  run({}, {}, {9});
  run({(size_t)1 << 20, 12345}, {(size_t)3 << 20}, {800 * 1024 + 1});
  HostLayout L;                                               // an offset is where the previous region's padded end is
  CHECK(L.in(1) == 0 && L.in(0) == 256 && L.in(256) == 256 && L.scratch(257) == 512 && L.out(0) == 1024 && L.out(5) == 1024);
  CHECK(L.in_end() == 512 && L.out_begin() == 1024 && L.total() == 1280);
  if (failures) return 1;
  printf("host layout: ok\n");
  return 0;
}
