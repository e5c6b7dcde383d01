// scan_plan_run.cpp — rl_scan_plan.h on the host (test program,
// tests/test_scan_cpu.py): rlscan::plan against a brute-force loop that tries
// every cut length and keeps the longest whose sums fit. Stand-alone (its own
// main), built plain and under AddressSanitizer + UndefinedBehaviorSanitizer.
// Prints "ok <cases>".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rl_scan_plan.h"

using rlscan::Cut;
using rlscan::TileSum;

static int cases = 0;

static void fail(const char* what, int line) {
  std::printf("FAIL %s (line %d)\n", what, line);
  std::exit(1);
}
#define CHECK(x) do { if (!(x)) fail(#x, __LINE__); } while (0)

// the longest prefix of the tiles whose sums fit both capacities (and the 32-bit offsets' reach)
static uint32_t brute(const std::vector<TileSum>& t, uint64_t rec_cap, uint64_t byte_cap) {
  uint32_t best = 0;
  for (uint32_t k = 0; k <= t.size(); k++) {
    unsigned __int128 r = 0, b = 0;
    for (uint32_t i = 0; i < k; i++) {
      r += t[i].records;
      b += t[i].bytes;
    }
    if (r <= rec_cap && b <= byte_cap && b <= rlscan::BYTES_MAX) best = k; else break;
  }
  return best;
}

static Cut run(const std::vector<TileSum>& t, uint64_t rec_cap, uint64_t byte_cap, uint32_t want) {
  std::vector<uint64_t> base(t.size() + 1, 0xDEADBEEFDEADBEEFull);  // (exactly sized: ASan sees a write past the cut)
  const Cut c = rlscan::plan(t.data(), (uint32_t)t.size(), rec_cap, byte_cap, base.data());
  CHECK(c.tiles == brute(t, rec_cap, byte_cap));
  CHECK(c.tiles == want);
  uint64_t r = 0, b = 0, k = 0, l = 0;
  for (uint32_t i = 0; i < c.tiles; i++) {
    CHECK(base[i] == ((r << 32) | b));
    r += t[i].records, b += t[i].bytes, k += t[i].keys, l += t[i].lost;
  }
  for (size_t i = c.tiles; i < base.size(); i++) CHECK(base[i] == 0xDEADBEEFDEADBEEFull);  // nothing past the cut
  CHECK(c.records == r && c.bytes == b && c.keys == k && c.lost == l);
  CHECK(r <= rec_cap && b <= byte_cap && b <= rlscan::BYTES_MAX);
  const Cut d = rlscan::plan(t.data(), (uint32_t)t.size(), rec_cap, byte_cap, nullptr);  // (base is optional)
  CHECK(d.tiles == c.tiles && d.records == c.records && d.bytes == c.bytes);
  cases++;
  return c;
}

int main() {
  const TileSum A{3, 30, 2, 1}, B{5, 100, 5, 0}, Z{0, 0, 0, 0}, C{1, 7, 1, 0};
  // no tiles
  run({}, 10, 10, 0);
  CHECK(rlscan::plan(nullptr, 0, 0, 0, nullptr).tiles == 0);
  // the first tile not fitting (records, then bytes), also with capacity zero
  run({A, B}, 2, 1000, 0);
  run({A, B}, 1000, 29, 0);
  run({A, B}, 0, 0, 0);
  // empty tiles always fit, up to the first tile with records
  run({Z, Z, A}, 0, 0, 2);
  run({Z, Z, Z}, 0, 0, 3);
  // an exact fit, one short of a fit (records and bytes)
  run({A, B, C}, 9, 137, 3);
  run({A, B, C}, 8, 137, 2);
  run({A, B, C}, 9, 136, 2);
  run({A, B}, 8, 130, 2);
  run({A, B}, 7, 130, 1);
  run({A, B}, 8, 129, 1);
  // the record cap binds before the byte cap, and the reverse
  run({A, B, B, B}, 13, 1 << 20, 3);
  run({A, B, B, B}, 1 << 20, 231, 3);
  run({A, B, B, B}, 13, 131, 2);
  // the cut never skips a tile that does not fit to take a later one that would
  run({A, B, C}, 4, 1000, 1);
  // the 2^32 byte bound: the stem offsets are 32-bit whatever stem_cap says
  const TileSum G{1000, 0x7FFFFFFFull, 1000, 0}, H{1, 1, 1, 0}, I{2, 2, 1, 0};
  run({G, G, H, I}, ~0ull, ~0ull, 3);              // 2^32 - 1 bytes exactly: fits; one more byte does not
  run({G, G, I}, ~0ull, ~0ull, 2);
  run({G, G, H}, ~0ull, 0xFFFFFFFFull, 3);
  run({G, G, H}, ~0ull, 0xFFFFFFFEull, 2);
  run({TileSum{1, 0x100000000ull, 1, 0}}, ~0ull, ~0ull, 0);
  run({G, G, H}, 0xFFFFFFFFull, ~0ull, 3);         // (rec_cap as large as rl_records::n goes)
  // a short last tile is a tile like any other to the planner; tiles_of rounds up
  CHECK(rlscan::tiles_of(0) == 0 && rlscan::tiles_of(1) == 1 && rlscan::tiles_of(256) == 1);
  CHECK(rlscan::tiles_of(1024) == 1 && rlscan::tiles_of(1025) == 2 && rlscan::tiles_of(1ull << 32) == (1u << 22));
  CHECK(rlscan::TILE == 1024);
  run({B, B, TileSum{2, 20, 1, 1}}, 12, 220, 3);
  // random tiles against the brute force
  uint64_t x = 88172645463325252ull;
  auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
  for (int it = 0; it < 4000; it++) {
    std::vector<TileSum> t(rnd() % 9);
    uint64_t tr = 0, tb = 0;
    for (TileSum& s : t) {
      s.records = rnd() % 4 ? rnd() % 50 : 0;
      s.bytes = s.records * (1 + rnd() % 300);
      s.keys = s.records ? 1 + rnd() % s.records : 0;
      s.lost = s.keys ? rnd() % 2 : 0;
      tr += s.records, tb += s.bytes;
    }
    const uint64_t rc = rnd() % 3 ? rnd() % (tr + 2) : tr, bc = rnd() % 3 ? rnd() % (tb + 2) : tb;
    run(t, rc, bc, brute(t, rc, bc));
  }
  std::printf("ok %d\n", cases);
  return 0;
}
