// log_geom_run.cpp — rl_log_geom.h on the host (test program,
// tests/test_relog_cpu.py): log_part_cap against the rule as rl_create has
// always stated it (std::max / two loops, restated below) over the three
// floors, the cap, exact powers of two and one above, and random requests.
// Stand-alone (its own main), built plain and under AddressSanitizer +
// UndefinedBehaviorSanitizer. Prints "cap <history_entries> <max_batch> <per
// partition>" for the pinned requests, then "ok <cases>".
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "rl_log_geom.h"

static const uint32_t PARTS = 64;
static const uint64_t PART_MAX = 1ull << 25;
static int cases = 0;

static void fail(const char* what, int line) {
  std::printf("FAIL %s (line %d)\n", what, line);
  std::exit(1);
}
#define CHECK(x) do { if (!(x)) fail(#x, __LINE__); } while (0)

// the rule in rl_create's words
static uint64_t stated(uint64_t history_entries, uint32_t max_batch) {
  const uint64_t want = std::max<uint64_t>(history_entries / PARTS, std::max<uint64_t>(max_batch / 16, 1024));
  uint64_t cap = 1;
  while (cap * 2 <= want && cap * 2 <= PART_MAX) cap *= 2;
  if (cap < want && cap < PART_MAX) cap *= 2;
  return cap;
}

static uint64_t one(uint64_t he, uint32_t mb) {
  const uint64_t cap = rl::log_part_cap(he, mb, PARTS, PART_MAX);
  CHECK(cap == stated(he, mb));
  CHECK((cap & (cap - 1)) == 0 && cap >= 1024 && cap <= PART_MAX);
  CHECK(cap >= mb / 16u || cap == PART_MAX);
  CHECK(cap >= he / PARTS || cap == PART_MAX);
  CHECK(cap == 1024 || cap / 2 < std::max<uint64_t>(he / PARTS, mb / 16u));  // (the smallest such power of two)
  cases++;
  return cap;
}

int main() {
  const uint64_t pinned[][2] = {
      {1, 1u << 14},          {1ull << 16, 1u << 14},       {(1ull << 16) + 64, 1u << 14}, {1ull << 18, 1u << 14},
      {1ull << 20, 1u << 20}, {1, 1u << 20},                {1, 8388608},                  {1ull << 31, 1u << 14},
      {(1ull << 31) - 1, 1},  {(1ull << 30) + 64, 1u << 16}, {1ull << 27, 1u << 20},       {(1ull << 27) + 63, 1u << 20},
      {(1ull << 27) + 64, 1u << 20}, {65535, 1},            {65536 + 63, 1},               {1ull << 28, 1u << 22}};
  for (const auto& p : pinned) std::printf("cap %llu %u %llu\n", (unsigned long long)p[0], (unsigned)p[1],
                                           (unsigned long long)one(p[0], (uint32_t)p[1]));
  for (uint32_t k = 0; k <= 31; k++)  // exact powers of two, one below, one partition's worth above
    for (uint32_t mb : {1u, 1u << 14, 1u << 17, 8388608u}) {
      one(1ull << k, mb);
      if (k) one((1ull << k) - 1, mb);
      if ((1ull << k) + PARTS <= (1ull << 31)) one((1ull << k) + PARTS, mb);
    }
  uint64_t x = 0x9E3779B97F4A7C15ull;
  for (int i = 0; i < 20000; i++) {
    x ^= x << 13; x ^= x >> 7; x ^= x << 17;
    const uint64_t he = 1 + (x >> 8) % (1ull << (1 + (x & 31)));
    const uint32_t mb = 1 + (uint32_t)((x >> 40) % 8388608u);
    if (he <= (1ull << 31)) one(he, mb);
  }
  CHECK(rl::log_entries_fit(1ull << 31, PARTS, PART_MAX) && !rl::log_entries_fit((1ull << 31) + 1, PARTS, PART_MAX));
  CHECK(rl::log_entries_fit(1, PARTS, PART_MAX));
  std::printf("ok %d\n", cases);
  return 0;
}
