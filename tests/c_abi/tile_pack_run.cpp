// tile_pack_run.cpp — rl_tile.h compiled for the host (test program,
// tests/test_tile_pack_cpu.py): every (index, hits) of the edge sets packs into
// one 8-byte record and either round-trips or flags the escape, in which case
// the unpack reads the hits array at exactly `index` and nowhere else.
//
//   g++ -std=c++17 -Wall -Wextra -I ratelimit_amd/csrc tile_pack_run.cpp
//
// Prints "ok <cases>" and exits 0, or the first difference and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rl_tile.h"

namespace {

[[noreturn]] void die(const char* what, uint32_t index, uint32_t hits) {
  printf("FAIL index %u hits %u: %s\n", index, hits, what);
  exit(1);
}

}  // namespace

int main() {
  static_assert(rl::TILE_IDX_BITS == 23 && rl::TILE_HITS_ESC == 511, "23 index bits, 9 hits bits");
  const uint32_t top = (1u << 23) - 1;
  const uint32_t indices[] = {0u, 1u, 4095u, 4096u, 4097u, 65535u, 65536u, (1u << 22) - 1, 1u << 22, top - 1, top};
  const uint32_t hits[] = {0u, 1u, 2u, 255u, 256u, 509u, 510u, 511u, 512u, 1023u, 65535u, 65536u,
                           0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFEu, 0xFFFFFFFFu};
  const uint32_t keys[] = {0u, 1u, 0x003FFFFFu, 0x00400000u, 0xFFC00000u, 0xFFFFFFFFu};
  int cases = 0;
  for (uint32_t index : indices)
    for (uint32_t h : hits)
      for (uint32_t key : keys) {
        const rl::TileRec e = rl::tile_pack(key, index, h);
        if (e.key != key) die("the key changed", index, h);
        if (rl::tile_index(e.iv) != index) die("the index changed", index, h);
        const bool esc = rl::tile_escaped(e.iv);
        if (esc != (h >= 511u)) die("the escape flag is wrong", index, h);
        if (!esc && (e.iv >> 23) != h) die("inline hits differ", index, h);
        // inline hits: the array is never touched (a null pointer would fault)
        if (!esc && rl::tile_hits(e.iv, nullptr) != h) die("inline hits do not round-trip", index, h);
        // escaped hits: an array of exactly index + 1 words, the last one the
        // hits (a read at any other index is out of bounds or returns a canary)
        std::vector<uint32_t> arr((size_t)index + 1, 0xA5A5A5A5u ^ h);
        arr[index] = h;
        uint32_t k2 = ~key, i2 = ~index, h2 = ~h;
        rl::tile_unpack(e, arr.data(), k2, i2, h2);
        if (k2 != key || i2 != index || h2 != h) die("tile_unpack does not round-trip", index, h);
        cases++;
      }
  // hits of 511 itself is escaped, not taken for the marker's value
  if (!rl::tile_escaped(rl::tile_pack(0, 0, 511).iv) || rl::tile_escaped(rl::tile_pack(0, top, 510).iv))
    die("the escape boundary moved", 0, 511);
  // index bits never spill into the hits bits
  if (rl::tile_pack(0, top, 0).iv != top) die("the index spilled into the hits bits", top, 0);
  printf("ok %d\n", cases);
  return 0;
}
