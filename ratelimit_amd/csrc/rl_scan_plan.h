// rl_scan_plan.h — where one rl_scan call cuts: which of the counted tiles fit
// the caller's remaining capacity, and where each of them writes. Plain C++,
// shared by the engine (rl_engine.hip), the kernels (rl_scan.hip: TileSum) and
// a host driver (tests/c_abi/scan_plan_run.cpp).
//
// k_scan_count leaves one TileSum per tile of RL_SCAN_TILE slots. A call
// covers whole tiles, in slot order, as long as the records and the stem bytes
// of all covered tiles stay within the capacities; it stops in front of the
// first tile that does not fit (a tile without records always fits, so empty
// stretches never end a page). Each covered tile's output base is the sum of
// the tiles before it: no output position depends on the order in which
// workgroups run, and the same table gives the same bytes whatever the
// capacities were.
#pragma once

#include <stdint.h>

namespace rlscan {

constexpr uint32_t TILE = 1024;  // == RL_SCAN_TILE
// the stem bytes of one call stay below 2^32: rl_records' offsets are 32-bit
constexpr uint64_t BYTES_MAX = 0xFFFFFFFFull;

struct TileSum {
  uint64_t records, bytes, keys, lost;  // of the tile's selected keys after the query's filters
};

struct Cut {
  uint32_t tiles;           // tiles covered: sums[0 .. tiles)
  uint64_t records, bytes;  // their sums (== the position after the last covered tile)
  uint64_t keys, lost;
};

// rec_cap / byte_cap: what is left of the caller's capacity (byte_cap already
// clamped so that the call's total stays <= BYTES_MAX). base[i] (i < the
// result's tiles; may be null) = records << 32 | bytes in front of tile i,
// relative to this span (both < 2^32 where base is used: the engine stages a
// span's records in 32-bit positions and asks for rec_cap <= 2^32 - 1).
inline Cut plan(const TileSum* sums, uint32_t n, uint64_t rec_cap, uint64_t byte_cap, uint64_t* base) {
  Cut c{0, 0, 0, 0, 0};
  if (byte_cap > BYTES_MAX) byte_cap = BYTES_MAX;
  for (uint32_t i = 0; i < n; i++) {
    const TileSum& t = sums[i];
    // (no sum overflows: a tile holds at most TILE keys of 65535 bytes and a bounded chain each)
    if (t.records > rec_cap - c.records || t.bytes > byte_cap - c.bytes) break;
    if (base) base[i] = (c.records << 32) | c.bytes;
    c.records += t.records;
    c.bytes += t.bytes;
    c.keys += t.keys;
    c.lost += t.lost;
    c.tiles = i + 1;
  }
  return c;
}

// tiles of a shard of nslots slots (the last one may be short)
inline uint64_t tiles_of(uint64_t nslots) { return (nslots + TILE - 1) / TILE; }

}  // namespace rlscan
