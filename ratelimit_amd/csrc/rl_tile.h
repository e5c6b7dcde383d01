// rl_tile.h — the record k_part leaves per descriptor in the tile layout and
// the bucket kernels gather: 8 bytes, {sort key, index | hits9 << 23}.
// hits9 is the raw HitsAddend for 0..510; 511 (TILE_HITS_ESC) sends the reader
// to the batch's hits array at `index` (the array k_part read: b.hits, or
// Scratch::hit_a of a routed owner batch). Plain C++ (no HIP types), so the
// host-side test builds it alone.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define RL_TILE_HD __host__ __device__
#else
#define RL_TILE_HD
#endif

namespace rl {

constexpr uint32_t TILE_IDX_BITS = 23;  // descriptor index (max_batch <= 2^23)
constexpr uint32_t TILE_IDX_MASK = (1u << TILE_IDX_BITS) - 1u;
constexpr uint32_t TILE_HITS_ESC = (1u << (32 - TILE_IDX_BITS)) - 1u;  // 511: hits live in the array

struct __attribute__((aligned(8))) TileRec {
  uint32_t key;  // sort key (high 32 bits of the stem hash)
  uint32_t iv;   // index | hits9 << TILE_IDX_BITS
};
static_assert(sizeof(TileRec) == 8, "one dwordx2 per record");

RL_TILE_HD inline TileRec tile_pack(uint32_t key, uint32_t index, uint32_t hits) {
  const uint32_t h9 = hits < TILE_HITS_ESC ? hits : TILE_HITS_ESC;
  return TileRec{key, (index & TILE_IDX_MASK) | (h9 << TILE_IDX_BITS)};
}
RL_TILE_HD inline uint32_t tile_index(uint32_t iv) { return iv & TILE_IDX_MASK; }
RL_TILE_HD inline bool tile_escaped(uint32_t iv) { return (iv >> TILE_IDX_BITS) == TILE_HITS_ESC; }
// The raw hits of a record's second word; `hits` is read only for an escaped record.
RL_TILE_HD inline uint32_t tile_hits(uint32_t iv, const uint32_t* hits) {
  return tile_escaped(iv) ? hits[iv & TILE_IDX_MASK] : iv >> TILE_IDX_BITS;
}
// The one unpack every tile reader goes through.
RL_TILE_HD inline void tile_unpack(const TileRec& e, const uint32_t* hits, uint32_t& key, uint32_t& index,
                                   uint32_t& h) {
  key = e.key;
  index = tile_index(e.iv);
  h = tile_hits(e.iv, hits);
}

}  // namespace rl
