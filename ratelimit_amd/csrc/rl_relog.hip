// rl_relog.hip — rl_resize_history: the history log rebuilt at another size
// from the live chains only, on the device (gfx950).
//
// k_relog_place reads the table once, one lane per slot, grid-stride,
// consecutive lanes on consecutive slots; a slot's first 32 bytes hold all it
// needs (tag, cur.ws, chain head). A live slot with a chain walks it twice
// under log_find's checks (chain_walk_end, rl_chain.h). Walk 1 counts the
// entries the walk accepts and notes how it ended. The wave then reserves room
// for all its lanes' entries with ONE atomic on its partition's counter (the
// partition chosen by workgroup and wave, as log_append chooses it) and the
// lanes take their bases from a wave prefix sum, so a wave's copies are one
// contiguous run of the new log and a key's copies are contiguous within it,
// oldest at the lowest index. Walk 2 copies entry j (newest = 0) of a chain of
// L entries to base + L - 1 - j as two whole 16-B stores: slot, tag, t_app and
// the window record verbatim, prev = the copy below it; the oldest copy's prev
// is LOG_NONE where the old walk ended at the chain's end and LOG_LOST where it
// broke. map[i] = the chain's new head (LOG_LOST for a chain of no accepted
// entry). Nothing but the new log, map and ctr is written: the old log and the
// table are only read, so the walks of one launch all see the same chains. A
// wave whose reservation passes the new capacity writes nothing and raises the
// overflow word (the host then drops the new log). The per-lane totals are
// folded per workgroup, one atomic per counter and workgroup.
//
// k_relog_commit, launched only once every shard has placed: ring = map[i] for
// the live slots that had a chain. The kernel boundary is the only
// synchronisation; no workgroup waits for another.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rl_chain.h"
#include "rl_device.h"
#include "rl_kernels.h"
#include "rl_slot_img.h"

namespace rl {

static_assert(LOG_MAX_HOPS * 64ull < (1ull << 32), "a wave's entries fit the 32-bit prefix sum");

__global__ __launch_bounds__(256) void k_relog_place(const TableDev t, uint64_t nslots, LogEnt* __restrict__ to,
                                                     uint32_t to_cap, uint32_t* __restrict__ map,
                                                     unsigned long long* ctr) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t p = (blockIdx.x * 4u + wave) & (LOG_PARTS - 1u);
  unsigned long long v[3] = {0, 0, 0};  // chains, entries kept, chains that end in LOG_LOST
  uint32_t longest = 0;
  // (the trip count is the workgroup's: every lane of a wave reaches the shuffles)
  for (uint64_t i0 = blockIdx.x * 256ull; i0 < nslots; i0 += (uint64_t)gridDim.x * 256) {
    const uint64_t i = i0 + threadIdx.x;
    SlotImg im;
    bool has = false;
    if (i < nslots) {
      load_img_head(&t.slots[i], im);
      has = im.tag() >= 2 && im.ring() != RING_NONE;
    }
    uint32_t len = 0;
    bool broken = false;
    if (has) {
      broken = chain_walk_end(t, (uint32_t)i, im.tag(), im.ring(), im.cur().ws, [&](LogEnt&, uint32_t) {
                 len++;
                 return true;
               }) != CHAIN_END;
    }
    uint32_t incl = len;  // the wave's inclusive prefix sum of len
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t o = __shfl_up(incl, d);
      if (lane >= (uint32_t)d) incl += o;
    }
    const uint32_t total = __shfl(incl, 63);
    unsigned long long wbase = 0;
    if (total) {
      if (lane == 0) wbase = atomicAdd(&ctr[(size_t)p * LOG_CTR_STRIDE], (unsigned long long)total);
      wbase = __shfl(wbase, 0);
    }
    const bool fits = wbase + total <= to_cap;
    if (total && !fits && lane == 0) atomicAdd(&ctr[RELOG_CTR_STATS + 4], 1ull);
    if (!has) continue;
    v[0]++;
    v[1] += len;
    v[2] += broken;
    longest = len > longest ? len : longest;
    if (!fits) continue;
    const uint32_t base = (uint32_t)wbase + (incl - len);  // (below to_cap <= LOG_PART_MAX)
    map[i] = len ? (p << LOG_POS_BITS) | (base + len - 1u) : LOG_LOST;
    if (!len) continue;
    LogEnt* dst = to + (size_t)p * to_cap;
    const uint32_t oldest = broken ? LOG_LOST : LOG_NONE;
    chain_walk_end(t, (uint32_t)i, im.tag(), im.ring(), im.cur().ws, [&](LogEnt& e, uint32_t j) {
      if (j >= len) return false;  // (nothing writes the old log between the walks: never taken)
      const uint32_t at = base + len - 1u - j;
      const uint4* s = reinterpret_cast<const uint4*>(&e);
      const uint4 a = s[0], b = s[1];
      uint4* d = reinterpret_cast<uint4*>(&dst[at]);
      d[0] = make_uint4(a.x, a.y, j + 1u == len ? oldest : (p << LOG_POS_BITS) | (at - 1u), a.w);
      d[1] = b;
      return true;
    });
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const uint32_t o = __shfl_xor(longest, m);
    longest = o > longest ? o : longest;
  }
  __shared__ unsigned long long sh[4][3];
  __shared__ uint32_t shl[4];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const unsigned long long x = wave_sum(v[k]);
    if (lane == 0) sh[wave][k] = x;
  }
  if (lane == 0) shl[wave] = longest;
  __syncthreads();
  if (threadIdx.x < 3) {
    const unsigned long long x = sh[0][threadIdx.x] + sh[1][threadIdx.x] + sh[2][threadIdx.x] + sh[3][threadIdx.x];
    if (x) atomicAdd(&ctr[RELOG_CTR_STATS + threadIdx.x], x);
  } else if (threadIdx.x == 3) {
    uint32_t x = shl[0];
    for (int k = 1; k < 4; k++) x = shl[k] > x ? shl[k] : x;
    if (x) atomicMax(&ctr[RELOG_CTR_STATS + 3], (unsigned long long)x);
  }
}

__global__ __launch_bounds__(256) void k_relog_commit(Slot* slots, uint64_t nslots, const uint32_t* __restrict__ map) {
  for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < nslots; i += (uint64_t)gridDim.x * 256) {
    SlotImg im;
    load_img_head(&slots[i], im);
    if (im.tag() < 2 || im.ring() == RING_NONE) continue;
    slots[i].ring = map[i];
  }
}

static uint32_t relog_grid(uint64_t nslots) { return (uint32_t)((nslots + 255) / 256 < 2048 ? (nslots + 255) / 256 : 2048); }

void launch_relog_place(const TableDev& t, uint64_t nslots, LogEnt* to, uint32_t to_cap, uint32_t* map,
                        unsigned long long* ctr, hipStream_t st) {
  if (!nslots) return;
  k_relog_place<<<relog_grid(nslots), 256, 0, st>>>(t, nslots, to, to_cap, map, ctr);
}

void launch_relog_commit(Slot* slots, uint64_t nslots, const uint32_t* map, hipStream_t st) {
  if (!nslots) return;
  k_relog_commit<<<relog_grid(nslots), 256, 0, st>>>(slots, nslots, map);
}

}  // namespace rl
