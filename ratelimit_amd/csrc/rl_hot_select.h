// rl_hot_select.h — what rl_hot_keys selects and how its answer is ordered,
// shared by the device scan (rl_hot.hip), the host merge (rl_api.hip) and a
// host driver (tests/c_abi/hot_select_run.cpp). Plain C++; RLH_HD is
// __host__ __device__ under hipcc and empty otherwise.
//
// A record is a slot's newest window (Slot::cur: the record rl_export_range
// emits last for its key). It matches a query read at the clock `now` when
//   its unit is in the mask (0: every unit),
//   ws == now - now % div(unit)          (the window `now` falls in),
//   now <= expire                        (the Redis key is live),
//   count >= min_count, and
//   with BLOCKED, now < lc               (the local over-limit cache entry is live).
// The answer is ordered by count descending, ties by stem bytes ascending
// (memcmp, the shorter first), then by unit. Each shard answers the top k of
// its own records; the top k of their union is the top k of the table.
#pragma once

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RLH_HD __host__ __device__ __forceinline__
#else
#define RLH_HD inline
#endif

#include <algorithm>
#include <vector>

namespace rlhot {

constexpr uint32_t BLOCKED = 0x1u;        // == RL_HOT_BLOCKED
constexpr uint32_t UNIT_BITS = 0x1Eu;     // bits 1..4: rl_unit second .. day
constexpr uint32_t WS_NONE = 0xFFFFFFFFu; // == WS_INVALID: the slot has no record

struct Query {
  uint32_t now, min_count, unit_mask, flags;
};

RLH_HD uint32_t unit_div(uint32_t unit) {  // utils.UnitToDivider
  return unit == 1u ? 1u : unit == 2u ? 60u : unit == 3u ? 3600u : 86400u;
}

RLH_HD bool match(const Query& q, uint32_t unit, uint32_t ws, uint32_t count, uint32_t expire, uint32_t lc) {
  if (unit < 1u || unit > 4u || ws == WS_NONE) return false;
  if (q.unit_mask && !((q.unit_mask >> unit) & 1u)) return false;
  if (ws != q.now - q.now % unit_div(unit)) return false;
  if (q.now > expire || count < q.min_count) return false;
  return !(q.flags & BLOCKED) || q.now < lc;
}

// One record of an answer; stem points into storage the caller keeps.
struct Rec {
  uint32_t count, ws, expire, lc;
  uint32_t unit, len;
  const uint8_t* stem;
};

RLH_HD int stem_cmp(const uint8_t* a, uint32_t alen, const uint8_t* b, uint32_t blen) {
  const uint32_t m = alen < blen ? alen : blen;
#if defined(__HIP_DEVICE_COMPILE__)
  for (uint32_t i = 0; i < m; i++)
    if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
#else
  if (const int c = m ? memcmp(a, b, m) : 0) return c < 0 ? -1 : 1;
#endif
  return alen < blen ? -1 : alen > blen ? 1 : 0;
}

// a comes before b in an answer
RLH_HD bool before(const Rec& a, const Rec& b) {
  if (a.count != b.count) return a.count > b.count;
  const int c = stem_cmp(a.stem, a.len, b.stem, b.len);
  if (c) return c < 0;
  return a.unit < b.unit;
}

// The answer's order, and its first k records (k >= size: all of them).
inline void order_top(std::vector<Rec>& r, uint32_t k) {
  std::sort(r.begin(), r.end(), [](const Rec& a, const Rec& b) { return before(a, b); });
  if (r.size() > k) r.resize(k);
}

// The shards' answers (each the top k of its shard, in any order) merged:
// the top k of their union, ordered.
inline std::vector<Rec> merge(const std::vector<std::vector<Rec>>& shards, uint32_t k) {
  std::vector<Rec> all;
  for (const std::vector<Rec>& s : shards) all.insert(all.end(), s.begin(), s.end());
  order_top(all, k);
  return all;
}

// threshold = the count of an ordered answer's last record (0: empty), above =
// its records with a larger count (every such record of the table is in it).
inline void summarize(const std::vector<Rec>& r, uint32_t* threshold, uint64_t* above) {
  *threshold = r.empty() ? 0u : r.back().count;
  uint64_t a = 0;
  for (const Rec& x : r) a += x.count > *threshold;
  *above = a;
}

}  // namespace rlhot
