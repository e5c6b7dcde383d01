// rl_hot.hip — rl_hot_keys: the K busiest (or currently blocked) keys of the
// table at one clock, selected on the device (gfx950).
//
// The table is scanned once, range by range (at most 2^22 slots each, like
// the export; the first ranges are small and double, eng_hot_keys). k_hot_scan
// reads the first 32 bytes of every slot (tag, unit, newest window), one lane per
// slot, sums the matching records and their counts, and compacts (count, slot)
// of the matching ones into a candidate pool: every one while the pool has
// not been cut yet, afterwards only counts above the running threshold (the
// pool then already holds K records at or above it, so a tied record need not
// enter: which of the tied ones are answered is unspecified). After a range
// whose candidates took the pool past 2K, k_hot_select finds the K-th largest
// count in the pool by a radix select over its four bytes (LDS histograms),
// keeps the records above it and as many tied ones as make K, and raises the
// threshold. A last cut to K, then k_hot_size / k_hot_gather fetch the
// winners' window fields and stems (export_stem: inline bytes and arena) for
// one copy to the host, which orders them (rl_hot_select.h).
//
// The pool holds at most 2K + one range of entries, so device scratch does
// not grow with the table; the slots are read once, the winners' slots twice.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rl_device.h"
#include "rl_kernels.h"
#include "rl_slot_img.h"
#include "rl_hot_select.h"

namespace rl {

namespace {

__device__ inline uint32_t lanes_below(unsigned long long m) {
  return (uint32_t)__popcll(m & ((1ull << (threadIdx.x & 63u)) - 1ull));
}

}  // namespace

// Grid-stride with a trip count uniform per workgroup; matched / hits are kept
// per lane and folded per workgroup, one atomic per counter (k_export_count's
// comment: a wave's own atomics on one line cost more than the scan). The
// pool's places are reserved once per workgroup and iteration, and only by
// iterations that have a candidate: after the first cut almost none has.
__global__ __launch_bounds__(256) void k_hot_scan(const TableDev t, uint64_t s0, uint64_t s1, const rlhot::Query q,
                                                  uint32_t k, HotState* st, unsigned long long* __restrict__ pool,
                                                  uint32_t pool_cap) {
  const uint32_t full = st->full, thr = st->thr;  // (k_hot_select writes them, between launches)
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  unsigned long long v[2] = {0, 0};
  __shared__ uint32_t wcnt[4];
  __shared__ uint32_t base_sh;
  for (uint64_t b = s0 + blockIdx.x * 256ull; b < s1; b += (uint64_t)gridDim.x * 256) {
    const uint64_t i = b + threadIdx.x;
    bool cand = false;
    uint32_t count = 0;
    if (i < s1) {
      SlotImg im;
      load_img_head(&t.slots[i], im);  // (the stems are not needed: half the bytes through the vector path)
      const Win w = im.cur();
      if (im.tag() >= 2 && rlhot::match(q, im.unit(), w.ws, w.count, w.expire, w.lc)) {
        count = w.count;
        v[0] += 1;
        v[1] += count;
        cand = k && (!full || count > thr);
      }
    }
    if (!__syncthreads_or(cand)) continue;  // (also keeps wcnt / base_sh of the last reservation until all have read them)
    const unsigned long long m = __ballot(cand);
    if (lane == 0) wcnt[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) base_sh = atomicAdd(&st->pool_n, wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3]);
    __syncthreads();
    if (cand) {
      uint32_t pos = base_sh + lanes_below(m);
      for (uint32_t x = 0; x < wave; x++) pos += wcnt[x];
      if (pos < pool_cap) pool[pos] = ((unsigned long long)count << 32) | (uint32_t)i;
      else atomicOr(&st->err, 1u);  // (cannot happen: the pool holds 2K + a range)
    }
  }
  __shared__ unsigned long long sh[4][2];
#pragma unroll
  for (int j = 0; j < 2; j++) {
    const unsigned long long x = wave_sum(v[j]);
    if (lane == 0) sh[wave][j] = x;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    const unsigned long long x = sh[0][threadIdx.x] + sh[1][threadIdx.x] + sh[2][threadIdx.x] + sh[3][threadIdx.x];
    if (x) atomicAdd(threadIdx.x ? &st->hits : &st->matched, x);
  }
}

// One workgroup. Does nothing while the pool holds at most `limit` entries
// (limit >= k). Otherwise: the K-th largest count T by a radix select, most
// significant byte first; then the pool is compacted in place to the entries
// above T and K - (their number) of the tied ones, and T becomes the scan's
// threshold. Counters are heavily skewed (almost every candidate falls into
// one bin), so a wave counts its lanes per bin first (ballot on the leader's
// bin) and touches LDS once per distinct bin, not once per lane.
constexpr uint32_t HOT_SELECT_THREADS = 1024;
__global__ __launch_bounds__(HOT_SELECT_THREADS) void k_hot_select(HotState* st, unsigned long long* pool,
                                                                   uint32_t pool_cap, uint32_t k, uint32_t limit) {
  const uint32_t n = st->pool_n < pool_cap ? st->pool_n : pool_cap;
  if (n <= limit || !k) return;  // (uniform)
  const uint32_t lane = threadIdx.x & 63u;
  __shared__ uint32_t hist[256];
  __shared__ uint32_t s_prefix, s_need, s_kept, s_ties;
  uint32_t prefix = 0, mask = 0, need = k;
  for (int shift = 24; shift >= 0; shift -= 8) {
    if (threadIdx.x < 256) hist[threadIdx.x] = 0;
    __syncthreads();
    for (uint32_t b = 0; b < n; b += HOT_SELECT_THREADS) {
      const uint32_t i = b + threadIdx.x;
      const uint32_t c = i < n ? (uint32_t)(pool[i] >> 32) : 0u;
      const bool ok = i < n && (c & mask) == prefix;
      const uint32_t bin = (c >> shift) & 255u;
      unsigned long long pending = __ballot(ok);
      while (pending) {  // (uniform per wave)
        const int leader = __ffsll((long long)pending) - 1;
        const uint32_t lb = (uint32_t)__shfl((int)bin, leader);
        const unsigned long long same = __ballot(ok && bin == lb);
        if ((int)lane == leader) atomicAdd(&hist[lb], (uint32_t)__popcll(same));
        pending &= ~same;
      }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t acc = 0, b = 255;
      while (b && acc + hist[b] < need) acc += hist[b--];  // (n > k: the K-th exists)
      s_prefix = prefix | (b << shift);
      s_need = need - acc;
    }
    __syncthreads();
    prefix = s_prefix;
    need = s_need;
    mask |= 255u << shift;
  }
  const uint32_t T = prefix;  // `need` of the entries with count == T stay
  if (threadIdx.x == 0) s_kept = s_ties = 0;
  for (uint32_t b = 0; b < n; b += HOT_SELECT_THREADS) {
    const uint32_t i = b + threadIdx.x;
    const unsigned long long e = i < n ? pool[i] : 0ull;
    const uint32_t c = (uint32_t)(e >> 32);
    const bool tie = i < n && c == T;
    bool keep = i < n && c > T;
    // a kept entry lands at or below its own place: every lane has read this
    // chunk before any of them writes into it
    __syncthreads();
    const unsigned long long tb = __ballot(tie);
    if (tb) {
      const int leader = __ffsll((long long)tb) - 1;
      uint32_t at = 0;
      if ((int)lane == leader) at = atomicAdd(&s_ties, (uint32_t)__popcll(tb));
      at = (uint32_t)__shfl((int)at, leader);
      keep = keep || (tie && at + lanes_below(tb) < need);
    }
    const unsigned long long kb = __ballot(keep);
    if (kb) {
      const int leader = __ffsll((long long)kb) - 1;
      uint32_t at = 0;
      if ((int)lane == leader) at = atomicAdd(&s_kept, (uint32_t)__popcll(kb));
      at = (uint32_t)__shfl((int)at, leader);
      if (keep) pool[at + lanes_below(kb)] = e;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    st->pool_n = s_kept;
    st->thr = T;
    st->full = 1;
  }
}

// The winners' stem bytes (what the gather will write).
__global__ __launch_bounds__(256) void k_hot_size(const TableDev t, HotState* st, const unsigned long long* __restrict__ pool,
                                                  uint32_t pool_cap) {
  const uint32_t n = st->pool_n < pool_cap ? st->pool_n : pool_cap;
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  unsigned long long len = 0;
  if (j < n) len = t.slots[(uint32_t)pool[j]].key_len;
  len = wave_sum(len);
  if ((threadIdx.x & 63u) == 0 && len) atomicAdd(&st->stem_bytes, len);
}

// One lane per winner: its slot's newest window and whole stem. The stems'
// places are reserved per wave (an inclusive scan of the lengths, one atomic).
__global__ __launch_bounds__(256) void k_hot_gather(const TableDev t, HotState* st,
                                                    const unsigned long long* __restrict__ pool, uint32_t n,
                                                    const HotOutDev o) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
  SlotImg im;
  uint32_t len = 0, slot = 0;
  if (j < n) {
    slot = (uint32_t)pool[j];
    load_img_lo(&t.slots[slot], im);
    len = im.key_len();
  }
  unsigned long long x = len;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const unsigned long long y = __shfl_up(x, d);
    if (lane >= d) x += y;
  }
  const unsigned long long tot = __shfl(x, 63);
  unsigned long long base = 0;
  if (lane == 0 && tot) base = atomicAdd(&st->cursor, tot);
  base = __shfl(base, 0);
  if (j >= n) return;
  const unsigned long long B = base + x - len;
  const Win w = im.cur();
  o.off[j] = (uint32_t)B;
  o.len[j] = len;
  o.unit[j] = (uint8_t)im.unit();
  o.ws[j] = w.ws;
  o.count[j] = w.count;
  o.expire[j] = w.expire;
  o.lc[j] = w.lc;
  if (B + len <= o.stem_cap) export_stem(t, &t.slots[slot], len, o.stem + B);
  else atomicOr(&st->err, 2u);  // (cannot happen: k_hot_size summed the same lengths)
}

void launch_hot_scan(const TableDev& t, uint64_t s0, uint64_t s1, const rlhot::Query& q, uint32_t k, HotState* st,
                     unsigned long long* pool, uint32_t pool_cap, hipStream_t stream) {
  if (s1 > s0) {
    const uint64_t wg = (s1 - s0 + 255) / 256;
    k_hot_scan<<<(uint32_t)(wg < 2048 ? wg : 2048), 256, 0, stream>>>(t, s0, s1, q, k, st, pool, pool_cap);
  }
}

void launch_hot_select(HotState* st, unsigned long long* pool, uint32_t pool_cap, uint32_t k, uint32_t limit,
                       hipStream_t stream) {
  k_hot_select<<<1, HOT_SELECT_THREADS, 0, stream>>>(st, pool, pool_cap, k, limit);
}

void launch_hot_size(const TableDev& t, HotState* st, const unsigned long long* pool, uint32_t pool_cap, uint32_t k,
                     hipStream_t stream) {
  if (k) k_hot_size<<<(k + 255) / 256, 256, 0, stream>>>(t, st, pool, pool_cap);
}

void launch_hot_gather(const TableDev& t, HotState* st, const unsigned long long* pool, uint32_t n, const HotOutDev& o,
                       hipStream_t stream) {
  if (n) k_hot_gather<<<(n + 255) / 256, 256, 0, stream>>>(t, st, pool, n, o);
}

}  // namespace rl
