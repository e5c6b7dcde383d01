// rl_scan.hip — rl_scan: list the records of the keys whose stem begins with
// one of up to 64 prefixes, selected on the device, page by page (gfx950).
//
// The table is read in tiles of RL_SCAN_TILE slots, one workgroup per tile,
// one lane per slot. k_scan_count selects: the prefixes sit in LDS as
// k_forget_scan keeps them (their bytes, and per prefix one 16-B record: first
// dword, its length mask, length, offset; every lane reads the same address, a
// broadcast), and a slot's first 32 bytes (tag, key_len, unit, cur, chain
// head, stem bytes 0..3) reject most slots: tag < 2, a unit outside the mask,
// key_len below the shortest prefix, the first dword against each prefix's
// under its mask (rl_forget_match.h). Only survivors read the rest of the slot,
// and the arena only where a prefix reaches past the inline bytes. A selected
// key's records are the export's (export_next, rl_slot_img.h), filtered:
// RL_SCAN_NEWEST takes the slot's cur alone and never walks the chain,
// RL_SCAN_LIVE keeps the records with now <= expire. Each slot's word (records,
// prefix index, chain lost) goes to cnt; the tile's sums (records, stem bytes,
// keys, lost chains) are folded in the workgroup and written with plain stores:
// no atomic takes part in anything that decides an output position.
//
// The host cuts from the tile sums (rl_scan_plan.h) and k_scan_write runs over
// the covered tiles only: a lane's output place is its tile's base plus an
// in-workgroup exclusive scan of (records, bytes), k_export_write's shape
// without its atomic. Each lane writes its key's records oldest first.
//
// The per-prefix sums (keys, records, hits) describe the covered tiles only, so
// the kernel that runs over exactly those adds them: k_scan_write for a
// listing call, k_scan_count for a count-only call (which covers all it
// counts). Either way they go through an LDS histogram flushed once per
// workgroup, its non-zero bins only; sums do not depend on the order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rl_device.h"
#include "rl_kernels.h"
#include "rl_slot_img.h"
#include "rl_forget_match.h"
#include "rl_scan_plan.h"

namespace rl {

static_assert(rlscan::TILE == RL_SCAN_TILE, "rl_scan_plan.h restates the ABI's tile");
static_assert(rlforget::PREFIX_BYTES == 256 * 16, "the prefixes are staged with one 16-B load per lane of the first 256");
static_assert(slot_key_dw(0) == 7, "stem bytes 0..3 are the last dword of the slot's first 32 bytes");

namespace {

constexpr uint32_t SCAN_THREADS = rlscan::TILE;
constexpr uint32_t SCAN_WAVES = SCAN_THREADS / 64;
// a slot's word in cnt: records (a chain has at most LOG_MAX_HOPS entries) |
// prefix index << 24 | chain lost << 31
constexpr uint32_t SCAN_REC_MASK = 0x00FFFFFFu;
constexpr uint32_t SCAN_PFX_SHIFT = 24;
constexpr uint32_t SCAN_LOST = 0x80000000u;
static_assert(LOG_MAX_HOPS + 1u <= SCAN_REC_MASK, "a key's records fit the slot word");
static_assert(RL_FORGET_PREFIX_MAX <= 64, "the prefix index takes 6 bits of the slot word");

struct ScanLds {
  __attribute__((aligned(16))) uint8_t pfx[rlforget::PREFIX_BYTES];
  uint32_t off[rlforget::PREFIX_MAX + 1];
  uint4 head[rlforget::PREFIX_MAX];  // first dword, its mask, length, offset
  unsigned long long hist[rlforget::PREFIX_MAX][3];  // keys, records, hits
  uint32_t minlen;
};

__device__ inline void hist_clear(ScanLds& L) {
  if (threadIdx.x < rlforget::PREFIX_MAX * 3) (&L.hist[0][0])[threadIdx.x] = 0;
}

// after a barrier that follows every lane's adds
__device__ inline void hist_flush(ScanLds& L, uint32_t np, unsigned long long* byp) {
  const uint32_t bins = (np ? np : 1u) * 3;
  if (threadIdx.x < bins) {
    const unsigned long long x = (&L.hist[0][0])[threadIdx.x];
    if (x) atomicAdd(&byp[threadIdx.x], x);
  }
}

__device__ inline bool rec_live(const ScanQueryDev& q, const Win& w) {
  return !(q.flags & RL_SCAN_LIVE) || q.now <= w.expire;
}

}  // namespace

__global__ __launch_bounds__(SCAN_THREADS) void k_scan_count(const TableDev t, uint64_t nslots, uint64_t tile0,
                                                             const ScanQueryDev q, uint32_t* __restrict__ cnt,
                                                             rlscan::TileSum* __restrict__ sums,
                                                             unsigned long long* byp) {
  __shared__ ScanLds L;
  const uint32_t np = q.np;
  if (threadIdx.x < 256) reinterpret_cast<uint4*>(L.pfx)[threadIdx.x] = reinterpret_cast<const uint4*>(q.pfx)[threadIdx.x];
  if (threadIdx.x <= np) L.off[threadIdx.x] = q.poff[threadIdx.x];
  hist_clear(L);
  __syncthreads();
  if (threadIdx.x < np) {
    // (the host has checked the offsets; clamped all the same: no LDS read past the prefixes)
    const uint32_t a = L.off[threadIdx.x] < rlforget::PREFIX_BYTES ? L.off[threadIdx.x] : rlforget::PREFIX_BYTES;
    const uint32_t e = L.off[threadIdx.x + 1] < rlforget::PREFIX_BYTES ? L.off[threadIdx.x + 1] : rlforget::PREFIX_BYTES;
    const uint32_t len = e > a ? e - a : 0u;
    L.head[threadIdx.x] = uint4{rlforget::head_dword(L.pfx + a, len), len ? rlforget::head_mask(len) : 0u, len, a};
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t m = np ? 0xFFFFFFFFu : 0u;
    for (uint32_t p = 0; p < np; p++) m = L.head[p].z < m ? L.head[p].z : m;
    L.minlen = m;
  }
  __syncthreads();
  const uint32_t minlen = L.minlen;
  const uint64_t i = (tile0 + blockIdx.x) * (uint64_t)SCAN_THREADS + threadIdx.x;
  uint32_t r = 0, hit = 0, len = 0;
  unsigned long long hits = 0;
  bool lost = false;
  if (i < nslots) {
    const Slot* s = &t.slots[i];
    SlotImg im;
    load_img_head(s, im);
    len = im.key_len();
    bool sel = im.tag() >= 2 && len >= minlen && !(q.unit_mask && !((q.unit_mask >> im.unit()) & 1u));
    if (sel && np) {
      const uint32_t dw0 = im.v[1].w;  // stem bytes 0..3
      hit = np;
      for (uint32_t p = 0; p < np; p++) {  // (in entry order: the key is counted under the lowest matching prefix)
        const uint4 h = L.head[p];
        if (!h.z || !rlforget::head_may_match(len, dw0, h.z, h.x, h.y)) continue;
        const uint8_t* ext = len > KEY_IN ? t.arena + (size_t)slot_ext(s) * 16 : nullptr;
        if (rlforget::begins_with(len, s->key, ext, L.pfx + h.w, h.z)) {
          hit = p;
          break;
        }
      }
      sel = hit != np;
    }
    if (sel) {
      const Win cur = im.cur();
      if (!(q.flags & RL_SCAN_NEWEST)) {
        bool brk = false;
        Win w{WS_INVALID, 0, 0, 0};
        for (bool any = true; export_next(t, (uint32_t)i, im, any, w.ws, &w, &brk); any = false)
          if (rec_live(q, w)) {
            r++;
            hits += w.count;
          }
        lost = brk;
      }
      if (cur.ws != WS_INVALID && rec_live(q, cur)) {
        r++;
        hits += cur.count;
      }
      lost = lost && r;  // (a key without a record left is no key of the answer)
    }
    if (cnt) cnt[i - tile0 * SCAN_THREADS] = r ? r | (hit << SCAN_PFX_SHIFT) | (lost ? SCAN_LOST : 0u) : 0u;
    if (r && byp) {
      atomicAdd(&L.hist[hit][0], 1ull);
      atomicAdd(&L.hist[hit][1], (unsigned long long)r);
      atomicAdd(&L.hist[hit][2], hits);
    }
  }
  __shared__ unsigned long long sh[SCAN_WAVES][4];
  const unsigned long long v[4] = {r, (unsigned long long)r * len, r ? 1ull : 0ull, lost ? 1ull : 0ull};
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const unsigned long long x = wave_sum(v[k]);
    if ((threadIdx.x & 63u) == 0) sh[threadIdx.x >> 6][k] = x;
  }
  __syncthreads();  // (also: every lane's histogram adds are done)
  if (threadIdx.x < 4) {
    unsigned long long x = 0;
    for (uint32_t w = 0; w < SCAN_WAVES; w++) x += sh[w][threadIdx.x];
    reinterpret_cast<unsigned long long*>(&sums[blockIdx.x])[threadIdx.x] = x;
  }
  if (byp) hist_flush(L, np, byp);
}

// Tile tile0 + blockIdx.x writes at base[blockIdx.x] (records << 32 | stem
// bytes, both relative to the span's staging o of rec_cap records / byte_cap
// bytes); a record's stem offset is byte0 + its place in the staging. A lane
// whose records would leave the staging writes nothing and raises *err: the
// counts it was cut from were another table's.
__global__ __launch_bounds__(SCAN_THREADS) void k_scan_write(const TableDev t, uint64_t nslots, uint64_t tile0,
                                                             const ScanQueryDev q, const uint32_t* __restrict__ cnt,
                                                             const unsigned long long* __restrict__ base, uint32_t byte0,
                                                             const ExportDev o, uint32_t rec_cap, uint32_t byte_cap,
                                                             unsigned long long* byp, uint32_t* err) {
  __shared__ unsigned long long hist[rlforget::PREFIX_MAX][3];
  __shared__ unsigned long long wtot[SCAN_WAVES];
  if (threadIdx.x < rlforget::PREFIX_MAX * 3) (&hist[0][0])[threadIdx.x] = 0;
  const uint64_t i = (tile0 + blockIdx.x) * (uint64_t)SCAN_THREADS + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t c = i < nslots ? cnt[i - tile0 * SCAN_THREADS] : 0u, r = c & SCAN_REC_MASK;
  const uint32_t hit = (c >> SCAN_PFX_SHIFT) & 63u;
  SlotImg im;
  uint32_t len = 0;
  if (r) {
    load_img_lo(&t.slots[i], im);
    len = im.key_len();
  }
  const unsigned long long mine = ((unsigned long long)r << 32) | ((unsigned long long)r * len);
  unsigned long long x = mine;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const unsigned long long y = __shfl_up(x, d);
    if (lane >= d) x += y;
  }
  if (lane == 63) wtot[wave] = x;
  __syncthreads();  // (also: the histogram is zero)
  if (threadIdx.x == 0) {
    unsigned long long run = base[blockIdx.x];
    for (uint32_t k = 0; k < SCAN_WAVES; k++) {
      const unsigned long long w = wtot[k];
      wtot[k] = run;  // (exclusive: the tile's base and the waves before k)
      run += w;
    }
  }
  __syncthreads();
  if (r) {
    const unsigned long long at = wtot[wave] + x - mine;
    uint32_t R = (uint32_t)(at >> 32), B = (uint32_t)at;
    if ((at >> 32) + r > rec_cap || (at & 0xFFFFFFFFull) + (unsigned long long)r * len > byte_cap) {
      atomicOr(err, 1u);
    } else {
      const Slot* s = &t.slots[i];
      const uint8_t unit = (uint8_t)im.unit();
      uint32_t j = 0;
      unsigned long long hits = 0;
      auto put = [&](const Win& w) {
        if (j == r || !rec_live(q, w)) return;  // (never more than counted)
        o.off[R] = byte0 + B;
        o.unit[R] = unit;
        o.flags[R] = (uint8_t)((c & SCAN_LOST) && j == 0 ? RL_REC_CHAIN_LOST : 0u);
        o.ws[R] = w.ws;
        o.count[R] = w.count;
        o.expire[R] = w.expire;
        o.lc[R] = w.lc;
        export_stem(t, s, len, o.stem + B);
        hits += w.count;
        R++;
        B += len;
        j++;
      };
      const Win cur = im.cur();
      if (!(q.flags & RL_SCAN_NEWEST)) {
        Win w{WS_INVALID, 0, 0, 0};
        bool brk;
        for (bool any = true; j < r && export_next(t, (uint32_t)i, im, any, w.ws, &w, &brk); any = false) put(w);
      }
      if (cur.ws != WS_INVALID) put(cur);
      if (j != r) atomicOr(err, 2u);  // (the table changed between the passes: they share one stream, so never)
      atomicAdd(&hist[hit][0], 1ull);
      atomicAdd(&hist[hit][1], (unsigned long long)j);
      atomicAdd(&hist[hit][2], hits);
    }
  }
  __syncthreads();
  const uint32_t bins = (q.np ? q.np : 1u) * 3;
  if (threadIdx.x < bins) {
    const unsigned long long h = (&hist[0][0])[threadIdx.x];
    if (h) atomicAdd(&byp[threadIdx.x], h);
  }
}

void launch_scan_count(const TableDev& t, uint64_t nslots, uint64_t tile0, uint32_t ntiles, const ScanQueryDev& q,
                       uint32_t* cnt, rlscan::TileSum* sums, unsigned long long* byp, hipStream_t st) {
  if (!ntiles || q.np > rlforget::PREFIX_MAX) return;
  k_scan_count<<<ntiles, SCAN_THREADS, 0, st>>>(t, nslots, tile0, q, cnt, sums, byp);
}

void launch_scan_write(const TableDev& t, uint64_t nslots, uint64_t tile0, uint32_t ntiles, const ScanQueryDev& q,
                       const uint32_t* cnt, const unsigned long long* base, uint32_t byte0, const ExportDev& o,
                       uint32_t rec_cap, uint32_t byte_cap, unsigned long long* byp, uint32_t* err, hipStream_t st) {
  if (!ntiles || q.np > rlforget::PREFIX_MAX) return;
  k_scan_write<<<ntiles, SCAN_THREADS, 0, st>>>(t, nslots, tile0, q, cnt, base, byte0, o, rec_cap, byte_cap, byp, err);
}

}  // namespace rl
