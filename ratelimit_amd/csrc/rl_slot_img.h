// rl_slot_img.h — device helpers of the table scans that more than one
// translation unit compiles (rl_kernels.hip: probing, export; rl_hot.hip: the
// hot-key scan; rl_scan.hip: the prefix scan): a slot's whole 64-B sector in registers, a slot's whole stem,
// a wave's sum.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rl_device.h"
#include "rl_kernels.h"

namespace rl {

__device__ inline uint32_t u4w(const uint4& a, uint32_t j) { return j == 0 ? a.x : j == 1 ? a.y : j == 2 ? a.z : a.w; }

__device__ inline uint32_t slot_ext(const Slot* s) { return reinterpret_cast<const uint32_t*>(s)[SLOT_EXT_DW]; }

// A slot image for probing: the whole 64-B slot (tag, length, flags, cur,
// history chain head, stem bytes 0..35). Plain loads are enough: within a launch only
// CAS inserts change tags, and a lane only ever looks for its own stem, which
// no other lane inserts.
struct SlotImg {
  uint4 v[4];
  __device__ inline uint32_t dw(uint32_t k) const { return u4w(v[k >> 2], k & 3); }
  __device__ inline uint32_t tag() const { return v[0].x; }
  __device__ inline uint32_t key_len() const { return v[0].y & 0xFFFFu; }
  __device__ inline uint32_t unit() const { return (v[0].y >> 16) & 0xFFu; }
  __device__ inline uint32_t flags() const { return v[0].y >> 24; }
  __device__ inline Win cur() const { return Win{v[0].z, v[0].w, v[1].x, v[1].y}; }
  __device__ inline uint32_t ring() const { return v[1].z; }
};

__device__ inline void load_img_lo(const Slot* s, SlotImg& im) {
  const uint4* p = reinterpret_cast<const uint4*>(s);
#pragma unroll
  for (int j = 0; j < 4; j++) im.v[j] = p[j];
}

// The slot's first 32 bytes only (tag, length, unit, flags, cur, chain head):
// what a scan that never compares stems reads. dw(k >= 8) is undefined.
__device__ inline void load_img_head(const Slot* s, SlotImg& im) {
  const uint4* p = reinterpret_cast<const uint4*>(s);
  im.v[0] = p[0];
  im.v[1] = p[1];
  // both loads are issued here: left alone, the compiler sinks the second one
  // into the branch that first needs it, and a lane pays two memory round trips
  asm volatile("" : "+v"(im.v[1].x));
}

__device__ inline unsigned long long wave_sum(unsigned long long x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m);
  return x;
}

// A slot's whole stem: its inline bytes, then (longer than KEY_IN) the arena's.
__device__ inline void export_stem(const TableDev& t, const Slot* s, uint32_t len, uint8_t* dst) {
  const uint32_t il = slot_inline(len);
  for (uint32_t k = 0; k < il; k++) dst[k] = s->key[k];
  if (len > KEY_IN) {
    const uint8_t* ek = t.arena + (size_t)slot_ext(s) * 16;
    for (uint32_t k = KEY_SPLIT; k < len; k++) dst[k] = ek[k - KEY_SPLIT];
  }
}

// The walk of a slot's history chain that the export and rl_scan share (the
// checks are described at the export, rl_kernels.hip). False: the walk broke.
template <typename F>
__device__ inline bool export_walk(const TableDev& t, uint32_t si, const SlotImg& im, F f) {
  uint32_t ptr = im.ring(), tprev = im.cur().ws, saved = LOG_NONE, power = 1, lam = 0;
  for (uint32_t hops = 0; ptr != LOG_NONE; hops++) {
    const uint32_t pos = ptr & LOG_POS_MASK;
    if (hops == LOG_MAX_HOPS || pos >= t.log_cap || ptr == saved) return false;
    if (++lam == power) {
      saved = ptr;
      power <<= 1;
      lam = 0;
    }
    const uint4* e = reinterpret_cast<const uint4*>(&t.log[(size_t)(ptr >> LOG_POS_BITS) * t.log_cap + pos]);
    const uint4 a = e[0], b = e[1];
    // overwritten (owner, order), or no record of a window below its t_app
    if (a.x != si || a.y != im.tag() || a.w > tprev || b.x >= a.w) return false;
    f(Win{b.x, b.y, b.z, b.w});
    tprev = a.w;
    ptr = a.z;
  }
  return true;
}

// The newest version of the smallest logged window of slot si above lo (any:
// the smallest of all). False: none. *lost: the walk broke.
__device__ inline bool export_next(const TableDev& t, uint32_t si, const SlotImg& im, bool any, uint32_t lo, Win* out,
                                   bool* lost) {
  Win best{WS_INVALID, 0, 0, 0};
  const uint32_t cw = im.cur().ws;
  *lost = !export_walk(t, si, im, [&](const Win& w) {
    if (w.ws >= cw) return;  // (cur is the key's newest window)
    if ((any || w.ws > lo) && w.ws < best.ws) best = w;  // (<: among versions of one window, the first met)
  });
  *out = best;
  return best.ws != WS_INVALID;
}

}  // namespace rl
