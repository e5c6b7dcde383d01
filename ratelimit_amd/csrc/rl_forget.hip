// rl_forget.hip — rl_forget's prefix mode: delete every key whose stem begins
// with one of up to 64 prefixes, selected on the device (gfx950). (The keyed
// mode, one lane per stem, lives beside k_lookup in rl_kernels.hip: it shares
// that kernel's staging and probing.)
//
// k_forget_scan reads the table once, one lane per slot, grid-stride. The
// prefixes sit in LDS (at most 4 KB of bytes, and per prefix one 16-B record:
// first dword, its length mask, length, offset), where every lane reads the
// same address, a broadcast. A slot's first 32 bytes hold its tag, key_len and
// stem bytes 0..3, so most slots are rejected on those alone (tag < 2, key_len
// below the shortest prefix, first dword against each prefix's under its
// mask: rl_forget_match.h); only the survivors read the slot's other stem
// bytes, and the arena only where a prefix reaches past the inline bytes. A
// matching lane owns its slot, so the deletion is two plain stores, tag =
// TAG_TOMB and ring = LOG_NONE: what k_sweep leaves behind. No atomics touch
// the table. The counters are kept per lane and folded per workgroup, one
// atomic each (k_hot_scan's way); the per-prefix counts go through an LDS
// histogram flushed once per workgroup, its non-zero bins only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rl_device.h"
#include "rl_kernels.h"
#include "rl_slot_img.h"
#include "rl_forget_match.h"

namespace rl {

static_assert(rlforget::KEY_IN == KEY_IN && rlforget::KEY_SPLIT == KEY_SPLIT, "rl_forget_match.h restates the slot layout");
static_assert(rlforget::PREFIX_MAX == RL_FORGET_PREFIX_MAX && rlforget::PREFIX_BYTES == RL_FORGET_PREFIX_BYTES,
              "rl_forget_match.h restates the ABI's limits");
static_assert(rlforget::PREFIX_BYTES == 256 * 16, "k_forget_scan stages the prefixes with one 16-B load per lane");
static_assert(slot_key_dw(0) == 7, "stem bytes 0..3 are the last dword of the slot's first 32 bytes");

__global__ __launch_bounds__(256) void k_forget_scan(const TableDev t, uint64_t nslots, const uint8_t* __restrict__ pfx,
                                                     const uint32_t* __restrict__ poff, uint32_t np, uint32_t dry,
                                                     unsigned long long* ctr, uint32_t* removed) {
  __shared__ __attribute__((aligned(16))) uint8_t s_pfx[rlforget::PREFIX_BYTES];
  __shared__ uint32_t s_off[rlforget::PREFIX_MAX + 1];
  __shared__ uint4 s_head[rlforget::PREFIX_MAX];  // first dword, its mask, length, offset
  __shared__ uint32_t s_hist[rlforget::PREFIX_MAX];
  __shared__ uint32_t s_minlen;
  reinterpret_cast<uint4*>(s_pfx)[threadIdx.x] = reinterpret_cast<const uint4*>(pfx)[threadIdx.x];
  if (threadIdx.x <= np) s_off[threadIdx.x] = poff[threadIdx.x];
  if (threadIdx.x < rlforget::PREFIX_MAX) s_hist[threadIdx.x] = 0;
  __syncthreads();
  if (threadIdx.x < np) {
    // (the host has checked the offsets; clamped all the same: no LDS read past the prefixes)
    const uint32_t a = s_off[threadIdx.x] < rlforget::PREFIX_BYTES ? s_off[threadIdx.x] : rlforget::PREFIX_BYTES;
    const uint32_t e = s_off[threadIdx.x + 1] < rlforget::PREFIX_BYTES ? s_off[threadIdx.x + 1] : rlforget::PREFIX_BYTES;
    const uint32_t len = e > a ? e - a : 0u;
    s_head[threadIdx.x] = uint4{rlforget::head_dword(s_pfx + a, len), len ? rlforget::head_mask(len) : 0u, len, a};
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t m = 0xFFFFFFFFu;
    for (uint32_t p = 0; p < np; p++) m = s_head[p].z < m ? s_head[p].z : m;
    s_minlen = m;
  }
  __syncthreads();
  const uint32_t minlen = s_minlen;
  unsigned long long v[3] = {0, 0, 0};
  for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < nslots; i += (uint64_t)gridDim.x * 256) {
    Slot* s = &t.slots[i];
    SlotImg im;
    load_img_head(s, im);
    const uint32_t len = im.key_len();
    if (im.tag() < 2 || len < minlen) continue;
    const uint32_t dw0 = im.v[1].w;  // stem bytes 0..3
    uint32_t hit = np;
    for (uint32_t p = 0; p < np; p++) {  // (in entry order: the slot is counted under the lowest matching prefix)
      const uint4 h = s_head[p];
      if (!h.z || !rlforget::head_may_match(len, dw0, h.z, h.x, h.y)) continue;
      const uint8_t* ext = len > KEY_IN ? t.arena + (size_t)slot_ext(s) * 16 : nullptr;
      if (rlforget::begins_with(len, s->key, ext, s_pfx + h.w, h.z)) {
        hit = p;
        break;
      }
    }
    if (hit == np) continue;
    v[0] += 1;
    v[1] += im.ring() != LOG_NONE;
    if (len > KEY_IN) v[2] += (len - KEY_SPLIT + 15) / 16;
    atomicAdd(&s_hist[hit], 1u);
    if (!dry) {
      s->tag = TAG_TOMB;
      s->ring = LOG_NONE;
    }
  }
  __shared__ unsigned long long sh[4][3];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const unsigned long long x = wave_sum(v[k]);
    if (lane == 0) sh[wave][k] = x;
  }
  __syncthreads();  // (also: every lane's histogram adds are done)
  if (threadIdx.x < 3) {
    const unsigned long long x = sh[0][threadIdx.x] + sh[1][threadIdx.x] + sh[2][threadIdx.x] + sh[3][threadIdx.x];
    if (x) atomicAdd(&ctr[threadIdx.x], x);
  }
  if (threadIdx.x < np && s_hist[threadIdx.x]) atomicAdd(&removed[threadIdx.x], s_hist[threadIdx.x]);
}

void launch_forget_scan(const TableDev& t, uint64_t nslots, const uint8_t* pfx, const uint32_t* poff, uint32_t np,
                        uint32_t dry, unsigned long long* ctr, uint32_t* removed, hipStream_t st) {
  if (!np || np > rlforget::PREFIX_MAX || !nslots) return;
  const uint64_t wg = (nslots + 255) / 256;
  k_forget_scan<<<(uint32_t)(wg < 2048 ? wg : 2048), 256, 0, st>>>(t, nslots, pfx, poff, np, dry, ctr, removed);
}

}  // namespace rl
