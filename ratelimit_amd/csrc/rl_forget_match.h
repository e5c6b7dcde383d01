// rl_forget_match.h — does a stored stem begin with a prefix? The comparison
// of rl_forget's prefix mode over the table's stem layout, shared by the
// device scan (rl_forget.hip) and a host driver
// (tests/c_abi/forget_match_run.cpp). Plain C++; RLF_HD is
// __host__ __device__ under hipcc and empty otherwise.
//
// A stem of key_len bytes is stored as the slot keeps it (rl_device.h): at
// most KEY_IN bytes whole in Slot::key; a longer one its first KEY_SPLIT
// bytes there and bytes [KEY_SPLIT, key_len) in the long-stem arena, stem byte
// KEY_SPLIT at the arena copy's byte 0 (the slot's last stem dword is then the
// arena offset, no stem byte). A prefix of plen >= 1 bytes matches when
// key_len >= plen and the stem's first plen bytes equal the prefix's.
//
// The scan rejects most slots on their first 32 bytes, which hold the tag,
// key_len and stem bytes 0..3 (Slot::key starts at byte 28): head_may_match
// compares the stem's first dword with the prefix's under the prefix's length
// mask. It never rejects a match (bytes of that dword past a short stem are
// masked off only where the prefix is as short, and key_len >= plen is asked
// first); begins_with then decides on every byte.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RLF_HD __host__ __device__ __forceinline__
#else
#define RLF_HD inline
#endif

namespace rlforget {

constexpr uint32_t KEY_IN = 36;         // == rl::KEY_IN
constexpr uint32_t KEY_SPLIT = 32;      // == rl::KEY_SPLIT
constexpr uint32_t PREFIX_MAX = 64;     // == RL_FORGET_PREFIX_MAX
constexpr uint32_t PREFIX_BYTES = 4096; // == RL_FORGET_PREFIX_BYTES

// stem bytes kept in the slot for a stem of key_len bytes (== rl::slot_inline)
RLF_HD uint32_t inline_len(uint32_t key_len) { return key_len <= KEY_IN ? key_len : KEY_SPLIT; }

// The bytes of a prefix's first dword that the prefix covers (plen >= 1).
RLF_HD uint32_t head_mask(uint32_t plen) { return plen >= 4u ? 0xFFFFFFFFu : (1u << (8u * plen)) - 1u; }

// A prefix's first dword, little-endian like the slot's, zero above its bytes.
template <typename P>
RLF_HD uint32_t head_dword(P p, uint32_t plen) {
  uint32_t w = 0;
  for (uint32_t k = 0; k < 4u && k < plen; k++) w |= (uint32_t)p[k] << (8u * k);
  return w;
}

// The filter on a slot's first 32 bytes: dw0 = the slot's first stem dword
// (whatever lies above a stem shorter than 4 bytes), pdw0 / pmask = the
// prefix's head_dword / head_mask.
RLF_HD bool head_may_match(uint32_t key_len, uint32_t dw0, uint32_t plen, uint32_t pdw0, uint32_t pmask) {
  return key_len >= plen && ((dw0 ^ pdw0) & pmask) == 0u;
}

// inl: the slot's stem bytes (Slot::key; bytes [0, inline_len(key_len)) are
// read). ext: the stem's arena copy, read only when key_len > KEY_IN and the
// prefix reaches past KEY_SPLIT (bytes [0, plen - KEY_SPLIT)); else it may be
// null. p: the prefix's plen bytes.
template <typename I, typename E, typename P>
RLF_HD bool begins_with(uint32_t key_len, I inl, E ext, P p, uint32_t plen) {
  if (key_len < plen) return false;
  const uint32_t il = inline_len(key_len);
  const uint32_t a = plen < il ? plen : il;
  for (uint32_t k = 0; k < a; k++)
    if (inl[k] != p[k]) return false;
  for (uint32_t k = il; k < plen; k++)  // (only a stem longer than KEY_IN gets here: il == KEY_SPLIT)
    if (ext[k - KEY_SPLIT] != p[k]) return false;
  return true;
}

}  // namespace rlforget
