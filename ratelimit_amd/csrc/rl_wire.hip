// rl_wire.hip — serialized envoy.service.ratelimit.v3.RateLimitRequest
// payloads parsed on the device (rl_do_limit_wire_async): what rl_packer_pack
// and rl_request_batch_pack build on the host, built here from the payload
// bytes as they crossed the link, then handed to the unchanged k_match chain.
//
// k_wire_count: one workgroup per tile of RL_WIRE_TILE messages, one lane per
// message. The tile's payload bytes are staged in LDS (coalesced dword loads;
// global reads when they do not fit W_IN_WORDS); each lane walks its message
// once (rl_wire_parse.h) for its status, descriptor count, entry count, domain
// length and entry bytes. k_wire_scan (one workgroup: at most max_requests /
// 256 tiles) turns the tiles' sums into the tile index of
// rl_request_batch_packed and the batch totals.
//
// k_wire_emit: one workgroup per tile, starting from its index entry. Every
// RL_WIRE_OK message is walked again and its arrays written: the byte arrays
// (entry bytes, domain bytes, key and value lengths) are assembled in LDS and
// stored as dwords, byte stores only in the dwords neighbouring tiles share.
//
// Overrides (ctxs with rl_override_rules_enable; the <true> instantiations): a
// message whose descriptors carry `limit` is walked a second time by its lane
// of k_wire_count, now that its domain is known, and every override's
// descriptorKey is hashed (SipHash-1-3 under the ctx's key, streamed from the
// payload) and looked up, find-only, in the intern table. A message with a key
// that was not found goes to the batch's miss list; k_wire_intern, one
// workgroup ordered after the previous batch's, inserts those keys and turns
// the messages it cannot serve into RL_WIRE_DEFERRED (their reqw and their
// tile's sums patched) before k_wire_scan reads the sums. k_wire_emit looks
// the ids up again, find-only, and writes the dense override arrays.
//
// Untrusted bytes: every read is bounded by the message's own end, and a
// message is read only if msg_off[q] <= msg_off[q + 1] <= msgs_bytes (else
// WIRE_ERR_OFF fails the batch and the lane skips). Every store of k_wire_emit
// lands inside the range the tile's checked index entry gives the lane; a
// re-walk that would leave its counted share stops and sets MATCH_ERR_WIRE.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/ratelimit_hip.h"
#include "rl_device.h"
#include "rl_match.h"
#include "rl_wire_parse.h"

namespace rl {

namespace {

constexpr uint32_t WT = RL_WIRE_TILE;
static_assert(WT == 256, "k_wire_*: one lane per message of a tile");
constexpr uint32_t W_IN_WORDS = 24576 / 4;   // payload bytes staged per tile (a C1 tile: about 21 KB)
constexpr uint32_t W_ENT_WORDS = 16384 / 4;  // entry bytes assembled per tile
constexpr uint32_t W_DOM_WORDS = 4096 / 4;   // domain bytes
constexpr uint32_t W_LEN_WORDS = 4096 / 4;   // key lengths; as many value lengths

struct LdsSrc {
  const uint8_t* p;  // LDS copy of [base, ...), base a multiple of 4
  uint32_t base;
  __device__ __forceinline__ uint8_t operator[](uint32_t i) const { return p[i - base]; }
};
struct GlobalSrc {
  const uint8_t* p;
  __device__ __forceinline__ uint8_t operator[](uint32_t i) const { return p[i]; }
};

__device__ __forceinline__ bool fits(uint32_t a, uint32_t b, uint32_t total, uint32_t cap) {
  return a <= b && b <= total && ((b + 3) >> 2) - (a >> 2) <= cap;
}

// Bytes [a, b) of a 4-byte aligned buffer into LDS words (word 0 = byte a & ~3);
// reads up to 3 bytes past b (the buffer's copy is padded).
__device__ __forceinline__ void stage_words(const uint8_t* src, uint32_t a, uint32_t b, uint32_t* lds) {
  const uint32_t w0 = a >> 2, nw = ((b + 3) >> 2) - w0;
  const uint32_t* s32 = reinterpret_cast<const uint32_t*>(src) + w0;
  for (uint32_t i = threadIdx.x; i < nw; i += WT) lds[i] = s32[i];
}

// Bytes [a, b) assembled in LDS (word 0 = byte a & ~3) to the 4-byte aligned
// array g: dword stores, byte stores in the two end dwords other tiles share.
__device__ __forceinline__ void flush_words(uint8_t* g, uint32_t a, uint32_t b, const uint32_t* lds) {
  const uint32_t w0 = a >> 2, nw = ((b + 3) >> 2) - w0;
  uint32_t* g32 = reinterpret_cast<uint32_t*>(g);
  for (uint32_t i = threadIdx.x; i < nw; i += WT) {
    const uint64_t lo = (uint64_t)(w0 + i) * 4;
    if (lo >= a && lo + 4 <= b) {
      g32[w0 + i] = lds[i];
    } else {
      for (uint32_t k = 0; k < 4; k++)
        if (lo + k >= a && lo + k < b) g[lo + k] = ((const uint8_t*)lds)[i * 4 + k];
    }
  }
}

// 256 lanes: wave-level inclusive scans by shuffles, then across the 4 waves.
__device__ inline uint32_t block_excl_scan(uint32_t v, uint32_t* tmp, uint32_t* total) {
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  uint32_t x = v;
#pragma unroll
  for (uint32_t o = 1; o < 64; o <<= 1) {
    const uint32_t y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  if (lane == 63) tmp[wv] = x;
  __syncthreads();
  uint32_t base = 0;
  for (uint32_t k = 0; k < wv; k++) base += tmp[k];
  *total = tmp[0] + tmp[1] + tmp[2] + tmp[3];
  __syncthreads();
  return base + x - v;
}

// The tile's payload range [A, B) and whether it is staged in LDS.
__device__ __forceinline__ bool tile_range(const WireDev& w, uint32_t t, uint32_t* A, uint32_t* B) {
  const uint32_t q0 = t * WT, q1 = min(q0 + WT, w.n_req);
  *A = w.msg_off[q0];
  *B = w.msg_off[q1];
  return fits(*A, *B, w.msgs_bytes, W_IN_WORDS);
}

// Message q's bytes [a, b), if its offsets are in order and inside the payload section.
__device__ __forceinline__ bool lane_range(const WireDev& w, uint32_t q, uint32_t* a, uint32_t* b) {
  *a = w.msg_off[q];
  *b = w.msg_off[q + 1];
  return *a <= *b && *b <= w.msgs_bytes;
}

// ---- the intern table of override stats keys (OvDev, rl_match.h) -------------

#define RL_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// descriptor_key's bytes into SipHash-1-3 (the length is known beforehand).
struct OvHash {
  StemHasher hs;
  uint64_t m;
  uint32_t n;
  __device__ __forceinline__ OvHash(const OvDev& t, uint32_t len) : hs(HashKey{t.k0, t.k1, 32}, len), m(0), n(0) {}
  __device__ __forceinline__ void sep(uint8_t c) {
    m |= (uint64_t)c << (8u * (n & 7u));
    if ((++n & 7u) == 0) {
      hs.word(m);
      m = 0;
    }
  }
  template <class B>
  __device__ __forceinline__ void bytes(const B& b, uint32_t pos, uint32_t len) {
    for (uint32_t i = 0; i < len; i++) sep(b[pos + i]);
  }
  __device__ __forceinline__ uint64_t finish() { return hs.finish(m, 32); }
};
// ... against a stored key of k_len bytes
struct OvCmp {
  const uint8_t* k;
  uint32_t k_len, i;
  bool eq;
  __device__ __forceinline__ void sep(uint8_t c) {
    if (i < k_len) eq = eq && k[i] == c;
    else eq = false;
    i++;
  }
  template <class B>
  __device__ __forceinline__ void bytes(const B& b, uint32_t pos, uint32_t len) {
    for (uint32_t j = 0; j < len && eq; j++) sep(b[pos + j]);
  }
};
// ... into the arena (k_len bytes reserved)
struct OvCopy {
  uint8_t* k;
  uint32_t k_len, i;
  __device__ __forceinline__ void sep(uint8_t c) {
    if (i < k_len) k[i] = c;
    i++;
  }
  template <class B>
  __device__ __forceinline__ void bytes(const B& b, uint32_t pos, uint32_t len) {
    for (uint32_t j = 0; j < len; j++) sep(b[pos + j]);
  }
};

// One override's key (the descriptor [p, e) of a message with domain [dp, dp + dl)): its length
// and hash; false if it is longer than OV_KEY_MAX.
template <class B>
__device__ __forceinline__ bool ov_key(const OvDev& t, const B& b, uint32_t dp, uint32_t dl, uint32_t p, uint32_t e,
                                       uint32_t* len, uint64_t* h) {
  rlwire::KeyLen L;
  rlwire::descriptor_key(b, dp, dl, p, e, L);
  if (L.n > OV_KEY_MAX) return false;
  OvHash H(t, (uint32_t)L.n);
  rlwire::descriptor_key(b, dp, dl, p, e, H);
  *len = (uint32_t)L.n;
  *h = H.finish();
  return true;
}

// A published slot word against the key: its index, or OV_NONE.
template <class B>
__device__ __forceinline__ uint32_t ov_confirm(const OvDev& t, unsigned long long v, const B& b, uint32_t dp,
                                               uint32_t dl, uint32_t p, uint32_t e, uint32_t len) {
  const uint32_t idx = (uint32_t)v - 1u;
  if (idx >= t.capacity) return OV_NONE;
  // the key's bytes, offset and length were stored before the word was published
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  const uint32_t kl = t.klen[idx], ko = t.koff[idx];
  if (kl != len || ko > t.arena_cap || kl > t.arena_cap - ko) return OV_NONE;
  OvCmp c{t.arena + ko, kl, 0, true};
  rlwire::descriptor_key(b, dp, dl, p, e, c);
  return c.eq && c.i == kl ? idx : OV_NONE;
}

// Find-only: the key's index, or OV_NONE (not there, not yet published, or the probe bound reached).
template <class B>
__device__ __forceinline__ uint32_t ov_find(const OvDev& t, const B& b, uint32_t dp, uint32_t dl, uint32_t p,
                                            uint32_t e, uint32_t len, uint64_t h) {
  const uint32_t tag = (uint32_t)(h >> 32);
  uint32_t i = (uint32_t)h & t.mask;
  for (uint32_t k = 0; k < OV_PROBE; k++, i = (i + 1u) & t.mask) {
    const unsigned long long v = __hip_atomic_load(t.slots + i, RL_AGENT);
    if (!v) return OV_NONE;
    if ((uint32_t)(v >> 32) != tag || (uint32_t)v == OV_BUSY || (uint32_t)v == OV_DEAD) continue;
    const uint32_t idx = ov_confirm(t, v, b, dp, dl, p, e, len);
    if (idx != OV_NONE) return idx;
  }
  return OV_NONE;
}

// The count walk's sink on an enabled ctx: the overrides counted, their units checked.
struct OvCountSink : rlwire::CountSink {
  uint32_t n_ov = 0;
  bool bad_unit = false;
  template <class B>
  __device__ __forceinline__ void limit(const B&, uint32_t, uint32_t, uint32_t unit, uint32_t, uint32_t) {
    n_ov++;
    if (unit < 1u || unit > 4u) bad_unit = true;
  }
};

// The second walk of a message with overrides (its domain known): every key looked up.
struct OvFindSink {
  const OvDev& t;
  uint32_t dp, dl, n_rules;
  bool too_long = false, full = false, missed = false;
  template <class B>
  __device__ __forceinline__ void entry(const B&, uint32_t, uint32_t, uint32_t, uint32_t) {}
  __device__ __forceinline__ void descriptor(uint32_t) {}
  template <class B>
  __device__ __forceinline__ void limit(const B& b, uint32_t, uint32_t, uint32_t, uint32_t p, uint32_t e) {
    uint32_t len;
    uint64_t h;
    if (!ov_key(t, b, dp, dl, p, e, &len, &h)) {
      too_long = true;
      return;
    }
    const uint32_t idx = ov_find(t, b, dp, dl, p, e, len, h);
    if (idx == OV_NONE) missed = true;
    else if (idx >= n_rules - min(n_rules, t.first_rule)) full = true;  // (first_rule + idx >= n_rules)
  }
};

template <bool OV>
__global__ __launch_bounds__(256) void k_wire_count(WireDev w, OvDev ov) {
  __shared__ uint32_t s_in[W_IN_WORDS];
  __shared__ uint32_t s_tmp[4];
  const uint32_t t = blockIdx.x, tid = threadIdx.x, q = t * WT + tid;
  uint32_t A, B;
  const bool staged = tile_range(w, t, &A, &B);
  if (staged) stage_words(w.msgs, A, B, s_in);
  __syncthreads();
  const bool valid = q < w.n_req;
  uint32_t a = 0, b = 0;
  const bool readable = valid && lane_range(w, q, &a, &b);
  if (valid && !readable) atomicOr(w.cnt + 4, WIRE_ERR_OFF);
  uint32_t st = rlwire::ST_OK, nd = 0, ne = 0, dl = 0, eb = 0;
  if (readable) {
    typename std::conditional<OV, OvCountSink, rlwire::CountSink>::type s;
    // (a tile with a decreasing offset fails the batch, but its other lanes may lie outside [A, B))
    const rlwire::Message m =
        staged && a >= A && b <= B
            ? rlwire::walk_message<LdsSrc, decltype(s), !OV>(LdsSrc{(const uint8_t*)s_in, A & ~3u}, a, b, s)
            : rlwire::walk_message<GlobalSrc, decltype(s), !OV>(GlobalSrc{w.msgs}, a, b, s);
    st = m.status;
    if constexpr (OV) {
      if (st == rlwire::ST_OK && s.n_ov) {
        if (s.bad_unit || (uint64_t)s.n_ov * (m.dom_len + 1ull) > (uint64_t)OV_WORK_X * (b - a)) {
          st = rlwire::ST_DEFERRED;
        } else {
          OvFindSink f{ov, m.dom_pos, m.dom_len, w.n_rules};
          (void)rlwire::walk_message<GlobalSrc, OvFindSink, false>(GlobalSrc{w.msgs}, a, b, f);
          if (f.too_long || f.full) {
            st = rlwire::ST_DEFERRED;
            if (f.full && !f.too_long) atomicAdd(ov.ctr + 1, 1ull);
          } else {
            atomicOr(w.cnt + 5, 1u);
            if (f.missed) {
              const uint32_t at = atomicAdd(w.cnt + 6, 1u);
              if (at < w.n_req) w.miss[at] = q;
            }
          }
        }
      }
    }
    if (st == rlwire::ST_OK) {
      nd = m.n_desc;
      ne = s.n_ent;
      dl = m.dom_len;
      eb = s.ent_bytes;
    }
  }
  if (valid) w.reqw[q] = make_uint4(nd | st << 24, ne, dl, eb);  // (OK: nd <= 65535)
  uint4 T;
  (void)block_excl_scan(nd, s_tmp, &T.x);
  (void)block_excl_scan(ne, s_tmp, &T.y);
  (void)block_excl_scan(dl, s_tmp, &T.z);
  (void)block_excl_scan(eb, s_tmp, &T.w);
  if (tid == 0) w.tsum[t] = T;
}

// k_wire_intern's walk of one listed message: every override key found or
// inserted. again: a slot another lane of this workgroup is still writing
// holds the key's tag; the message is walked again after the next barrier.
struct OvInternSink {
  const OvDev& t;
  uint32_t dp, dl, n_rules;
  bool again = false, fail = false, full = false;
  template <class B>
  __device__ __forceinline__ void entry(const B&, uint32_t, uint32_t, uint32_t, uint32_t) {}
  __device__ __forceinline__ void descriptor(uint32_t) {}
  __device__ __forceinline__ bool room(unsigned long long s, uint32_t len) const {
    return (uint32_t)(s >> 32) < t.capacity && (uint32_t)s <= t.arena_cap && len <= t.arena_cap - (uint32_t)s;
  }
  template <class B>
  __device__ __forceinline__ void limit(const B& b, uint32_t, uint32_t, uint32_t unit, uint32_t p, uint32_t e) {
    if (again || fail) return;
    uint32_t len;
    uint64_t h;
    if (unit < 1u || unit > 4u || !ov_key(t, b, dp, dl, p, e, &len, &h)) {
      fail = true;
      return;
    }
    const uint32_t tag = (uint32_t)(h >> 32);
    uint32_t i = (uint32_t)h & t.mask, idx = OV_NONE;
    for (uint32_t k = 0; k < OV_PROBE && idx == OV_NONE; k++, i = (i + 1u) & t.mask) {
      unsigned long long v = __hip_atomic_load(t.slots + i, RL_AGENT);
      if (!v) {
        // (no slot is taken for a key the table has no room for: a taken slot cannot be given back)
        if (!room(__hip_atomic_load(t.ctr, RL_AGENT), len)) break;
        const unsigned long long busy = (unsigned long long)tag << 32 | OV_BUSY;
        v = atomicCAS(t.slots + i, 0ull, busy);
        if (!v) {
          // the slot is this lane's: an id and the key's bytes, both or neither
          unsigned long long s = __hip_atomic_load(t.ctr, RL_AGENT);
          bool got = false;
          for (uint32_t tries = 0; tries < 4096u && room(s, len); tries++) {
            const unsigned long long was = atomicCAS(t.ctr, s, s + (1ull << 32) + len);
            if (was == s) {
              got = true;
              break;
            }
            s = was;
          }
          if (!got) {
            __hip_atomic_store(t.slots + i, (unsigned long long)tag << 32 | OV_DEAD, RL_AGENT);
            break;
          }
          idx = (uint32_t)(s >> 32);
          OvCopy c{t.arena + (uint32_t)s, len, 0};
          rlwire::descriptor_key(b, dp, dl, p, e, c);
          t.koff[idx] = (uint32_t)s;
          t.klen[idx] = len;
          // publish: the key's stores are complete and visible device-wide before the word is
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          __hip_atomic_store(t.slots + i, (unsigned long long)tag << 32 | (idx + 1u), RL_AGENT);
          break;
        }
      }
      if ((uint32_t)(v >> 32) != tag || (uint32_t)v == OV_DEAD) continue;
      if ((uint32_t)v == OV_BUSY) {
        again = true;
        return;
      }
      idx = ov_confirm(t, v, b, dp, dl, p, e, len);
    }
    if (idx == OV_NONE || idx >= n_rules - min(n_rules, t.first_rule)) fail = full = true;
  }
};

constexpr uint32_t OV_ROUNDS = 64;  // walks of one message before it is deferred instead

// One workgroup, after the batch's k_wire_count and the previous batch's
// k_wire_intern: the keys the count stage missed are inserted, each once. No
// lane waits for another: a lane that meets a slot still being written gives
// up the round, and every such slot is published or dead by the barrier that
// ends the round. A message that cannot be served becomes RL_WIRE_DEFERRED.
__global__ __launch_bounds__(256) void k_wire_intern(WireDev w, OvDev ov) {
  const uint32_t n_miss = min(w.cnt[6], w.n_req);
  for (uint32_t base = 0; base < n_miss; base += 256) {
    const uint32_t j = base + threadIdx.x;
    uint32_t q = 0, a = 0, b = 0;
    bool pending = j < n_miss, fail = false, full = false;
    rlwire::Message m{};
    if (pending) {
      q = w.miss[j];
      pending = q < w.n_req && (w.reqw[q].x >> 24) == rlwire::ST_OK && lane_range(w, q, &a, &b);
    }
    if (pending) {
      OvCountSink cs;
      m = rlwire::walk_message<GlobalSrc, OvCountSink, false>(GlobalSrc{w.msgs}, a, b, cs);
      if (m.status != rlwire::ST_OK || cs.bad_unit) {
        pending = false;
        fail = true;
      }
    }
    for (uint32_t round = 0; round < OV_ROUNDS; round++) {
      if (pending) {
        OvInternSink s{ov, m.dom_pos, m.dom_len, w.n_rules};
        (void)rlwire::walk_message<GlobalSrc, OvInternSink, false>(GlobalSrc{w.msgs}, a, b, s);
        pending = s.again;
        fail = s.fail;
        full = s.full;
      }
      if (!__syncthreads_or(pending)) break;
    }
    if (pending) fail = full = true;
    if (fail) {  // as if k_wire_count had deferred it: no counts in its reqw, none in its tile's sums
      const uint4 rw = w.reqw[q];
      w.reqw[q] = make_uint4(rlwire::ST_DEFERRED << 24, 0, 0, 0);
      uint32_t* ts = reinterpret_cast<uint32_t*>(w.tsum + q / WT);
      atomicSub(ts + 0, rw.x & 0xFFFFFFu);
      atomicSub(ts + 1, rw.y);
      atomicSub(ts + 2, rw.z);
      atomicSub(ts + 3, rw.w);
      if (full) atomicAdd(ov.ctr + 1, 1ull);
    }
  }
}

// One workgroup: the exclusive scan of the tiles' sums, 256 tiles at a time.
__global__ __launch_bounds__(256) void k_wire_scan(WireDev w) {
  __shared__ uint32_t s_tmp[4];
  const uint32_t tid = threadIdx.x;
  unsigned long long c0 = 0, c1 = 0, c2 = 0, c3 = 0;
  for (uint32_t c = 0; c < w.tiles; c += 256) {
    const uint32_t t = c + tid;
    const uint4 v = t < w.tiles ? w.tsum[t] : make_uint4(0, 0, 0, 0);
    uint4 T;
    const uint32_t e0 = block_excl_scan(v.x, s_tmp, &T.x), e1 = block_excl_scan(v.y, s_tmp, &T.y),
                   e2 = block_excl_scan(v.z, s_tmp, &T.z), e3 = block_excl_scan(v.w, s_tmp, &T.w);
    if (t < w.tiles)
      w.index[t] = make_uint4((uint32_t)(c0 + e0), (uint32_t)(c1 + e1), (uint32_t)(c2 + e2), (uint32_t)(c3 + e3));
    c0 += T.x;
    c1 += T.y;
    c2 += T.z;
    c3 += T.w;
  }
  if (tid == 0) {
    // (in-order offsets bound every sum by msgs_bytes < 2^32; anything else has failed the batch already)
    const bool over = (c0 | c1 | c2 | c3) >> 32;
    const uint4 tot = make_uint4((uint32_t)c0, (uint32_t)c1, (uint32_t)c2, (uint32_t)c3);
    w.index[w.tiles] = tot;
    w.cnt[0] = tot.x;
    w.cnt[1] = tot.y;
    w.cnt[2] = tot.z;
    w.cnt[3] = tot.w;
    if (over) w.cnt[4] |= WIRE_ERR_SUM;
    w.desc_first[w.n_req] = tot.x;
  }
}

// The re-walk's sink: one message's arrays, every store inside the lane's share
// [d, d1) x [e, e1) x [bo, b1). The byte and length arrays are LDS regions
// (index = array index - bias) or the global arrays (bias 0).
struct EmitSink {
  uint32_t q;
  uint32_t d, d1, e, e1, bo, b1;
  uint32_t de, db;  // the current descriptor's first entry and byte
  uint32_t* req;
  uint32_t* ent_first;
  uint32_t* desc_off;
  uint16_t* kl;
  uint16_t* vl;
  uint32_t len_bias;
  uint8_t* ent;
  uint32_t ent_bias;
  bool bad;
  template <class B>
  __device__ __forceinline__ void entry(const B& b, uint32_t kp, uint32_t kn, uint32_t vp, uint32_t vn) {
    const uint32_t len = kn + vn + 2u;
    if (bad || e >= e1 || len > b1 - bo) {
      bad = true;
      return;
    }
    uint8_t* dst = ent + (bo - ent_bias);
    for (uint32_t i = 0; i < kn; i++) dst[i] = b[kp + i];
    dst[kn] = '_';
    dst += kn + 1u;
    for (uint32_t i = 0; i < vn; i++) dst[i] = b[vp + i];
    dst[vn] = '_';
    kl[e - len_bias] = (uint16_t)kn;
    vl[e - len_bias] = (uint16_t)vn;
    e++;
    bo += len;
  }
  __device__ __forceinline__ void descriptor(uint32_t) {
    if (bad || d >= d1) {
      bad = true;
      return;
    }
    req[d] = q;
    ent_first[d] = de;
    desc_off[d] = db;
    d++;
    de = e;
    db = bo;
  }
};

// ... on an enabled ctx: the message's overrides counted.
struct OvEmitSink : EmitSink {
  uint32_t n_ov;
  template <class B>
  __device__ __forceinline__ void limit(const B&, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t) {
    n_ov++;
  }
};

// The second walk of an emitted message with overrides: the dense override
// arrays of its descriptors [d, d + nd), the ids from a find-only lookup.
struct OvStoreSink {
  const OvDev& t;
  uint32_t dp, dl, n_rules, d, nd;
  uint8_t* ovf;
  uint32_t* ov_rpu;
  uint8_t* ov_unit;
  uint32_t* ov_rule;
  bool bad;
  template <class B>
  __device__ __forceinline__ void entry(const B&, uint32_t, uint32_t, uint32_t, uint32_t) {}
  __device__ __forceinline__ void descriptor(uint32_t) {}
  template <class B>
  __device__ __forceinline__ void limit(const B& b, uint32_t ord, uint32_t rpu, uint32_t unit, uint32_t p, uint32_t e) {
    uint32_t len;
    uint64_t h;
    if (bad || ord >= nd || unit < 1u || unit > 4u || !ov_key(t, b, dp, dl, p, e, &len, &h)) {
      bad = true;
      return;
    }
    const uint32_t idx = ov_find(t, b, dp, dl, p, e, len, h);
    if (idx == OV_NONE || idx >= n_rules - min(n_rules, t.first_rule)) {
      bad = true;
      return;
    }
    ovf[d + ord] = 1;
    ov_rpu[d + ord] = rpu;
    ov_unit[d + ord] = (uint8_t)unit;
    ov_rule[d + ord] = t.first_rule + idx;
  }
};

// One OK message walked again; true if it filled exactly its counted share.
template <bool OV, class B, class S>
__device__ __forceinline__ bool emit_message(const B& src, uint32_t a, uint32_t b, S& s, uint32_t nd, uint32_t dl,
                                             uint8_t* dom, uint32_t* hits, uint32_t* dom_pos) {
  const rlwire::Message m = rlwire::walk_message<B, S, !OV>(src, a, b, s);
  *dom_pos = m.dom_pos;
  if (s.bad || m.status != rlwire::ST_OK || m.n_desc != nd || s.d != s.d1 || s.e != s.e1 || s.bo != s.b1 ||
      m.dom_len != dl)
    return false;
  for (uint32_t i = 0; i < dl; i++) dom[i] = src[m.dom_pos + i];
  *hits = m.hits;
  return true;
}

template <bool OV>
__global__ __launch_bounds__(256) void k_wire_emit(WireDev w, WireOut o, OvDev ov) {
  __shared__ uint32_t s_in[W_IN_WORDS];
  __shared__ uint32_t s_ent[W_ENT_WORDS];
  __shared__ uint32_t s_dom[W_DOM_WORDS];
  __shared__ uint32_t s_kl[W_LEN_WORDS];
  __shared__ uint32_t s_vl[W_LEN_WORDS];
  __shared__ uint32_t s_st[WT / 4];
  __shared__ uint32_t s_tmp[4];
  const uint32_t t = blockIdx.x, tid = threadIdx.x, q0 = t * WT, q = q0 + tid;
  const bool valid = q < w.n_req;
  const uint4 I0 = w.index[t], I1 = w.index[t + 1];
  const uint4 rw = valid ? w.reqw[q] : make_uint4(0, 0, 0, 0);
  const uint32_t st = rw.x >> 24, nd = rw.x & 0xFFFFFFu, ne = rw.y, dl = rw.z, eb = rw.w;
  uint4 T;
  const uint32_t x_nd = block_excl_scan(nd, s_tmp, &T.x), x_ne = block_excl_scan(ne, s_tmp, &T.y),
                 x_dl = block_excl_scan(dl, s_tmp, &T.z), x_eb = block_excl_scan(eb, s_tmp, &T.w);
  // the tile's index entry against its own sums and the totals (uniform per workgroup)
  const bool ok = I0.x <= I1.x && I0.y <= I1.y && I0.z <= I1.z && I0.w <= I1.w && I1.x <= o.tot.x &&
                  I1.y <= o.tot.y && I1.z <= o.tot.z && I1.w <= o.tot.w && I1.x - I0.x == T.x &&
                  I1.y - I0.y == T.y && I1.z - I0.z == T.z && I1.w - I0.w == T.w;
  if (!ok) {
    if (tid == 0) atomicOr(o.err, MATCH_ERR_WIRE);
    return;
  }
  uint32_t A, B;
  const bool staged = tile_range(w, t, &A, &B);
  if (staged) stage_words(w.msgs, A, B, s_in);
  const bool ent_asm = fits(I0.w, I1.w, o.tot.w, W_ENT_WORDS), dom_asm = fits(I0.z, I1.z, o.tot.z, W_DOM_WORDS);
  // (entries <= msgs_bytes / 2: twice their count fits 32 bits)
  const bool len_asm = fits(2u * I0.y, 2u * I1.y, 2u * o.tot.y, W_LEN_WORDS);
  __syncthreads();
  const uint32_t d0 = I0.x + x_nd, e0 = I0.y + x_ne, z0 = I0.z + x_dl, b0 = I0.w + x_eb;
  uint32_t hits = 0;
  if (valid && st == rlwire::ST_OK) {
    typename std::conditional<OV, OvEmitSink, EmitSink>::type s;
    if constexpr (OV) s.n_ov = 0;
    s.q = q;
    s.d = d0;
    s.d1 = d0 + nd;
    s.e = s.de = e0;
    s.e1 = e0 + ne;
    s.bo = s.db = b0;
    s.b1 = b0 + eb;
    s.req = o.req;
    s.ent_first = o.ent_first;
    s.desc_off = o.desc_off;
    s.kl = len_asm ? (uint16_t*)s_kl : o.klen;
    s.vl = len_asm ? (uint16_t*)s_vl : o.vlen;
    s.len_bias = len_asm ? (I0.y & ~1u) : 0u;
    s.ent = ent_asm ? (uint8_t*)s_ent : o.desc;
    s.ent_bias = ent_asm ? (I0.w & ~3u) : 0u;
    s.bad = false;
    uint8_t* dom = dom_asm ? (uint8_t*)s_dom + (z0 - (I0.z & ~3u)) : o.dom + z0;
    uint32_t a = 0, b = 0, dom_pos = 0;
    // the lane's share lies inside the tile's (no sum wrapped), its message inside the payload
    bool good = x_nd <= T.x && nd <= T.x - x_nd && x_ne <= T.y && ne <= T.y - x_ne && x_dl <= T.z &&
                dl <= T.z - x_dl && x_eb <= T.w && eb <= T.w - x_eb && lane_range(w, q, &a, &b);
    if (good)
      good = staged && a >= A && b <= B
                 ? emit_message<OV>(LdsSrc{(const uint8_t*)s_in, A & ~3u}, a, b, s, nd, dl, dom, &hits, &dom_pos)
                 : emit_message<OV>(GlobalSrc{w.msgs}, a, b, s, nd, dl, dom, &hits, &dom_pos);
    if constexpr (OV) {
      if (good && s.n_ov) {  // (its descriptors are [d0, d0 + nd) of the arrays: inside the lane's share)
        OvStoreSink v{ov, dom_pos, dl, w.n_rules, d0, nd, o.ovf, o.ov_rpu, o.ov_unit, o.ov_rule, false};
        (void)rlwire::walk_message<GlobalSrc, OvStoreSink, false>(GlobalSrc{w.msgs}, a, b, v);
        good = !v.bad;
      }
    }
    if (!good) atomicOr(o.err, MATCH_ERR_WIRE);
  }
  if (valid) {
    o.dom_off[q] = z0;
    o.hits[q] = hits;
    o.now[q] = w.now32[q];
    w.desc_first[q] = d0;
  }
  ((uint8_t*)s_st)[tid] = valid ? (uint8_t)st : (uint8_t)0;
  if (tid == 0) {  // (the next tile writes the same values as its first offsets)
    o.dom_off[min(q0 + WT, w.n_req)] = I1.z;
    o.ent_first[I1.x] = I1.y;
    o.desc_off[I1.x] = I1.w;
  }
  __syncthreads();
  if (ent_asm) flush_words(o.desc, I0.w, I1.w, s_ent);
  if (dom_asm) flush_words(o.dom, I0.z, I1.z, s_dom);
  if (len_asm) {
    flush_words((uint8_t*)o.klen, 2u * I0.y, 2u * I1.y, s_kl);
    flush_words((uint8_t*)o.vlen, 2u * I0.y, 2u * I1.y, s_vl);
  }
  // the tile's statuses: whole dwords (the array is padded to the tile)
  if (tid < WT / 4 && q0 + tid * 4u < w.n_req) reinterpret_cast<uint32_t*>(w.status)[q0 / 4 + tid] = s_st[tid];
}

__global__ __launch_bounds__(256) void k_wire_code(const uint8_t* __restrict__ status, uint8_t* __restrict__ o_code,
                                                   uint32_t n_req) {
  const uint32_t q = blockIdx.x * 256 + threadIdx.x;
  if (q < n_req && status[q] != rlwire::ST_OK) o_code[q] = 0;
}

}  // namespace

void launch_wire_count(const WireDev& w, hipStream_t st, const OvDev* ov, hipEvent_t ov_order, bool ov_wait) {
  if (ov && w.tiles) {
    k_wire_count<true><<<w.tiles, 256, 0, st>>>(w, *ov);
    // one k_wire_intern at a time, in batch order: count stages of consecutive batches overlap on their streams
    if (ov_wait) (void)hipStreamWaitEvent(st, ov_order, 0);
    k_wire_intern<<<1, 256, 0, st>>>(w, *ov);
    (void)hipEventRecord(ov_order, st);
  } else if (w.tiles) {
    k_wire_count<false><<<w.tiles, 256, 0, st>>>(w, OvDev{});
  }
  k_wire_scan<<<1, 256, 0, st>>>(w);
}

void launch_wire_emit(const WireDev& w, const WireOut& o, hipStream_t st, const OvDev* ov) {
  if (!w.tiles) return;
  if (ov) k_wire_emit<true><<<w.tiles, 256, 0, st>>>(w, o, *ov);
  else k_wire_emit<false><<<w.tiles, 256, 0, st>>>(w, o, OvDev{});
}

void launch_wire_code(const uint8_t* status, uint8_t* o_code, uint32_t n_req, hipStream_t st) {
  if (n_req) k_wire_code<<<(n_req + 255) / 256, 256, 0, st>>>(status, o_code, n_req);
}

}  // namespace rl
