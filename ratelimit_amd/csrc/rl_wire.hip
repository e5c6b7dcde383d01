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
// Untrusted bytes: every read is bounded by the message's own end, and a
// message is read only if msg_off[q] <= msg_off[q + 1] <= msgs_bytes (else
// WIRE_ERR_OFF fails the batch and the lane skips). Every store of k_wire_emit
// lands inside the range the tile's checked index entry gives the lane; a
// re-walk that would leave its counted share stops and sets MATCH_ERR_WIRE.
#include <hip/hip_runtime.h>

#include "../../include/ratelimit_hip.h"
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

__global__ __launch_bounds__(256) void k_wire_count(WireDev w) {
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
    rlwire::CountSink s;
    // (a tile with a decreasing offset fails the batch, but its other lanes may lie outside [A, B))
    const rlwire::Message m = staged && a >= A && b <= B
                                  ? rlwire::walk_message(LdsSrc{(const uint8_t*)s_in, A & ~3u}, a, b, s)
                                  : rlwire::walk_message(GlobalSrc{w.msgs}, a, b, s);
    st = m.status;
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

// One OK message walked again; true if it filled exactly its counted share.
template <class B>
__device__ __forceinline__ bool emit_message(const B& src, uint32_t a, uint32_t b, EmitSink& s, uint32_t nd,
                                             uint32_t dl, uint8_t* dom, uint32_t* hits) {
  const rlwire::Message m = rlwire::walk_message(src, a, b, s);
  if (s.bad || m.status != rlwire::ST_OK || m.n_desc != nd || s.d != s.d1 || s.e != s.e1 || s.bo != s.b1 ||
      m.dom_len != dl)
    return false;
  for (uint32_t i = 0; i < dl; i++) dom[i] = src[m.dom_pos + i];
  *hits = m.hits;
  return true;
}

__global__ __launch_bounds__(256) void k_wire_emit(WireDev w, WireOut o) {
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
    EmitSink s;
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
    uint32_t a = 0, b = 0;
    // the lane's share lies inside the tile's (no sum wrapped), its message inside the payload
    bool good = x_nd <= T.x && nd <= T.x - x_nd && x_ne <= T.y && ne <= T.y - x_ne && x_dl <= T.z &&
                dl <= T.z - x_dl && x_eb <= T.w && eb <= T.w - x_eb && lane_range(w, q, &a, &b);
    if (good)
      good = staged && a >= A && b <= B
                 ? emit_message(LdsSrc{(const uint8_t*)s_in, A & ~3u}, a, b, s, nd, dl, dom, &hits)
                 : emit_message(GlobalSrc{w.msgs}, a, b, s, nd, dl, dom, &hits);
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

void launch_wire_count(const WireDev& w, hipStream_t st) {
  if (w.tiles) k_wire_count<<<w.tiles, 256, 0, st>>>(w);
  k_wire_scan<<<1, 256, 0, st>>>(w);
}

void launch_wire_emit(const WireDev& w, const WireOut& o, hipStream_t st) {
  if (w.tiles) k_wire_emit<<<w.tiles, 256, 0, st>>>(w, o);
}

void launch_wire_code(const uint8_t* status, uint8_t* o_code, uint32_t n_req, hipStream_t st) {
  if (n_req) k_wire_code<<<(n_req + 255) / 256, 256, 0, st>>>(status, o_code, n_req);
}

}  // namespace rl
