// rl_match.hip — the request path on the device: the service's GetLimit per
// descriptor (src/config/config_impl.go:243-298, called from
// constructLimitsToCheck, src/service/ratelimit.go:104-143), compaction of
// the matched descriptors into the DoLimit batch (the nil / unlimited ones
// never reach DoLimit, ratelimit.go:140-143 and base_limiter.go:78-81), and
// the per-descriptor answer of shouldRateLimitWorker (ratelimit.go:176-190)
// with, on request, the rest of that function per request.
//
// k_match: one lane per descriptor. The config trie is an open-addressing
// index of (parent node, key bytes) -> node, a few KB that stays in L2; the
// walk is GetLimit's loop: look up "key_value", else "key"; a node with a
// limit answers only at the descriptor's last entry; descend while the node
// has children. Matched descriptors get a stem length; a device-wide scan of
// (matched << 40 | stem bytes) gives each its slot in the compacted batch and
// k_match_emit writes the DoLimit arrays and the stem
//   prefix ‖ domain ‖ '_' ‖ Σ(key ‖ '_' ‖ value ‖ '_')   (cache_key.go:62-71)
// (the descriptor's entry bytes already are the tail). k_match_expand maps the
// DoLimit results back to every descriptor. k_verdict / k_verdict_final reduce
// them to the answer per request (ratelimit.go:163-209): the overall code, the
// header descriptor's values and global shadow mode.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "../../include/ratelimit_hip.h"
#include "rl_match.h"

namespace rl {

namespace {

constexpr uint32_t MT = 256;                // descriptors per workgroup
constexpr uint32_t IN_WORDS = 8192 / 4;     // entry bytes staged per workgroup (LDS; 32 B per descriptor)
constexpr uint32_t OUT_WORDS = 12288 / 4;   // stem bytes assembled per workgroup (LDS; 48 B per descriptor)
constexpr unsigned long long M40 = (1ull << 40) - 1;

// Byte sources for the walk: the workgroup's entry bytes staged in LDS
// (coalesced dword loads), or global memory when a workgroup's bytes do not fit.
struct LdsBytes {
  const uint8_t* p;  // LDS copy of [base & ~3, ...)
  uint32_t base;
  __device__ __forceinline__ uint8_t operator[](uint32_t i) const { return p[i - base]; }
};
struct GlobalBytes {
  const uint8_t* p;
  __device__ __forceinline__ uint8_t operator[](uint32_t i) const { return p[i]; }
};

// Stage bytes [a, b) of a 4-byte aligned buffer into LDS words (word 0 = byte a & ~3).
// Reads may run up to 3 bytes past b (the buffers are padded).
__device__ __forceinline__ void stage_words(const uint8_t* src, uint32_t a, uint32_t b, uint32_t* lds) {
  const uint32_t w0 = a >> 2, nw = ((b + 3) >> 2) - w0;
  const uint32_t* s32 = reinterpret_cast<const uint32_t*>(src) + w0;
  for (uint32_t i = threadIdx.x; i < nw; i += MT) lds[i] = s32[i];
}

template <class R>
__device__ __forceinline__ uint64_t hash_r(int32_t parent, const R& rd, uint32_t a, uint32_t len) {
  uint64_t h = 0xcbf29ce484222325ull ^ ((uint64_t)(uint32_t)(parent + 1) * 0x9E3779B97F4A7C15ull);
  for (uint32_t i = 0; i < len; i++) {
    h ^= rd[a + i];
    h *= 0x100000001b3ull;
  }
  h ^= h >> 33;
  h *= 0xff51afd7ed558ccdull;
  h ^= h >> 33;
  return h;  // == cfg_hash over the same bytes
}

// rateLimitDescriptor.descriptors[key] lookup (a Go map of finalKey) at `parent`
// (-1: the domains map, config_impl.go:247). Collision-exact.
template <class R>
__device__ __forceinline__ int32_t cfg_find(const CfgDev& c, int32_t parent, const R& rd, uint32_t a, uint32_t len) {
  const uint64_t h = hash_r(parent, rd, a, len);
  const uint32_t tag = (uint32_t)(h >> 32);
  uint32_t pos = (uint32_t)h & c.mask;
  for (uint32_t i = 0; i <= c.mask; i++) {
    const unsigned long long e = c.index[pos];
    if (!e) return -1;
    if ((uint32_t)e == tag) {
      const uint32_t nd = (uint32_t)(e >> 32) - 1u;
      const CfgNode& N = c.nodes[nd];
      if (N.parent == parent && N.key_len == len) {
        uint32_t k = 0;
        while (k < len && c.keys[N.key_off + k] == rd[a + k]) k++;
        if (k == len) return (int32_t)nd;
      }
    }
    pos = (pos + 1) & c.mask;
  }
  return -1;
}

// GetLimit's walk (config_impl.go:268-295) over the entries [e0, e1) whose
// bytes start at b0: look up "key_value", else "key"; a node with a limit
// answers only at the last entry; descend while the node has children.
template <class R>
__device__ __forceinline__ int32_t walk(const CfgDev& c, const ReqDev& r, int32_t root, const R& rd, uint32_t b0,
                                        uint32_t e0, uint32_t e1) {
  int32_t node = root, hit = -1;
  uint32_t p = b0;
  for (uint32_t e = e0; e < e1; e++) {
    const uint32_t kl = r.klen[e], vl = r.vlen[e];
    int32_t nx = cfg_find(c, node, rd, p, kl + 1u + vl);  // key_value
    if (nx < 0) nx = cfg_find(c, node, rd, p, kl);        // key
    if (nx >= 0 && c.nodes[nx].has_limit && e == e1 - 1) hit = nx;
    if (nx >= 0 && c.nodes[nx].n_children) node = nx;
    else break;
    p += kl + vl + 2u;
  }
  return hit;
}

// Whether a workgroup's byte range [a, b) is well formed and fits `cap` LDS words.
__device__ __forceinline__ bool fits(uint32_t a, uint32_t b, uint32_t total, uint32_t cap) {
  return a <= b && b <= total && ((b + 3) >> 2) - (a >> 2) <= cap;
}

__global__ __launch_bounds__(MT) void k_match(CfgDev cg, ReqDev r, MatchBuf m) {
  __shared__ uint32_t s_in[IN_WORDS];
  extern __shared__ __attribute__((aligned(16))) uint32_t s_cfg[];  // cg.blob_words (dynamic: only what the config needs)
  const uint32_t d0 = blockIdx.x * MT, d1 = min(d0 + MT, r.n_desc);
  const uint32_t ba = r.desc_off[d0], bb = r.desc_off[d1];
  const bool staged = fits(ba, bb, r.desc_total, IN_WORDS);
  if (staged) stage_words(r.desc, ba, bb, s_in);
  // a small config (the usual case: a few KB) is walked from LDS
  CfgDev c = cg;
  if (cg.blob_words) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(cg.blob);
    for (uint32_t i = threadIdx.x; i < cg.blob_words; i += MT) s_cfg[i] = src[i];
    c.nodes = reinterpret_cast<const CfgNode*>(s_cfg);
    c.index = reinterpret_cast<const unsigned long long*>(s_cfg + cg.idx_word);
    c.prefix = reinterpret_cast<const uint8_t*>(s_cfg + cg.key_word);
    c.keys = c.prefix + cg.prefix_len;
  }
  __syncthreads();
  const uint32_t d = d0 + threadIdx.x;
  if (d >= d1) return;
  const uint32_t q = r.req[d];
  uint32_t kind = RL_MATCH_NONE, rpu = 0, rule = 0, unit = 0, shadow = 0;
  unsigned long long v = 0;
  const uint32_t e0 = r.ent_first[d], e1 = r.ent_first[d + 1];
  const uint32_t b0 = r.desc_off[d], b1 = r.desc_off[d + 1];
  bool bad = q >= r.n_req || e1 < e0 || e1 > r.n_ent || b1 < b0 || b1 > r.desc_total ||
             (staged && (b0 < ba || b1 > bb));
  if (!bad) bad = r.dom_off[q + 1] < r.dom_off[q] || r.dom_off[q + 1] > r.dom_total;
  if (!bad) {
    // entry byte layout: Σ(key ‖ '_' ‖ value ‖ '_') must fill [b0, b1)
    uint64_t tot = 0;
    for (uint32_t e = e0; e < e1; e++) tot += (uint64_t)r.klen[e] + r.vlen[e] + 2u;
    bad = tot != (uint64_t)(b1 - b0);
  }
  if (bad) {
    atomicOr(m.count + 2, MATCH_ERR_REQ);
  } else {
    const uint32_t da = r.dom_off[q], dl = r.dom_off[q + 1] - da;
    const int32_t root = cfg_find(c, -1, GlobalBytes{r.dom}, da, dl);  // this.domains[domain] (:247)
    if (root >= 0) {
      if (r.ovf && (r.ovf[d] & 1u)) {  // descriptor.GetLimit() != nil (:254-266): never shadow
        kind = RL_MATCH_LIMIT;
        rpu = r.ov_rpu[d];
        unit = r.ov_unit[d];
        rule = r.ov_rule[d];
      } else {
        const int32_t hit = staged ? walk(c, r, root, LdsBytes{(const uint8_t*)s_in, ba & ~3u}, b0, e0, e1)
                                   : walk(c, r, root, GlobalBytes{r.desc}, b0, e0, e1);
        if (hit >= 0) {
          const CfgNode& N = c.nodes[hit];
          kind = N.unlimited ? RL_MATCH_UNLIMITED : RL_MATCH_LIMIT;
          rpu = N.rpu;
          unit = N.unit;
          rule = N.rule;
          shadow = N.shadow;
        }
      }
      if (kind == RL_MATCH_LIMIT) v = (1ull << 40) | (uint64_t)(c.prefix_len + dl + 1u + (b1 - b0));
    }
  }
  m.v[d] = v;
  m.kind[d] = kind | unit << 8 | shadow << 16;
  m.rpu[d] = rpu;
  m.rule[d] = rule;
}

// s = inclusive scan of m.v. Matched descriptor d goes to position
// (s[d] >> 40) - 1 with its stem at byte (s[d] - v[d]) & (2^40 - 1). A
// workgroup's stems are contiguous in the output: they are assembled in LDS
// and written with coalesced dword stores (byte stores at the two ends, which
// neighbouring workgroups share).
__global__ __launch_bounds__(MT) void k_match_emit(CfgDev c, ReqDev r, MatchBuf m,
                                                   const unsigned long long* __restrict__ s, PackOut o) {
  __shared__ uint32_t s_in[IN_WORDS];
  __shared__ uint32_t s_out[OUT_WORDS];
  const uint32_t d0 = blockIdx.x * MT, d1 = min(d0 + MT, r.n_desc);
  const uint32_t ba = r.desc_off[d0], bb = r.desc_off[d1];
  const bool staged = fits(ba, bb, r.desc_total, IN_WORDS);
  const unsigned long long oa = (s[d0] - m.v[d0]) & M40, ob = s[d1 - 1] & M40;
  const bool assembled = ob <= o.stem_cap && ((ob + 3) >> 2) - (oa >> 2) <= OUT_WORDS;
  if (staged) stage_words(r.desc, ba, bb, s_in);
  __syncthreads();
  const uint32_t d = d0 + threadIdx.x;
  if (d < d1) {
    const unsigned long long incl = s[d], v = m.v[d];
    if (d == r.n_desc - 1) {
      const uint32_t cnt = (uint32_t)(incl >> 40);
      const unsigned long long tot = incl & M40;
      m.count[0] = cnt;
      m.count[1] = (uint32_t)(tot < 0xFFFFFFFFull ? tot : 0xFFFFFFFFull);
      if (tot > o.stem_cap) atomicOr(m.count + 2, MATCH_ERR_CAP);
      else o.off[cnt] = (uint32_t)tot;
    }
    const unsigned long long b = (incl - v) & M40, len = v & M40;
    if (v && b + len <= o.stem_cap) {  // (else MATCH_ERR_CAP, set by the last lane)
      const uint32_t j = (uint32_t)(incl >> 40) - 1u;
      const uint32_t q = r.req[d], k = m.kind[d];
      o.off[j] = (uint32_t)b;
      o.req[j] = q;
      o.unit[j] = (uint8_t)(k >> 8);
      o.flags[j] = (uint8_t)(k >> 16);  // RL_FLAG_SHADOW
      o.limit[j] = m.rpu[d];
      o.hits[j] = r.hits[q];
      o.rule[j] = m.rule[d];
      // prefix ‖ domain ‖ '_' ‖ entry bytes
      const uint32_t da = r.dom_off[q], dl = r.dom_off[q + 1] - da;
      const uint32_t b0 = r.desc_off[d], bl = r.desc_off[d + 1] - b0;
      uint8_t* dst = assembled ? (uint8_t*)s_out + (uint32_t)(b - (oa & ~3ull)) : o.stem + b;
      for (uint32_t i = 0; i < c.prefix_len; i++) dst[i] = c.prefix[i];
      dst += c.prefix_len;
      for (uint32_t i = 0; i < dl; i++) dst[i] = r.dom[da + i];
      dst[dl] = '_';
      dst += dl + 1;
      if (staged) {
        const uint8_t* src = (const uint8_t*)s_in + (b0 - (ba & ~3u));
        for (uint32_t i = 0; i < bl; i++) dst[i] = src[i];
      } else {
        for (uint32_t i = 0; i < bl; i++) dst[i] = r.desc[b0 + i];
      }
    }
  }
  if (!assembled) return;
  __syncthreads();
  const uint32_t w0 = (uint32_t)(oa >> 2), nw = (uint32_t)(((ob + 3) >> 2) - w0);
  uint32_t* out32 = reinterpret_cast<uint32_t*>(o.stem);
  for (uint32_t i = threadIdx.x; i < nw; i += MT) {
    const uint64_t lo = (uint64_t)(w0 + i) * 4;
    if (lo >= oa && lo + 4 <= ob) {
      out32[w0 + i] = s_out[i];
    } else {
      for (uint32_t k = 0; k < 4; k++)
        if (lo + k >= oa && lo + k < ob) o.stem[lo + k] = ((const uint8_t*)s_out)[i * 4 + k];
    }
  }
}

// shouldRateLimitWorker's statuses (ratelimit.go:176-190): nil limit ->
// {OK, nil, 0} (base_limiter.go:78-81); unlimited -> {OK, MaxUint32}; matched
// -> DoLimit's status.
__global__ __launch_bounds__(256) void k_match_expand(ReqDev r, MatchBuf m, const unsigned long long* __restrict__ s,
                                                      const uint8_t* __restrict__ code,
                                                      const uint32_t* __restrict__ rem,
                                                      const uint32_t* __restrict__ reset, ReqOutDev out) {
  const uint32_t d = blockIdx.x * 256 + threadIdx.x;
  if (d >= r.n_desc) return;
  const uint32_t k = m.kind[d], kind = k & 0xFFu;
  uint8_t cd = RL_CODE_OK;
  uint32_t rm = 0, rs = 0;
  if (kind == RL_MATCH_LIMIT) {
    const uint32_t j = (uint32_t)(s[d] >> 40) - 1u;
    cd = code[j];
    rm = rem[j];
    rs = reset[j];
  } else if (kind == RL_MATCH_UNLIMITED) {
    rm = 0xFFFFFFFFu;
  }
  out.code[d] = cd;
  out.rem[d] = rm;
  out.reset[d] = rs;
  out.match[d] = (uint8_t)kind;
  out.rule[d] = m.rule[d];
  out.rpu[d] = m.rpu[d];
  out.unit[d] = (uint8_t)(k >> 8);
}

// The rest of shouldRateLimitWorker (ratelimit.go:163-209, customHeadersEnabled):
// OverallCode and the descriptor "closest to its limit" behind the
// RateLimit-* headers. The reference's loop is order-dependent, but its result
// has a closed form over a request's descriptors (contiguous in the batch):
//   any OVER_LIMIT status  -> OVER_LIMIT, minimumDescriptor = the LAST such d
//                             (:185-190 overwrite it and pin minLimitRemaining to 0);
//   otherwise              -> OK, minimumDescriptor = the FIRST limited d with
//                             the smallest LimitRemaining (strict <, :173), none
//                             below MaxUint32 -> nil (minLimitRemaining starts there, :166).
// Both are order-free reductions: over[q] = max(d + 1) and
// min[q] = min(remaining << 32 | d), kept as ~min so that one zeroing
// initialises both.
//
// k_verdict: one lane per descriptor. A segmented inclusive scan over the
// wave's runs of equal req_idx (cross-lane shuffles; a lane combines with the
// lane `off` below only inside its own run) leaves each run's reduction in its
// last lane. A run that is the whole request (the usual case) is stored
// plainly; a request that continues in a neighbouring wave gets one atomic
// pair per (wave, request) segment.
__global__ __launch_bounds__(256) void k_verdict(VerdictDev v) {
  const uint32_t d = blockIdx.x * 256 + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u;
  const bool in = d < v.n_desc;
  const uint32_t q = in ? v.req[d] : 0xFFFFFFFFu;  // (no request has this index: n_req <= 2^32 - 1)
  uint32_t ov = 0;
  unsigned long long mn = ~0ull;
  if (in && v.match[d] == RL_MATCH_LIMIT) {  // CurrentLimit != nil (:172); unlimited ones carry none
    const uint32_t rm = v.rem[d];
    if (v.code[d] == RL_CODE_OVER_LIMIT) ov = d + 1u;
    if (rm != 0xFFFFFFFFu) mn = (unsigned long long)rm << 32 | d;
  }
  const uint32_t qp = __shfl_up(q, 1);
  const unsigned long long heads = __ballot(lane == 0 || qp != q);
  const int hl = 63 - __clzll(heads & (~0ull >> (63u - lane)));  // first lane of this lane's run
  for (uint32_t off = 1; off < 64; off <<= 1) {
    const uint32_t to = __shfl_up(ov, off);
    const unsigned long long tm = __shfl_up(mn, off);
    if ((int)lane - (int)off >= hl) {
      ov = max(ov, to);
      mn = min(mn, tm);
    }
  }
  const uint32_t qn = __shfl_down(q, 1);
  if (!in || q >= v.n_req || !(lane == 63 || qn != q)) return;
  // the run's last lane: does the request go on in another wave?
  bool open = false;
  if (hl == 0) {
    const uint32_t d0 = d - lane;
    open = d0 > 0 && v.req[d0 - 1] == q;
  }
  if (!open && lane == 63) open = d + 1u < v.n_desc && v.req[d + 1] == q;
  if (!open) {
    v.over[q] = ov;
    v.inv_min[q] = ~mn;
  } else {
    if (ov) atomicMax(v.over + q, ov);
    if (mn != ~0ull) atomicMax(v.inv_min + q, ~mn);
  }
}

// One lane per request: the chosen descriptor's header values
// (rateLimitLimitHeader / RemainingHeader / ResetHeader, ratelimit.go:213-237),
// global shadow mode (:203-207) and its counter: one ballot and one atomic per wave.
__global__ __launch_bounds__(256) void k_verdict_final(VerdictDev v) {
  const uint32_t q = blockIdx.x * 256 + threadIdx.x;
  bool shadowed = false;
  if (q < v.n_req) {
    const uint32_t ov = v.over[q];
    const unsigned long long im = v.inv_min[q];
    uint32_t d = RL_NO_DESCRIPTOR, fl = 0;
    uint8_t code = RL_CODE_OK;
    if (ov) {
      d = ov - 1u;
      code = RL_CODE_OVER_LIMIT;
      fl = RL_VERDICT_OVER_LIMIT;
      if (v.opts & RL_VERDICT_OPT_GLOBAL_SHADOW) {
        code = RL_CODE_OK;
        fl |= RL_VERDICT_GLOBAL_SHADOW;
        shadowed = true;
      }
    } else if (im) {
      d = (uint32_t)~im;
    }
    const bool has = d < v.n_desc;
    v.o_min[q] = has ? d : RL_NO_DESCRIPTOR;
    v.o_limit[q] = has ? v.rpu[d] : 0u;
    v.o_rem[q] = has ? v.rem[d] : 0u;
    v.o_reset[q] = has ? v.reset[d] : 0u;
    v.o_code[q] = code;
    v.o_flags[q] = (uint8_t)fl;
  }
  const unsigned long long b = __ballot(shadowed);
  if ((threadIdx.x & 63u) == 0 && b) atomicAdd(v.shadow, (unsigned long long)__popcll(b));
}

// ---- k_unpack_requests: a one-buffer request batch (rl_request_batch_packed)
// -> the offset arrays ReqDev reads (dom_off, req, ent_first, desc_off), the
// 64-bit clocks and the dense override arrays; lengths and bytes stay where
// the copy put them. Workgroups [0, tiles): one per tile of RQ_TILE requests,
// one lane per request, following k_unpack_prefixed: the tile's index entry
// gives its first descriptor, entry, domain byte and entry byte, so tiles are
// independent. The entry against the next one, the totals and the tile's own
// descriptor and domain-byte sums is checked before anything is written; the
// entry and entry-byte sums accumulate over the descriptor chunks, every lane
// bounded by the tile's checked end, and are compared at the end. Every store
// lands at a descriptor index in [I0.x, I1.x] or a request index of the tile,
// inside arrays of n + 1 and nq + 1 elements (the totals are host-checked), so
// a malformed tile fails the batch (MATCH_ERR_UNPACK) and never writes outside
// it. Workgroups from `tiles` on: one lane per override of the sparse list,
// scattered into the dense arrays (zeroed on the stream before the launch).
constexpr uint32_t RQ_TILE = RL_REQUESTS_TILE;
static_assert(RQ_TILE == 256, "k_unpack_requests: one lane per request of a tile");

// 256 lanes: wave-level inclusive scans by shuffles, then across the 4 waves.
template <typename T>
__device__ inline T block_excl_scan(T v, T* tmp, T* total) {
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  T x = v;
#pragma unroll
  for (uint32_t o = 1; o < 64; o <<= 1) {
    const T y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  if (lane == 63) tmp[wv] = x;
  __syncthreads();
  T base = 0;
  for (uint32_t k = 0; k < wv; k++) base += tmp[k];
  *total = tmp[0] + tmp[1] + tmp[2] + tmp[3];
  __syncthreads();
  return base + x - v;
}

struct UnpackReq {
  uint32_t nq, n, tiles, n_ov;
  uint4 tot;  // {n, n_ent, domain bytes, entry bytes}: the index's last entry, host-checked
  const uint32_t* reqw;
  const uint32_t* now32;
  const uint16_t* descw;
  const uint16_t* klen;
  const uint16_t* vlen;
  const uint32_t* index;
  const rl_request_override* ov;
  uint32_t* dom_off;
  int64_t* now;
  uint32_t* req;
  uint32_t* ent_first;
  uint32_t* desc_off;
  uint8_t* ovf;
  uint32_t* ov_rpu;
  uint8_t* ov_unit;
  uint32_t* ov_rule;
  uint32_t* err;  // MatchBuf::count + 2
};

__global__ __launch_bounds__(256) void k_unpack_requests(UnpackReq u) {
  __shared__ uint32_t s_tmp[3][4];
  __shared__ unsigned long long s_tmp64[4];
  __shared__ uint32_t s_first[RQ_TILE + 1];
  const uint32_t tid = threadIdx.x;
  if (blockIdx.x >= u.tiles) {  // the overrides
    const uint32_t i = (blockIdx.x - u.tiles) * 256 + tid;
    if (i >= u.n_ov) return;
    const rl_request_override o = u.ov[i];
    const bool bad = o.descriptor >= u.n || (i && u.ov[i - 1].descriptor >= o.descriptor) ||
                     (o.reserved[0] | o.reserved[1] | o.reserved[2]) != 0;
    if (bad) {
      atomicOr(u.err, MATCH_ERR_UNPACK);
      return;
    }
    u.ovf[o.descriptor] = 1;
    u.ov_rpu[o.descriptor] = o.requests_per_unit;
    u.ov_unit[o.descriptor] = o.unit;
    u.ov_rule[o.descriptor] = o.rule_id;
    return;
  }
  const uint32_t t = blockIdx.x, q0 = t * RQ_TILE, q = q0 + tid;
  const uint32_t* ix = u.index + 4ull * t;  // (a section is 4-byte aligned only)
  const uint4 I0 = make_uint4(ix[0], ix[1], ix[2], ix[3]), I1 = make_uint4(ix[4], ix[5], ix[6], ix[7]);
  const uint32_t rw = q < u.nq ? u.reqw[q] : 0u;
  const uint32_t nd = rw & 0xFFFFu, dl = rw >> 16;
  uint32_t T_nd, T_dl;
  const uint32_t e_nd = block_excl_scan(nd, s_tmp[0], &T_nd);
  const uint32_t e_dl = block_excl_scan(dl, s_tmp[1], &T_dl);
  // the tile's entry against its own sums and the totals (uniform per block)
  const bool ok = I0.x <= I1.x && I0.y <= I1.y && I0.z <= I1.z && I0.w <= I1.w && I1.x <= u.tot.x &&
                  I1.y <= u.tot.y && I1.z <= u.tot.z && I1.w <= u.tot.w && I1.x - I0.x == T_nd && I1.z - I0.z == T_dl;
  if (!ok) {
    if (tid == 0) atomicOr(u.err, MATCH_ERR_UNPACK);
    return;
  }
  s_first[tid] = I0.x + e_nd;
  if (tid == 0) s_first[RQ_TILE] = I1.x;
  if (q < u.nq) {
    u.now[q] = u.now32[q];
    u.dom_off[q] = I0.z + e_dl;
  }
  if (tid == 0) u.dom_off[min(q0 + RQ_TILE, u.nq)] = I1.z;  // (the next tile writes the same value)
  __syncthreads();
  // descriptors of the tile, 256 at a time: entry and byte offsets by block scans
  const uint32_t D = T_nd, E1 = I1.y;
  const unsigned long long span = I1.w - I0.w;
  uint32_t bad = 0;
  unsigned long long carry_e = 0, carry_b = 0;
  for (uint32_t c = 0; c < D; c += 256) {
    const uint32_t j = c + tid, d = I0.x + j;
    uint32_t ne = 0;
    if (j < D) {
      ne = u.descw[d];
      // request of descriptor d: the last tile request whose first descriptor <= d
      uint32_t lo = 0, hi = RQ_TILE;  // s_first[lo] <= d < s_first[hi]
      while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (s_first[mid] <= d) lo = mid;
        else hi = mid;
      }
      u.req[d] = q0 + lo;
    }
    uint32_t T_e;
    const uint32_t e_e = block_excl_scan(ne, s_tmp[2], &T_e);
    const unsigned long long ef64 = (unsigned long long)I0.y + carry_e + e_e;
    const uint32_t ef = (uint32_t)ef64;
    unsigned long long bl = 0;
    if (j < D) {
      if (ef64 + ne > E1) {  // (past the tile's checked end)
        bad = 1;
      } else {
        for (uint32_t e = ef; e < ef + ne; e++) bl += (unsigned long long)u.klen[e] + u.vlen[e] + 2u;
        if (bl > span) {
          bad = 1;
          bl = 0;
        }
      }
    }
    unsigned long long T_b;
    const unsigned long long e_b = block_excl_scan(bl, s_tmp64, &T_b);  // (256 x span < 2^40)
    if (j < D) {
      const unsigned long long bo = carry_b + e_b;
      if (bad || bo + bl > span) {
        bad = 1;
        u.ent_first[d] = I0.y;
        u.desc_off[d] = I0.w;
      } else {
        u.ent_first[d] = ef;
        u.desc_off[d] = I0.w + (uint32_t)bo;
      }
    }
    carry_e += T_e;
    carry_b += T_b;
  }
  if (tid == 0) {
    if (carry_e != I1.y - I0.y || carry_b != span) bad = 1;
    u.ent_first[I1.x] = I1.y;  // (the next tile writes the same values as its first offsets)
    u.desc_off[I1.x] = I1.w;
  }
  if (bad) atomicOr(u.err, MATCH_ERR_UNPACK);
}

}  // namespace

void launch_unpack_requests(const rl_request_batch_packed& pb, const uint8_t* buf, uint32_t* dom_off, int64_t* now,
                            uint32_t* req, uint32_t* ent_first, uint32_t* desc_off, uint8_t* ovf, uint32_t* ov_rpu,
                            uint8_t* ov_unit, uint32_t* ov_rule, uint32_t* err, hipStream_t st) {
  UnpackReq u;
  u.nq = pb.n_requests;
  u.n = pb.n_descriptors;
  u.tiles = (pb.n_requests + RQ_TILE - 1) / RQ_TILE;
  u.n_ov = pb.n_overrides;
  const uint32_t* host_tot = reinterpret_cast<const uint32_t*>(pb.buf + pb.index) + 4ull * u.tiles;
  u.tot = make_uint4(host_tot[0], host_tot[1], host_tot[2], host_tot[3]);
  u.reqw = reinterpret_cast<const uint32_t*>(buf + pb.req);
  u.now32 = reinterpret_cast<const uint32_t*>(buf + pb.now);
  u.descw = reinterpret_cast<const uint16_t*>(buf + pb.desc);
  u.klen = reinterpret_cast<const uint16_t*>(buf + pb.key_len);
  u.vlen = reinterpret_cast<const uint16_t*>(buf + pb.value_len);
  u.index = reinterpret_cast<const uint32_t*>(buf + pb.index);
  u.ov = reinterpret_cast<const rl_request_override*>(buf + pb.overrides);
  u.dom_off = dom_off;
  u.now = now;
  u.req = req;
  u.ent_first = ent_first;
  u.desc_off = desc_off;
  u.ovf = ovf;
  u.ov_rpu = ov_rpu;
  u.ov_unit = ov_unit;
  u.ov_rule = ov_rule;
  u.err = err;
  const uint32_t g = u.tiles + (u.n_ov + 255) / 256;
  if (g) k_unpack_requests<<<g, 256, 0, st>>>(u);
}

VerdictDev verdict_view(uint32_t n_req, uint32_t n_desc, uint32_t opts, const uint32_t* req, const uint8_t* match,
                        const uint8_t* code, const uint32_t* rem, const uint32_t* reset, const uint32_t* rpu,
                        uint8_t* block) {
  const VerdictLayout L = verdict_layout(n_req);
  VerdictDev v;
  v.n_req = n_req;
  v.n_desc = n_desc;
  v.opts = opts;
  v.req = req;
  v.match = match;
  v.code = code;
  v.rem = rem;
  v.reset = reset;
  v.rpu = rpu;
  v.inv_min = (unsigned long long*)(block + L.inv_min);
  v.over = (uint32_t*)(block + L.over);
  v.shadow = (unsigned long long*)(block + L.shadow);
  v.o_min = (uint32_t*)(block + L.o_min);
  v.o_limit = (uint32_t*)(block + L.o_limit);
  v.o_rem = (uint32_t*)(block + L.o_rem);
  v.o_reset = (uint32_t*)(block + L.o_reset);
  v.o_code = block + L.o_code;
  v.o_flags = block + L.o_flags;
  return v;
}

hipError_t launch_verdict(const VerdictDev& v, uint8_t* block, hipStream_t st) {
  if (!v.n_req) return hipSuccess;
  const hipError_t e = hipMemsetAsync(block, 0, verdict_layout(v.n_req).acc_bytes(), st);
  if (e != hipSuccess) return e;
  if (v.n_desc) k_verdict<<<(v.n_desc + 255) / 256, 256, 0, st>>>(v);
  k_verdict_final<<<(v.n_req + 255) / 256, 256, 0, st>>>(v);
  return hipGetLastError();
}

size_t match_scan_bytes(uint32_t n) {
  size_t bytes = 0;
  (void)hipcub::DeviceScan::InclusiveSum(nullptr, bytes, (const unsigned long long*)nullptr,
                                         (unsigned long long*)nullptr, (int)n, (hipStream_t)0);
  return bytes;
}

void launch_match(const CfgDev& cfg, const ReqDev& r, const MatchBuf& m, const PackOut& o, void* tmp,
                  size_t tmp_bytes, hipStream_t st) {
  if (!r.n_desc) return;
  const uint32_t g = (r.n_desc + 255) / 256;
  k_match<<<g, MT, (size_t)cfg.blob_words * 4, st>>>(cfg, r, m);
  (void)hipcub::DeviceScan::InclusiveSum(tmp, tmp_bytes, m.v, m.v + r.n_desc, (int)r.n_desc, st);
  k_match_emit<<<g, MT, 0, st>>>(cfg, r, m, m.v + r.n_desc, o);
}

void launch_match_expand(const ReqDev& r, const MatchBuf& m, const uint8_t* code, const uint32_t* rem,
                         const uint32_t* reset, const ReqOutDev& out, hipStream_t st) {
  if (!r.n_desc) return;
  k_match_expand<<<(r.n_desc + 255) / 256, 256, 0, st>>>(r, m, m.v + r.n_desc, code, rem, reset, out);
}

}  // namespace rl
