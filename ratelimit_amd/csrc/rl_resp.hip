// rl_resp.hip — serialized envoy.service.ratelimit.v3.RateLimitResponse
// payloads written on the device (rl_do_limit_wire_respond_async): what the
// caller would marshal on the host from rl_request_result and
// rl_request_verdict, built here from the same arrays while they are still on
// the device. The bytes are those of rl_resp_emit.h, shared with the host twin.
//
// k_resp_size: one lane per descriptor for its status' length. A scan
// (hipcub) gives soff, the status bytes before each descriptor. k_resp_req:
// one lane per request for its response's length (head, its statuses' bytes
// from soff, headers; 0 unless RL_WIRE_OK). A second scan gives resp_off.
//
// k_resp_emit: one workgroup per tile of RT descriptors, one lane per
// descriptor for its status, so a request of many descriptors costs what as
// many one-descriptor requests cost. The fixed parts belong to the tile of a
// descriptor too: a request's head to the tile of its first descriptor (for a
// request without descriptors: of the descriptor that follows it, or the last
// tile), its headers to the tile of its last one. With that every tile owns
// one contiguous byte span [A, B), the spans tile the buffer in order, and
// the tile's lanes walk its requests for their fixed parts. The span is
// assembled in LDS and stored as dwords, byte stores only in the two end
// dwords neighbouring tiles share; a span over R_LDS_WORDS is stored directly.
//
// Every store is bounded by the lane's own counted piece, the tile's span and
// the buffer's capacity: answers that would serialize to more than the scans
// counted (they cannot: the same arrays are read twice on one stream) or than
// the staging holds are cut, never written past it.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "../../include/ratelimit_hip.h"
#include "rl_match.h"
#include "rl_resp_emit.h"

namespace rl {

namespace {

constexpr uint32_t RT = 256;                  // descriptors per tile
constexpr uint32_t R_LDS_WORDS = 16384 / 4;   // bytes assembled per tile (a C1 tile: about 6 KB)

// Byte `pos` of the response buffer is p[pos - bias]: p is the LDS region of a
// span (bias = the span's first dword) or the global buffer (bias 0). The bias
// is taken off the index, never off the pointer: an LDS pointer moved below
// its region is no address at all.
struct ByteSink {
  uint8_t* p;
  uint32_t bias, pos, lo, end;
  __device__ __forceinline__ void put(uint8_t b) {
    if (pos >= lo && pos < end) p[pos - bias] = b;
    pos++;
  }
};

__device__ __forceinline__ rlresp::Status status_of(const RespDev& r, uint32_t d) {
  return rlresp::Status{r.code[d], r.match[d], r.rpu[d], r.unit[d], r.rem[d], r.reset[d]};
}

__device__ __forceinline__ bool req_ok(const RespDev& r, uint32_t q) { return !r.status || r.status[q] == RL_WIRE_OK; }

// Request q's fixed part: its overall code (0: no response) and its headers' bytes.
__device__ __forceinline__ uint32_t req_fixed(const RespDev& r, const rlresp::Format& f, uint32_t q, uint32_t* hdr) {
  *hdr = 0;
  if (!req_ok(r, q)) return 0;
  if (r.desc_first[q + 1] > r.desc_first[q])
    *hdr = rlresp::headers_size(f, r.o_min[q], r.o_limit[q], r.o_rem[q], r.o_reset[q]);
  return r.o_code[q];
}

__global__ __launch_bounds__(256) void k_resp_size(RespDev r) {
  const uint32_t d = blockIdx.x * 256 + threadIdx.x;
  if (d < r.n_desc) r.soff[d] = rlresp::status_size(status_of(r, d));
  else if (d == r.n_desc) r.soff[d] = 0;
}

__global__ __launch_bounds__(256) void k_resp_req(RespDev r, rlresp::Format f) {
  const uint32_t q = blockIdx.x * 256 + threadIdx.x;
  if (q > r.n_req) return;
  uint32_t len = 0;
  if (q < r.n_req && req_ok(r, q)) {
    uint32_t hdr;
    const uint32_t code = req_fixed(r, f, q, &hdr);
    const uint32_t da = r.desc_first[q], db = r.desc_first[q + 1];
    len = rlresp::head_size(code) + hdr;
    if (da < db && db <= r.n_desc) len += r.soff[db] - r.soff[da];
  }
  r.resp_off[q] = len;
}

// The first request in [0, n_req] whose first descriptor is >= d (n_req: none).
__device__ inline uint32_t first_req_from(const RespDev& r, uint32_t d) {
  uint32_t lo = 0, hi = r.n_req;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (r.desc_first[mid] < d) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// Where descriptor d's status starts.
__device__ __forceinline__ uint32_t status_off(const RespDev& r, uint32_t d) {
  const uint32_t q = min(r.req[d], r.n_req - 1);
  return r.resp_off[q] + rlresp::head_size(req_ok(r, q) ? r.o_code[q] : 0u) + (r.soff[d] - r.soff[r.desc_first[q]]);
}

// Where the span of the tile that starts at descriptor d0 < n_desc starts; ql = first_req_from(d0).
__device__ __forceinline__ uint32_t span_start(const RespDev& r, uint32_t d0, uint32_t ql) {
  return ql < r.n_req && r.desc_first[ql] == d0 ? r.resp_off[ql] : status_off(r, d0);
}

__global__ __launch_bounds__(256) void k_resp_emit(RespDev r, rlresp::Format f) {
  __shared__ uint32_t s_out[R_LDS_WORDS];
  __shared__ uint32_t s_q[2];
  const uint32_t t = blockIdx.x, tid = threadIdx.x, d0 = t * RT;
  const bool last = t + 1 == gridDim.x;
  const uint32_t d1 = last ? r.n_desc : d0 + RT;
  if (tid == 0) s_q[0] = t ? first_req_from(r, d0) : 0u;
  if (tid == 1) s_q[1] = last ? r.n_req : first_req_from(r, d1);
  __syncthreads();
  const uint32_t ql = s_q[0], qh = s_q[1];
  const uint32_t total = min(r.resp_off[r.n_req], r.cap);
  const uint32_t A = t ? span_start(r, d0, ql) : 0u;
  const uint32_t B = last ? total : span_start(r, d1, qh);
  // (uniform per workgroup) the span in order, inside the buffer, and small enough to assemble
  const bool sane = A <= B && B <= total;
  const bool lds = sane && ((B + 3) >> 2) - (A >> 2) <= R_LDS_WORDS;
  if (!sane) return;
  uint8_t* base = lds ? (uint8_t*)s_out : r.bytes;
  const uint32_t bias = lds ? (A & ~3u) : 0u;
  // a piece of `len` bytes at `at`: what lies outside the span or past the piece is dropped
  auto sink = [&](uint32_t at, uint32_t len) {
    return ByteSink{base, bias, at, A, (uint32_t)min((uint64_t)at + len, (uint64_t)B)};
  };
  // the statuses
  const uint32_t d = d0 + tid;
  if (d < d1) {
    const rlresp::Status a = status_of(r, d);
    ByteSink s = sink(status_off(r, d), rlresp::status_size(a));
    rlresp::emit_status(a, s);
  }
  // the fixed parts: heads of the requests [ql, qh), headers of those whose last descriptor is here
  for (uint32_t q = (ql ? ql - 1 : 0u) + tid; q < qh; q += RT) {
    uint32_t hdr;
    const uint32_t code = req_fixed(r, f, q, &hdr);
    if (q >= ql && code) {
      ByteSink s = sink(r.resp_off[q], rlresp::head_size(code));
      rlresp::emit_head(code, s);
    }
    const uint32_t db = r.desc_first[q + 1];
    if (hdr && db > d0 && db <= d1 && r.resp_off[q + 1] >= hdr) {
      ByteSink s = sink(r.resp_off[q + 1] - hdr, hdr);
      rlresp::emit_headers(f, r.o_min[q], r.o_limit[q], r.o_rem[q], r.o_reset[q], s);
    }
  }
  if (!lds) return;
  __syncthreads();
  const uint32_t w0 = A >> 2, nw = ((B + 3) >> 2) - w0;
  uint32_t* g32 = reinterpret_cast<uint32_t*>(r.bytes);
  for (uint32_t i = tid; i < nw; i += RT) {
    const uint64_t lo = (uint64_t)(w0 + i) * 4;
    if (lo >= A && lo + 4 <= B) {
      g32[w0 + i] = s_out[i];
    } else {
      for (uint32_t k = 0; k < 4; k++)
        if (lo + k >= A && lo + k < B) r.bytes[lo + k] = ((const uint8_t*)s_out)[i * 4 + k];
    }
  }
}

// bytes[0, min(resp_off[n_req], cap)) to the host: dwordx4 stores where dst
// is 16-byte aligned (rl_alloc_host's arrays are), grid-stride; the tail, or
// everything to a misaligned dst, in bytes.
__global__ __launch_bounds__(256) void k_resp_to_host(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                      const uint32_t* __restrict__ total, uint32_t cap) {
  const uint32_t B = min(*total, cap);
  const uint32_t tid = blockIdx.x * 256 + threadIdx.x, stride = gridDim.x * 256;
  const uint32_t n16 = ((uintptr_t)dst & 15u) ? 0u : B / 16;
  const uint4* s4 = reinterpret_cast<const uint4*>(src);
  uint4* d4 = reinterpret_cast<uint4*>(dst);
  for (uint32_t j = tid; j < n16; j += stride) d4[j] = s4[j];
  for (uint64_t j = (uint64_t)n16 * 16 + tid; j < B; j += stride) dst[j] = src[j];
}

size_t scan_bytes(uint32_t items) {
  size_t bytes = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)items,
                                         (hipStream_t)0);
  return bytes;
}

}  // namespace

RespLayout resp_layout(uint32_t nq, uint32_t n, uint64_t bound) {
  RespLayout L;
  size_t need = 0;
  auto piece = [&need](size_t bytes) {
    const size_t o = need;
    need += (std::max<size_t>(bytes, 1) + 255) & ~(size_t)255;
    return o;
  };
  L.tmp_bytes = std::max(scan_bytes(n + 1), scan_bytes(nq + 1));
  L.cap = (size_t)bound;
  L.soff = piece((n + 1) * 4ull);
  L.resp_off = piece((nq + 1) * 4ull);
  L.tmp = piece(L.tmp_bytes);
  L.bytes = piece(L.cap + 16);  // (whole dwords are stored up to the last byte's)
  L.total = need;
  return L;
}

hipError_t launch_respond(const RespDev& r, const rlresp::Format& f, hipStream_t st) {
  k_resp_size<<<r.n_desc / 256 + 1, 256, 0, st>>>(r);
  size_t tb = r.tmp_bytes;
  hipError_t e = hipcub::DeviceScan::ExclusiveSum(r.tmp, tb, r.soff, r.soff, (int)(r.n_desc + 1), st);
  if (e != hipSuccess) return e;
  k_resp_req<<<r.n_req / 256 + 1, 256, 0, st>>>(r, f);
  e = hipcub::DeviceScan::ExclusiveSum(r.tmp, tb, r.resp_off, r.resp_off, (int)(r.n_req + 1), st);
  if (e != hipSuccess) return e;
  k_resp_emit<<<std::max(1u, (r.n_desc + RT - 1) / RT), RT, 0, st>>>(r, f);
  return hipGetLastError();
}

void launch_respond_to_host(const RespDev& r, uint8_t* dst, hipStream_t st) {
  const uint32_t g = (uint32_t)std::min<uint64_t>(std::max<uint64_t>((r.cap / 16 + 255) / 256, 1), 1024);
  k_resp_to_host<<<g, 256, 0, st>>>(r.bytes, dst, r.resp_off + r.n_req, r.cap);
}

}  // namespace rl
