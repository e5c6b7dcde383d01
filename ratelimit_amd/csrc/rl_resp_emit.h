// rl_resp_emit.h — the canonical proto3 bytes of one
// envoy.service.ratelimit.v3.RateLimitResponse, shared by the device
// serializer (rl_resp.hip), the host twin (rl_response_serialize, rl_pack.cpp)
// and a host driver (tests/c_abi/resp_emit_run.cpp). Plain C++; RLR_HD is
// __host__ __device__ under hipcc and empty otherwise.
//
// What the reference sets (shouldRateLimitWorker, ratelimit.go:161-210):
//   RateLimitResponse: 1 overall_code, 2 statuses, 3 response_headers_to_add
//   DescriptorStatus:  1 code, 2 current_limit, 3 limit_remaining, 4 duration_until_reset
//   RateLimit:         1 requests_per_unit, 2 unit        Duration: 1 seconds
//   HeaderValue:       1 key, 2 value
// Fields in field-number order, zero scalars and empty strings omitted, minimal
// varints, a present sub-message written even when empty. Every value is a
// uint32, so every varint has at most 5 bytes and every length fits one byte.
//
// A response is   head (overall_code) | one status per descriptor | headers.
// The emitters write to a sink S with s.put(uint8_t); a sink bounds its own
// stores, the emitters never store.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RLR_HD __host__ __device__ __forceinline__
#else
#define RLR_HD inline
#endif

namespace rlresp {

constexpr uint32_t MATCH_LIMIT = 2;             // == RL_MATCH_LIMIT
constexpr uint32_t NO_DESCRIPTOR = 0xFFFFFFFFu; // == RL_NO_DESCRIPTOR
constexpr uint32_t KEY_MAX = 64;                // == RL_RESPONSE_KEY_MAX
constexpr uint32_t STATUS_MAX = 26;             // == RL_RESPONSE_STATUS_MAX: tag, length and the largest body
constexpr uint32_t HEADER_MAX = 16;             // one HeaderValue without its key's bytes

// One descriptor's answer (rl_request_result's arrays at one index).
struct Status {
  uint32_t code, match, rpu, unit, rem, reset;
};

// The three header keys (limit, remaining, reset), copied at the call.
struct Format {
  uint32_t headers;  // 0: no response_headers_to_add
  uint32_t klen[3];
  uint8_t key[3][KEY_MAX];
};

RLR_HD uint32_t varint_len(uint32_t v) { return v < (1u << 7) ? 1u : v < (1u << 14) ? 2u : v < (1u << 21) ? 3u : v < (1u << 28) ? 4u : 5u; }

RLR_HD uint32_t dec_len(uint32_t v) {
  uint32_t n = 1;
  while (v >= 10u) {
    v /= 10u;
    n++;
  }
  return n;
}

// a varint field's bytes: 0 when the value is zero (proto3 omits it)
RLR_HD uint32_t field_len(uint32_t v) { return v ? 1u + varint_len(v) : 0u; }

template <class S>
RLR_HD void put_varint(S& s, uint32_t v) {
  while (v >= 0x80u) {
    s.put((uint8_t)(v | 0x80u));
    v >>= 7;
  }
  s.put((uint8_t)v);
}

template <class S>
RLR_HD void put_field(S& s, uint8_t tag, uint32_t v) {
  if (!v) return;
  s.put(tag);
  put_varint(s, v);
}

// u32 -> decimal ASCII (strconv.FormatUint), 1 to 10 digits
template <class S>
RLR_HD void put_decimal(S& s, uint32_t v) {
  uint8_t d[10];
  uint32_t n = 0;
  do {
    d[n++] = (uint8_t)('0' + v % 10u);
    v /= 10u;
  } while (v);
  while (n) s.put(d[--n]);
}

RLR_HD uint32_t limit_len(const Status& a) { return field_len(a.rpu) + field_len(a.unit); }
RLR_HD uint32_t status_body_len(const Status& a) {
  uint32_t n = field_len(a.code) + field_len(a.rem);
  if (a.match == MATCH_LIMIT) n += 2u + limit_len(a) + 2u + field_len(a.reset);
  return n;
}

// One `statuses` element with its tag and length: at most STATUS_MAX bytes.
RLR_HD uint32_t status_size(const Status& a) { return 2u + status_body_len(a); }

template <class S>
RLR_HD void emit_status(const Status& a, S& s) {
  s.put(0x12);
  s.put((uint8_t)status_body_len(a));
  put_field(s, 0x08, a.code);
  if (a.match == MATCH_LIMIT) {
    s.put(0x12);
    s.put((uint8_t)limit_len(a));
    put_field(s, 0x08, a.rpu);
    put_field(s, 0x10, a.unit);
  }
  put_field(s, 0x18, a.rem);
  if (a.match == MATCH_LIMIT) {
    s.put(0x22);
    s.put((uint8_t)field_len(a.reset));
    put_field(s, 0x08, a.reset);
  }
}

// The request's fixed part: the head before its statuses ...
RLR_HD uint32_t head_size(uint32_t overall_code) { return field_len(overall_code); }
template <class S>
RLR_HD void emit_head(uint32_t overall_code, S& s) {
  put_field(s, 0x08, overall_code);
}

// ... and the three headers after them (min_desc: the request's minimumDescriptor).
RLR_HD uint32_t header_size(const Format& f, uint32_t k, uint32_t v) {
  return 2u + (f.klen[k] ? 2u + f.klen[k] : 0u) + 2u + dec_len(v);
}
RLR_HD uint32_t headers_size(const Format& f, uint32_t min_desc, uint32_t limit, uint32_t rem, uint32_t reset) {
  if (!f.headers || min_desc == NO_DESCRIPTOR) return 0;
  return header_size(f, 0, limit) + header_size(f, 1, rem) + header_size(f, 2, reset);
}
template <class S>
RLR_HD void emit_header(const Format& f, uint32_t k, uint32_t v, S& s) {
  s.put(0x1a);
  s.put((uint8_t)(header_size(f, k, v) - 2u));
  if (f.klen[k]) {
    s.put(0x0a);
    s.put((uint8_t)f.klen[k]);
    for (uint32_t i = 0; i < f.klen[k]; i++) s.put(f.key[k][i]);
  }
  s.put(0x12);
  s.put((uint8_t)dec_len(v));
  put_decimal(s, v);
}
template <class S>
RLR_HD void emit_headers(const Format& f, uint32_t min_desc, uint32_t limit, uint32_t rem, uint32_t reset, S& s) {
  if (!f.headers || min_desc == NO_DESCRIPTOR) return;
  emit_header(f, 0, limit, s);
  emit_header(f, 1, rem, s);
  emit_header(f, 2, reset, s);
}

// rl_response_format (any struct with its fields) -> Format. False: a key
// over KEY_MAX bytes, a NULL key with a length, or a non-zero reserved field.
// A null format, or one whose keys are all NULL, has no headers.
template <class F>
inline bool format_from(const F* f, Format* out) {
  *out = Format{};
  if (!f) return true;
  if (f->reserved) return false;
  const uint8_t* key[3] = {f->limit_key, f->remaining_key, f->reset_key};
  const uint32_t len[3] = {f->limit_key_len, f->remaining_key_len, f->reset_key_len};
  for (uint32_t k = 0; k < 3; k++) {
    if (len[k] > KEY_MAX || (!key[k] && len[k])) return false;
    if (key[k]) out->headers = 1;
    out->klen[k] = len[k];
    for (uint32_t i = 0; i < len[k]; i++) out->key[k][i] = key[k][i];
  }
  return true;
}

// rl_response_bound: no response of n_requests requests over n_descriptors descriptors is longer.
RLR_HD uint64_t bound(uint64_t n_requests, uint64_t n_descriptors, const Format& f) {
  uint64_t per = 2;
  if (f.headers) per += 3ull * HEADER_MAX + f.klen[0] + f.klen[1] + f.klen[2];
  return n_requests * per + (uint64_t)STATUS_MAX * n_descriptors;
}

}  // namespace rlresp
