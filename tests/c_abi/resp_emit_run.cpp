// resp_emit_run.cpp — the response emitter the kernels share
// (ratelimit_amd/csrc/rl_resp_emit.h) run on the host over a file of cases
// (test program for tests/test_respond_cpu.py; built plain and with
// -fsanitize=address,undefined). Every response is emitted into a heap block
// of exactly its counted size, so a byte past the count is a heap overflow.
//
// File (little-endian u32 words): has_keys, 3 x {len, bytes padded to 4},
// n_requests, then per request: overall_code, min_descriptor, header_limit,
// header_remaining, header_reset_s, n_descriptors, and per descriptor: code,
// match, requests_per_unit, unit, limit_remaining, reset_s.
// Output: "R <index> <size> <hex>" per request and "B <bound> <total>".
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "rl_resp_emit.h"

struct Sink {
  uint8_t* p;
  uint8_t* end;
  bool over = false;
  void put(uint8_t b) {
    if (p == end) {
      over = true;  // (reported below; the sanitizer build would also trap the store)
      return;
    }
    *p++ = b;
  }
};

struct Keys {  // rl_response_format's fields, for rlresp::format_from
  const uint8_t *limit_key, *remaining_key, *reset_key;
  uint16_t limit_key_len, remaining_key_len, reset_key_len, reserved;
};

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint8_t> buf;
  uint8_t tmp[4096];
  for (size_t n; (n = fread(tmp, 1, sizeof tmp, f)) > 0;) buf.insert(buf.end(), tmp, tmp + n);
  fclose(f);
  size_t p = 0;
  auto word = [&]() -> uint32_t {
    if (p + 4 > buf.size()) exit(3);
    uint32_t v;
    memcpy(&v, buf.data() + p, 4);
    p += 4;
    return v;
  };
  const uint32_t has_keys = word();
  std::vector<uint8_t> key[3];
  for (int k = 0; k < 3; k++) {
    const uint32_t len = word();
    if (p + ((len + 3) & ~3u) > buf.size()) return 3;
    key[k].assign(buf.data() + p, buf.data() + p + len);
    key[k].push_back(0);  // (a non-null pointer for an empty key)
    p += (len + 3) & ~3u;
  }
  Keys ks{};
  if (has_keys) {
    ks.limit_key = key[0].data();
    ks.remaining_key = key[1].data();
    ks.reset_key = key[2].data();
    ks.limit_key_len = (uint16_t)(key[0].size() - 1);
    ks.remaining_key_len = (uint16_t)(key[1].size() - 1);
    ks.reset_key_len = (uint16_t)(key[2].size() - 1);
  }
  rlresp::Format fmt;
  if (!rlresp::format_from(&ks, &fmt)) return 4;
  const uint32_t nq = word();
  uint64_t total = 0, nd_total = 0;
  for (uint32_t q = 0; q < nq; q++) {
    const uint32_t code = word(), min_desc = word(), hl = word(), hr = word(), hs = word(), nd = word();
    std::vector<rlresp::Status> st(nd);
    for (auto& a : st) {
      a.code = word();
      a.match = word();
      a.rpu = word();
      a.unit = word();
      a.rem = word();
      a.reset = word();
    }
    const uint32_t hdr = nd ? rlresp::headers_size(fmt, min_desc, hl, hr, hs) : 0;
    size_t size = rlresp::head_size(code) + hdr;
    for (const auto& a : st) size += rlresp::status_size(a);
    uint8_t* block = (uint8_t*)malloc(size ? size : 1);
    Sink s{block, block + size};
    rlresp::emit_head(code, s);
    for (const auto& a : st) rlresp::emit_status(a, s);
    if (hdr) rlresp::emit_headers(fmt, min_desc, hl, hr, hs, s);
    if (s.over || s.p != s.end) {
      fprintf(stderr, "request %u: emitted %zd of %zu counted bytes\n", q, (ptrdiff_t)(s.p - block), size);
      return 5;
    }
    printf("R %u %zu ", q, size);
    for (size_t i = 0; i < size; i++) printf("%02x", block[i]);
    printf("\n");
    free(block);
    total += size;
    nd_total += nd;
  }
  printf("B %llu %llu\n", (unsigned long long)rlresp::bound(nq, nd_total, fmt), (unsigned long long)total);
  return 0;
}
