// forget_match_run.cpp — rl_forget_match.h on the host, against memcmp (test
// program with its own main; tests/test_forget_cpu.py builds it plain and with
// -fsanitize=address,undefined).
//
// Every stem is stored the way a slot stores it: a 64-B image with key_len at
// byte 4 and the stem's inline bytes from byte 28, and, for a stem longer than
// KEY_IN, bytes [KEY_SPLIT, len) in an arena block of exactly that size on the
// heap (so a read past the stem's arena bytes is an ASan error), the image's
// last dword then holding a non-stem value. A stem of at most KEY_IN bytes
// gets no arena block (null). Stem lengths straddle the first dword,
// KEY_SPLIT, KEY_IN and a 16-byte arena granule; prefix lengths 1..40, 48, 49,
// 200. Per (stem, prefix length) the prefix is the stem's own beginning
// (equal to the stem where the lengths agree; one byte longer than the stem,
// and more, where they do not), then the same with only its last byte
// changed, with its first byte changed, and with a byte changed at each layout
// edge it covers. begins_with must equal memcmp on the flat stem, and
// head_may_match must never reject what memcmp accepts.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "rl_forget_match.h"

namespace {

struct Stored {
  std::vector<uint8_t> flat;  // the stem as the caller gave it
  uint8_t img[64];            // the slot
  uint8_t* ext;               // the arena copy, exactly len - KEY_SPLIT bytes (or null)
};

Stored store(uint32_t len, uint32_t seed) {
  Stored s;
  s.flat.resize(len);
  for (uint32_t k = 0; k < len; k++) s.flat[k] = (uint8_t)(97u + (k * 7u + seed * 13u + (k >> 3)) % 26u);
  memset(s.img, 0xEE, sizeof s.img);  // (bytes past a short stem are not zero: the mask must hide them)
  s.img[4] = (uint8_t)(len & 0xFF);
  s.img[5] = (uint8_t)(len >> 8);
  const uint32_t il = rlforget::inline_len(len);
  memcpy(s.img + 28, s.flat.data(), il);
  s.ext = nullptr;
  if (len > rlforget::KEY_IN) {
    s.ext = (uint8_t*)malloc(len - rlforget::KEY_SPLIT);
    memcpy(s.ext, s.flat.data() + rlforget::KEY_SPLIT, len - rlforget::KEY_SPLIT);
    const uint32_t off = 0x00ABCDEFu;  // (an arena offset where stem bytes 32..35 would be)
    memcpy(s.img + 60, &off, 4);
  }
  return s;
}

long checked = 0;

int check(const Stored& s, const std::vector<uint8_t>& p) {
  const uint32_t len = (uint32_t)s.flat.size(), plen = (uint32_t)p.size();
  const bool want = len >= plen && memcmp(s.flat.data(), p.data(), plen) == 0;
  // the prefix in a heap block of its own size: no read past it either
  uint8_t* pp = (uint8_t*)malloc(plen);
  memcpy(pp, p.data(), plen);
  const bool got = rlforget::begins_with(len, (const uint8_t*)s.img + 28, (const uint8_t*)s.ext, (const uint8_t*)pp, plen);
  uint32_t dw0;
  memcpy(&dw0, s.img + 28, 4);
  const bool may = rlforget::head_may_match(len, dw0, plen, rlforget::head_dword((const uint8_t*)pp, plen),
                                            rlforget::head_mask(plen));
  free(pp);
  checked++;
  if (got != want || (want && !may)) {
    printf("FAIL stem %u prefix %u: begins_with %d, memcmp %d, head_may_match %d\n", len, plen, (int)got, (int)want,
           (int)may);
    return 1;
  }
  // a prefix that differs inside its first dword (under the mask) is rejected by the filter
  if (may && !want && plen <= 4) {
    printf("FAIL stem %u prefix %u: the head filter passed a prefix of at most 4 bytes that does not match\n", len, plen);
    return 1;
  }
  return 0;
}

}  // namespace

int main() {
  const uint32_t stem_len[] = {1, 3, 4, 5, 31, 32, 33, 36, 37, 47, 48, 49, 200};
  std::vector<uint32_t> pre_len;
  for (uint32_t k = 1; k <= 40; k++) pre_len.push_back(k);
  for (uint32_t k : {48u, 49u, 200u}) pre_len.push_back(k);
  int bad = 0;
  uint32_t seed = 0;
  for (uint32_t len : stem_len) {
    Stored s = store(len, ++seed);
    for (uint32_t plen : pre_len) {
      // the stem's own beginning, continued past its end where the prefix is longer
      std::vector<uint8_t> p(plen);
      for (uint32_t k = 0; k < plen; k++) p[k] = k < len ? s.flat[k] : (uint8_t)(48u + k % 10u);
      bad += check(s, p);
      std::vector<uint32_t> at = {plen - 1, 0};
      for (uint32_t e : {3u, 4u, 31u, 32u, 35u, 36u, 47u, 48u})
        if (e < plen) at.push_back(e);
      for (uint32_t k : at) {  // one byte changed: the last, the first, each edge
        std::vector<uint8_t> q = p;
        q[k] ^= 0x01;
        bad += check(s, q);
      }
    }
    // the prefix equal to the stem, and one byte longer
    std::vector<uint8_t> whole = s.flat;
    bad += check(s, whole);
    whole.push_back('_');
    bad += check(s, whole);
    free(s.ext);
  }
  // masks and head dwords
  if (rlforget::head_mask(1) != 0xFFu || rlforget::head_mask(3) != 0xFFFFFFu || rlforget::head_mask(4) != 0xFFFFFFFFu ||
      rlforget::head_mask(200) != 0xFFFFFFFFu) {
    printf("FAIL head_mask\n");
    bad++;
  }
  const uint8_t abcde[] = {'a', 'b', 'c', 'd', 'e'};
  if (rlforget::head_dword(abcde, 2) != 0x6261u || rlforget::head_dword(abcde, 5) != 0x64636261u) {
    printf("FAIL head_dword\n");
    bad++;
  }
  if (bad) return 1;
  printf("ok %ld\n", checked);
  return 0;
}
