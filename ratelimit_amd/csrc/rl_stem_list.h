// rl_stem_list.h — the one check of a CSR stem list (n entries, n + 1 byte
// offsets) of rl_lookup, rl_forget and rl_scan: which fault, at which entry;
// the wording is the caller's (rl_maint.hip: stems_check). rl_import checks
// each record's unit and window between its offsets and the next record's and
// keeps its own loop. Plain C++, also built by tests/c_abi/maint_host_run.cpp.
#pragma once

#include <stdint.h>

namespace rlstem {

enum Fault { NONE, START, ENTRY, TOTAL };
struct Bad {
  Fault what;
  uint32_t i;  // the entry (ENTRY)
};
constexpr uint32_t ANY_LEN = 0xFFFFFFFFu;

// The first offset, then entry by entry, then the total against cap.
// AllowEmpty: an entry of 0 bytes passes; MaxLen: the longest entry in bytes.
// (Compile-time, so that each call's loop over a long list is the two or three
// integer comparisons its own loop was.)
template <bool AllowEmpty, uint32_t MaxLen>
inline Bad check(uint32_t n, const uint32_t* off, uint64_t cap) {
  if (!n) return {NONE, 0};
  if (off[0] != 0) return {START, 0};
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t a = off[i], b = off[i + 1];
    if (b < a || (b == a && !AllowEmpty) || b - a > MaxLen) return {ENTRY, i};
  }
  return {off[n] > cap ? TOTAL : NONE, n};
}

}  // namespace rlstem
