// maint_host_run.cpp — rl_stem_list.h and rl_shard_split.h on the host (test
// program, tests/test_maint_host_cpu.py). Stand-alone (its own main), built
// plain and under AddressSanitizer + UndefinedBehaviorSanitizer. Reads cases
// from stdin, one per line, and answers each with one line:
//
//   stem <allow_empty> <max_len> <cap> <n> <off[0]> .. <off[n]>
//     -> "<fault> <entry>"   (fault: 0 none, 1 start, 2 entry, 3 total)
//   split <n_shards> <one_shard> <n> <len[0]> .. <len[n-1]>
//     -> per shard "idx,..;off,..;<stems in hex>" joined by " | ", then
//        " # <round trips>": stem i is len[i] bytes (i * 7 + k) & 255; the
//        owner is FNV-1a of the stem mod n_shards, or n_shards - 1 for every
//        stem (one_shard); the round trips are put(take(x)) == x for a u8, a
//        u32 and an i64 column, and take of a null column reading as zeros.
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "rl_shard_split.h"
#include "rl_stem_list.h"

template <typename T>
static bool round_trip(const std::vector<rlsplit::Sub>& part, uint32_t n, T seed) {
  std::vector<T> x(n), y(n, T(-1));
  for (uint32_t i = 0; i < n; i++) x[i] = (T)(seed * (T)(i + 1));
  for (const rlsplit::Sub& s : part) {
    const std::vector<T> sub = rlsplit::take(x.data(), s.idx);
    if (sub.size() != s.idx.size()) return false;
    rlsplit::put(y.data(), s.idx, sub.data());
    for (T z : rlsplit::take((const T*)nullptr, s.idx))
      if (z != T()) return false;
  }
  return x == y;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string kind;
    in >> kind;
    if (kind == "stem") {
      int allow_empty;
      uint32_t max_len, n;
      uint64_t cap;
      in >> allow_empty >> max_len >> cap >> n;
      std::vector<uint32_t> off(n + 1);  // (exactly sized: ASan sees a read past the list)
      for (uint32_t& x : off) in >> x;
      const uint32_t* o = n ? off.data() : nullptr;  // the three rules the calls use: forget's, lookup's, scan's
      if (!allow_empty && max_len != 65535u && max_len != rlstem::ANY_LEN) return 6;
      if (allow_empty && max_len != rlstem::ANY_LEN) return 6;
      const rlstem::Bad b = allow_empty          ? rlstem::check<true, rlstem::ANY_LEN>(n, o, cap)
                            : max_len == 65535u ? rlstem::check<false, 65535u>(n, o, cap)
                                                : rlstem::check<false, rlstem::ANY_LEN>(n, o, cap);
      std::printf("%d %u\n", (int)b.what, b.what == rlstem::ENTRY ? b.i : 0u);
    } else if (kind == "split") {
      uint32_t n_shards, n;
      int one;
      in >> n_shards >> one >> n;
      std::vector<uint32_t> off(n + 1, 0);
      std::vector<uint8_t> bytes;
      for (uint32_t i = 0; i < n; i++) {
        uint32_t len;
        in >> len;
        for (uint32_t k = 0; k < len; k++) bytes.push_back((uint8_t)((i * 7 + k) & 255));
        off[i + 1] = (uint32_t)bytes.size();
      }
      auto owner = [&](const uint8_t* s, uint32_t len) {
        if (one) return n_shards - 1;
        uint32_t h = 2166136261u;
        for (uint32_t k = 0; k < len; k++) h = (h ^ s[k]) * 16777619u;
        return h % n_shards;
      };
      std::vector<rlsplit::Sub> part;
      if (!rlsplit::split(n, bytes.data(), off.data(), n_shards, owner, &part)) return 3;
      std::string out;
      for (size_t j = 0; j < part.size(); j++) {
        const rlsplit::Sub& s = part[j];
        if (j) out += " | ";
        for (size_t x = 0; x < s.idx.size(); x++) out += (x ? "," : "") + std::to_string(s.idx[x]);
        out += ";";
        for (size_t x = 0; x < s.off.size(); x++) out += (x ? "," : "") + std::to_string(s.off[x]);
        out += ";";
        char hex[3];
        for (uint8_t b : s.stems) {
          std::snprintf(hex, sizeof hex, "%02x", b);
          out += hex;
        }
      }
      const bool rt = round_trip<uint8_t>(part, n, 3) && round_trip<uint32_t>(part, n, 2654435761u) &&
                      round_trip<int64_t>(part, n, -1234567890123ll);
      // decreasing offsets are refused before the entry is read
      if (n >= 2 && off[1] > 0) {
        std::vector<uint32_t> bad(off);
        bad[2] = bad[1] - 1;
        std::vector<rlsplit::Sub> p2;
        if (rlsplit::split(n, bytes.data(), bad.data(), n_shards, owner, &p2)) return 4;
      }
      std::printf("%s # %s\n", out.c_str(), rt ? "ok" : "MISMATCH");
    } else if (!kind.empty()) {
      return 5;
    }
  }
  return 0;
}
