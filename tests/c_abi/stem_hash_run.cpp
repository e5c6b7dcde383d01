// stem_hash_run.cpp — rl_device.h's host reference of the keyed stem hash
// (hash_key_of, hash_stem_host) on the host (test program,
// tests/test_bucket_aim_cpu.py): the numpy restatement in tests/bucket_aim.py
// must give the same 64 bits. Stand-alone (its own main); the HIP headers are
// only on the include path, nothing of the runtime is called or linked.
// Reads lines "<hash_seed> <stem as hex digits>" and prints one line per stem:
// the hash as 16 hex digits.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rl_device.h"

int main() {
  char line[512];
  std::vector<uint8_t> stem;
  while (std::fgets(line, sizeof line, stdin)) {
    unsigned long long seed = 0;
    char hex[400] = "";
    if (std::sscanf(line, "%llu %399s", &seed, hex) < 1) continue;
    const size_t n = std::strlen(hex) / 2;
    stem.assign(n + 1, 0);  // (never empty: data() stays a valid pointer)
    for (size_t i = 0; i < n; i++) {
      unsigned b = 0;
      if (std::sscanf(hex + 2 * i, "%2x", &b) != 1) return 2;
      stem[i] = (uint8_t)b;
    }
    const rl::HashKey key = rl::hash_key_of(seed, 0);
    std::printf("%016" PRIx64 "\n", rl::hash_stem_host(key, stem.data(), (uint32_t)n));
  }
  return 0;
}
