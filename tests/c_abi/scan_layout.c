/* scan_layout.c — rl_scan_query, rl_scan_cursor, rl_scan_prefix_sum and
 * rl_scan_info as a C99 compiler lays them out (test program,
 * tests/test_scan_cpu.py).
 *
 * Compiled like forget_layout.c (`gcc -x c -std=c99 -Wall -Wextra -pedantic
 * -Werror` against include/ratelimit_hip.h alone); prints "S name size" per
 * struct, "F struct field offset size" per field and the constants, which the
 * test compares with the ctypes mirrors in ratelimit_amd/abi.py. The
 * redeclaration below compiles only while the header declares rl_scan with
 * exactly this signature. */
#include <stddef.h>
#include <stdio.h>

#include "ratelimit_hip.h"

extern int rl_scan(rl_ctx* ctx, const rl_scan_query* q, rl_scan_cursor* cur, rl_records* out,
                   rl_scan_prefix_sum* by_prefix, rl_scan_info* info);

#define S(T) printf("S %s %zu\n", #T, sizeof(T))
#define F(T, f) printf("F %s %s %zu %zu\n", #T, #f, offsetof(T, f), sizeof(((T*)0)->f))

int main(void) {
  S(rl_scan_query);
  F(rl_scan_query, n_prefixes); F(rl_scan_query, flags); F(rl_scan_query, prefix_bytes);
  F(rl_scan_query, prefix_off); F(rl_scan_query, now); F(rl_scan_query, unit_mask); F(rl_scan_query, reserved);
  S(rl_scan_cursor);
  F(rl_scan_cursor, shard); F(rl_scan_cursor, reserved); F(rl_scan_cursor, slot);
  S(rl_scan_prefix_sum);
  F(rl_scan_prefix_sum, keys); F(rl_scan_prefix_sum, records); F(rl_scan_prefix_sum, hits);
  S(rl_scan_info);
  F(rl_scan_info, slots_scanned); F(rl_scan_info, keys); F(rl_scan_info, records); F(rl_scan_info, stem_bytes);
  F(rl_scan_info, chains_lost); F(rl_scan_info, need_records); F(rl_scan_info, need_stem_bytes);
  F(rl_scan_info, time_floor);

  printf("C RL_ABI_VERSION %u\n", (unsigned)RL_ABI_VERSION);
  printf("C RL_SCAN_NEWEST %u\n", (unsigned)RL_SCAN_NEWEST);
  printf("C RL_SCAN_LIVE %u\n", (unsigned)RL_SCAN_LIVE);
  printf("C RL_SCAN_TILE %u\n", (unsigned)RL_SCAN_TILE);
  return 0;
}
