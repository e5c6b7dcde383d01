/* hot_layout.c — rl_hot_query / rl_hot_info as a C99 compiler lays them out
 * (test program, tests/test_hot_cpu.py).
 *
 * Compiled like lookup_layout.c (`gcc -x c -std=c99 -Wall -Wextra -pedantic
 * -Werror` against include/ratelimit_hip.h alone); prints "S name size" per
 * struct, "F struct field offset size" per field and the constants, which the
 * test compares with the ctypes mirror in ratelimit_amd/abi.py. The
 * redeclaration below compiles only while the header declares rl_hot_keys with
 * exactly this signature. */
#include <stddef.h>
#include <stdio.h>

#include "ratelimit_hip.h"

extern int rl_hot_keys(rl_ctx* ctx, const rl_hot_query* q, rl_records* out, rl_hot_info* info);

#define S(T) printf("S %s %zu\n", #T, sizeof(T))
#define F(T, f) printf("F %s %s %zu %zu\n", #T, #f, offsetof(T, f), sizeof(((T*)0)->f))

int main(void) {
  S(rl_hot_query);
  F(rl_hot_query, now); F(rl_hot_query, k); F(rl_hot_query, min_count); F(rl_hot_query, unit_mask);
  F(rl_hot_query, flags);

  S(rl_hot_info);
  F(rl_hot_info, slots); F(rl_hot_info, matched); F(rl_hot_info, hits); F(rl_hot_info, above);
  F(rl_hot_info, threshold); F(rl_hot_info, reserved); F(rl_hot_info, time_floor);

  printf("C RL_ABI_VERSION %u\n", (unsigned)RL_ABI_VERSION);
  printf("C RL_HOT_BLOCKED %u\n", (unsigned)RL_HOT_BLOCKED);
  return 0;
}
