/* resize_layout.c — rl_resize_info as a C99 compiler lays it out (test
 * program, tests/test_resize_abi.py).
 *
 * Compiled like hot_layout.c (`gcc -x c -std=c99 -Wall -Wextra -pedantic
 * -Werror` against include/ratelimit_hip.h alone); prints "S name size" per
 * struct, "F struct field offset size" per field and the constants, which the
 * test compares with the ctypes mirror in ratelimit_amd/abi.py. The
 * redeclaration below compiles only while the header declares rl_resize with
 * exactly this signature. */
#include <stddef.h>
#include <stdio.h>

#include "ratelimit_hip.h"

extern int rl_resize(rl_ctx* ctx, uint64_t table_slots, rl_resize_info* info);

#define S(T) printf("S %s %zu\n", #T, sizeof(T))
#define F(T, f) printf("F %s %s %zu %zu\n", #T, #f, offsetof(T, f), sizeof(((T*)0)->f))

int main(void) {
  S(rl_resize_info);
  F(rl_resize_info, slots_before); F(rl_resize_info, slots_after); F(rl_resize_info, keys);
  F(rl_resize_info, tombstones_dropped); F(rl_resize_info, log_entries_relinked);
  F(rl_resize_info, longest_probe); F(rl_resize_info, reserved);

  printf("C RL_ABI_VERSION %u\n", (unsigned)RL_ABI_VERSION);
  return 0;
}
