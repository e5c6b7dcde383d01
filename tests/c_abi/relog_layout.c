/* relog_layout.c — rl_history_resize_info as a C99 compiler lays it out (test
 * program, tests/test_relog_cpu.py).
 *
 * Compiled like scan_layout.c (`gcc -x c -std=c99 -Wall -Wextra -pedantic
 * -Werror` against include/ratelimit_hip.h alone); prints "S name size" per
 * struct, "F struct field offset size" per field and the constants, which the
 * test compares with the ctypes mirror in ratelimit_amd/abi.py. The
 * redeclarations below compile only while the header declares
 * rl_resize_history and rl_resize_arena with exactly these signatures. */
#include <stddef.h>
#include <stdio.h>

#include "ratelimit_hip.h"

extern int rl_resize_history(rl_ctx* ctx, uint64_t history_entries, rl_history_resize_info* info);
extern int rl_resize_arena(rl_ctx* ctx, uint64_t arena_bytes);

#define S(T) printf("S %s %zu\n", #T, sizeof(T))
#define F(T, f) printf("F %s %s %zu %zu\n", #T, #f, offsetof(T, f), sizeof(((T*)0)->f))

int main(void) {
  S(rl_history_resize_info);
  F(rl_history_resize_info, entries_before); F(rl_history_resize_info, entries_after);
  F(rl_history_resize_info, written_before); F(rl_history_resize_info, entries_kept);
  F(rl_history_resize_info, entries_dropped); F(rl_history_resize_info, chains);
  F(rl_history_resize_info, chains_lost); F(rl_history_resize_info, fill_max);
  F(rl_history_resize_info, longest_chain); F(rl_history_resize_info, reserved);

  printf("C RL_ABI_VERSION %u\n", (unsigned)RL_ABI_VERSION);
  return 0;
}
