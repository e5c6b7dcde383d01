/* forget_layout.c — rl_stems and rl_forget_info as a C99 compiler lays them
 * out (test program, tests/test_forget_cpu.py).
 *
 * Compiled like resize_layout.c (`gcc -x c -std=c99 -Wall -Wextra -pedantic
 * -Werror` against include/ratelimit_hip.h alone); prints "S name size" per
 * struct, "F struct field offset size" per field and the constants, which the
 * test compares with the ctypes mirrors in ratelimit_amd/abi.py. The
 * redeclaration below compiles only while the header declares rl_forget with
 * exactly this signature. */
#include <stddef.h>
#include <stdio.h>

#include "ratelimit_hip.h"

extern int rl_forget(rl_ctx* ctx, const rl_stems* in, uint32_t* removed, rl_forget_info* info);

#define S(T) printf("S %s %zu\n", #T, sizeof(T))
#define F(T, f) printf("F %s %s %zu %zu\n", #T, #f, offsetof(T, f), sizeof(((T*)0)->f))

int main(void) {
  S(rl_stems);
  F(rl_stems, n); F(rl_stems, flags); F(rl_stems, stem_bytes); F(rl_stems, stem_off);
  S(rl_forget_info);
  F(rl_forget_info, slots_scanned); F(rl_forget_info, keys); F(rl_forget_info, keys_with_history);
  F(rl_forget_info, arena_bytes);

  printf("C RL_ABI_VERSION %u\n", (unsigned)RL_ABI_VERSION);
  printf("C RL_FORGET_PREFIX %u\n", (unsigned)RL_FORGET_PREFIX);
  printf("C RL_FORGET_DRY_RUN %u\n", (unsigned)RL_FORGET_DRY_RUN);
  printf("C RL_FORGET_PREFIX_MAX %u\n", (unsigned)RL_FORGET_PREFIX_MAX);
  printf("C RL_FORGET_PREFIX_BYTES %u\n", (unsigned)RL_FORGET_PREFIX_BYTES);
  return 0;
}
