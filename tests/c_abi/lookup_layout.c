/* lookup_layout.c — rl_keys / rl_key_state as a C99 compiler lays them out
 * (test program, tests/test_lookup_cpu.py).
 *
 * Compiled like abi_layout.c (`gcc -x c -std=c99 -Wall -Wextra -pedantic
 * -Werror` against include/ratelimit_hip.h alone); prints "S name size" per
 * struct, "F struct field offset size" per field and the ABI version, which the
 * test compares with the ctypes mirror in ratelimit_amd/abi.py. The
 * redeclaration below compiles only while the header declares rl_lookup with
 * exactly this signature. */
#include <stddef.h>
#include <stdio.h>

#include "ratelimit_hip.h"

extern int rl_lookup(rl_ctx* ctx, const rl_keys* in, rl_key_state* out);

#define S(T) printf("S %s %zu\n", #T, sizeof(T))
#define F(T, f) printf("F %s %s %zu %zu\n", #T, #f, offsetof(T, f), sizeof(((T*)0)->f))

int main(void) {
  S(rl_keys);
  F(rl_keys, n); F(rl_keys, reserved); F(rl_keys, stem_bytes); F(rl_keys, stem_off); F(rl_keys, unit); F(rl_keys, now);

  S(rl_key_state);
  F(rl_key_state, status); F(rl_key_state, found); F(rl_key_state, count); F(rl_key_state, expire);
  F(rl_key_state, lc);

  printf("C RL_ABI_VERSION %u\n", (unsigned)RL_ABI_VERSION);
  return 0;
}
