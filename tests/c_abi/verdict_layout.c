/* verdict_layout.c — rl_request_verdict as a C99 compiler lays it out (test
 * program, tests/test_verdict_cpu.py).
 *
 * Compiled like lookup_layout.c (`gcc -x c -std=c99 -Wall -Wextra -pedantic
 * -Werror` against include/ratelimit_hip.h alone); prints "S name size" per
 * struct, "F struct field offset size" per field and the constants, which the
 * test compares with the ctypes mirror in ratelimit_amd/abi.py. The
 * redeclarations below compile only while the header declares both entry
 * points with exactly these signatures. */
#include <stddef.h>
#include <stdio.h>

#include "ratelimit_hip.h"

extern int rl_do_limit_requests_verdict(rl_ctx* ctx, const rl_request_batch* in, rl_request_result* out,
                                        uint32_t opts, rl_request_verdict* verdict);
extern int rl_debug_verdict(rl_ctx* ctx, uint32_t n_requests, uint32_t n_descriptors, const uint32_t* req_idx,
                            const uint8_t* match, const uint8_t* code, const uint32_t* limit_remaining,
                            const uint32_t* reset_s, const uint32_t* requests_per_unit, uint32_t opts,
                            rl_request_verdict* verdict);

#define S(T) printf("S %s %zu\n", #T, sizeof(T))
#define F(T, f) printf("F %s %s %zu %zu\n", #T, #f, offsetof(T, f), sizeof(((T*)0)->f))
#define K(c) printf("C %s %lu\n", #c, (unsigned long)(c))

int main(void) {
  S(rl_request_verdict);
  F(rl_request_verdict, overall_code); F(rl_request_verdict, flags); F(rl_request_verdict, min_descriptor);
  F(rl_request_verdict, header_limit); F(rl_request_verdict, header_remaining);
  F(rl_request_verdict, header_reset_s); F(rl_request_verdict, global_shadow);

  K(RL_ABI_VERSION);
  K(RL_NO_DESCRIPTOR);
  K(RL_VERDICT_OVER_LIMIT);
  K(RL_VERDICT_GLOBAL_SHADOW);
  K(RL_VERDICT_OPT_GLOBAL_SHADOW);
  return 0;
}
