/* requests_packed_layout.c — rl_request_override / rl_request_batch_packed as a
 * C99 compiler lays them out (test program, tests/test_requests_packed_cpu.py).
 *
 * Compiled like lookup_layout.c (`gcc -x c -std=c99 -Wall -Wextra -pedantic
 * -Werror` against include/ratelimit_hip.h alone); prints "S name size" per
 * struct, "F struct field offset size" per field and the constants, which the
 * test compares with the ctypes mirror in ratelimit_amd/abi.py. The
 * redeclarations below compile only while the header declares both functions
 * with exactly these signatures. */
#include <stddef.h>
#include <stdio.h>

#include "ratelimit_hip.h"

extern int rl_request_batch_pack(const rl_request_batch* in, uint8_t* buf, uint64_t buf_cap,
                                 rl_request_batch_packed* out);
extern int rl_do_limit_requests_packed_async(rl_ctx* ctx, const rl_request_batch_packed* in, rl_request_result* out,
                                             uint32_t opts, rl_request_verdict* verdict);

#define S(T) printf("S %s %zu\n", #T, sizeof(T))
#define F(T, f) printf("F %s %s %zu %zu\n", #T, #f, offsetof(T, f), sizeof(((T*)0)->f))

int main(void) {
  S(rl_request_override);
  F(rl_request_override, descriptor); F(rl_request_override, requests_per_unit); F(rl_request_override, rule_id);
  F(rl_request_override, unit); F(rl_request_override, reserved);

  S(rl_request_batch_packed);
  F(rl_request_batch_packed, n_requests); F(rl_request_batch_packed, n_descriptors);
  F(rl_request_batch_packed, n_entries); F(rl_request_batch_packed, n_rules);
  F(rl_request_batch_packed, n_overrides); F(rl_request_batch_packed, reserved);
  F(rl_request_batch_packed, buf); F(rl_request_batch_packed, buf_bytes);
  F(rl_request_batch_packed, req); F(rl_request_batch_packed, now); F(rl_request_batch_packed, hits);
  F(rl_request_batch_packed, desc); F(rl_request_batch_packed, key_len); F(rl_request_batch_packed, value_len);
  F(rl_request_batch_packed, domain_bytes); F(rl_request_batch_packed, entry_bytes);
  F(rl_request_batch_packed, overrides); F(rl_request_batch_packed, index);

  printf("C RL_ABI_VERSION %u\n", (unsigned)RL_ABI_VERSION);
  printf("C RL_REQUESTS_TILE %u\n", (unsigned)RL_REQUESTS_TILE);
  printf("C RL_REQUESTS_INFLIGHT %u\n", (unsigned)RL_REQUESTS_INFLIGHT);
  return 0;
}
