/* wire_layout.c — the wire-path additions of the C ABI as a C99 compiler sees
 * them (test program, like abi_layout.c): one line per struct ("S name
 * size"), per field ("F struct field offset size") and per constant ("C name
 * value") for tests/test_wire_cpu.py to compare with ratelimit_amd/abi.py. */
#include <stddef.h>
#include <stdio.h>

#include "ratelimit_hip.h"

#define S(T) printf("S %s %zu\n", #T, sizeof(T))
#define F(T, f) printf("F %s %s %zu %zu\n", #T, #f, offsetof(T, f), sizeof(((T*)0)->f))
#define K(c) printf("C %s %lu\n", #c, (unsigned long)(c))

int main(void) {
  S(rl_wire_batch);
  F(rl_wire_batch, n_requests); F(rl_wire_batch, n_rules); F(rl_wire_batch, buf); F(rl_wire_batch, buf_bytes);
  F(rl_wire_batch, msg_off); F(rl_wire_batch, now); F(rl_wire_batch, msgs); F(rl_wire_batch, msgs_bytes);

  S(rl_wire_result);
  F(rl_wire_result, req_status); F(rl_wire_result, desc_first); F(rl_wire_result, n_descriptors);
  F(rl_wire_result, desc_cap); F(rl_wire_result, reserved);

  K(RL_ABI_VERSION); K(RL_WIRE_TILE); K(RL_REQUESTS_TILE); K(RL_WIRE_OK); K(RL_WIRE_DEFERRED); K(RL_WIRE_MALFORMED);
  return 0;
}
