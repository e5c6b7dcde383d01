/* respond_layout.c — the response additions of the C ABI as a C99 compiler
 * sees them (test program, like wire_layout.c): one line per struct ("S name
 * size"), per field ("F struct field offset size") and per constant ("C name
 * value") for tests/test_respond_cpu.py to compare with ratelimit_amd/abi.py. */
#include <stddef.h>
#include <stdio.h>

#include "ratelimit_hip.h"

#define S(T) printf("S %s %zu\n", #T, sizeof(T))
#define F(T, f) printf("F %s %s %zu %zu\n", #T, #f, offsetof(T, f), sizeof(((T*)0)->f))
#define K(c) printf("C %s %lu\n", #c, (unsigned long)(c))

int main(void) {
  S(rl_response_format);
  F(rl_response_format, limit_key); F(rl_response_format, remaining_key); F(rl_response_format, reset_key);
  F(rl_response_format, limit_key_len); F(rl_response_format, remaining_key_len);
  F(rl_response_format, reset_key_len); F(rl_response_format, reserved);

  S(rl_response_batch);
  F(rl_response_batch, bytes); F(rl_response_batch, bytes_cap); F(rl_response_batch, resp_off);

  K(RL_ABI_VERSION); K(RL_RESPONSE_KEY_MAX); K(RL_RESPONSE_STATUS_MAX); K(RL_NO_DESCRIPTOR); K(RL_MATCH_LIMIT);
  return 0;
}
