/* override_layout.c — the device-interned override rules' additions of the C
 * ABI as a C99 compiler sees them (test program, like wire_layout.c): one line
 * per struct ("S name size"), per field ("F struct field offset size") and per
 * constant ("C name value") for tests/test_wire_override_cpu.py to compare
 * with ratelimit_amd/abi.py. */
#include <stddef.h>
#include <stdio.h>

#include "ratelimit_hip.h"

#define S(T) printf("S %s %zu\n", #T, sizeof(T))
#define F(T, f) printf("F %s %s %zu %zu\n", #T, #f, offsetof(T, f), sizeof(((T*)0)->f))
#define K(c) printf("C %s %lu\n", #c, (unsigned long)(c))

int main(void) {
  /* the entry points as the header declares them (unevaluated: nothing is linked) */
  (void)sizeof(rl_override_rules_enable((rl_ctx*)0, (const rl_override_rules_config*)0));
  (void)sizeof(rl_override_rules_info_get((rl_ctx*)0, (rl_override_rules_info*)0));
  (void)sizeof(rl_override_rule_keys((rl_ctx*)0, 0u, 0u, (uint8_t*)0, (uint64_t)0, (uint32_t*)0, (uint64_t*)0));
  S(rl_override_rules_config);
  F(rl_override_rules_config, first_rule); F(rl_override_rules_config, capacity);
  F(rl_override_rules_config, key_bytes); F(rl_override_rules_config, reserved);

  S(rl_override_rules_info);
  F(rl_override_rules_info, first_rule); F(rl_override_rules_info, capacity); F(rl_override_rules_info, rules);
  F(rl_override_rules_info, reserved); F(rl_override_rules_info, key_bytes_used);
  F(rl_override_rules_info, key_bytes_cap); F(rl_override_rules_info, deferred_full);

  K(RL_ABI_VERSION);
  return 0;
}
