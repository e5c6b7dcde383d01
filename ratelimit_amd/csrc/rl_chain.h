// rl_chain.h — the walk of a slot's history chain under log_find's checks,
// shared by the translation units that follow chains entry by entry
// (rl_kernels.hip: the local-cache gauge, the sweep, rl_resize's re-link;
// rl_relog.hip: rl_resize_history).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rl_device.h"
#include "rl_kernels.h"

namespace rl {

// How a walk ended: at the chain's end (LOG_NONE), because f said so, or at an
// entry the walk does not accept (overwritten: owner slot, tag or a rising
// t_app; LOG_LOST or any position past the partition; a cycle; LOG_MAX_HOPS).
enum ChainEnd : uint32_t { CHAIN_END = 0, CHAIN_STOPPED = 1, CHAIN_BROKEN = 2 };

// Walk the history chain of slot si (tag `tag`, chain head `head`, newest window
// cur_ws): f(entry, hop index) for each entry the log still holds, newest
// first (stops where one was overwritten, or when f says so). f may store to
// the entry's `slot` word (the resize's re-link): its other words are read first.
template <typename F>
__device__ inline ChainEnd chain_walk_end(const TableDev& t, uint32_t si, uint32_t tag, uint32_t head, uint32_t cur_ws,
                                          F f) {
  uint32_t ptr = head, tprev = cur_ws, saved = LOG_NONE, power = 1, lam = 0;
  for (uint32_t hops = 0; ptr != LOG_NONE; hops++) {  // (log_find's checks)
    if (hops == LOG_MAX_HOPS || ptr == saved) return CHAIN_BROKEN;
    const uint32_t pos = ptr & LOG_POS_MASK;
    if (pos >= t.log_cap) return CHAIN_BROKEN;
    if (++lam == power) {
      saved = ptr;
      power <<= 1;
      lam = 0;
    }
    LogEnt& e = t.log[(size_t)(ptr >> LOG_POS_BITS) * t.log_cap + pos];
    if (e.slot != si || e.tag != tag || e.t_app > tprev) return CHAIN_BROKEN;
    const uint32_t t_app = e.t_app, prev = e.prev;
    if (!f(e, hops)) return CHAIN_STOPPED;
    tprev = t_app;
    ptr = prev;
  }
  return CHAIN_END;
}

// ... for the callers that do not ask how it ended.
template <typename F>
__device__ inline void chain_walk_ent(const TableDev& t, uint32_t si, uint32_t tag, uint32_t head, uint32_t cur_ws, F f) {
  (void)chain_walk_end(t, si, tag, head, cur_ws, f);
}

}  // namespace rl
