// rl_engine_int.h — the file-local helpers of rl_engine.hip (where they are
// defined and described) that rl_maint.hip needs too. Hidden symbols.
#pragma once

#include <algorithm>

#include "rl_engine.h"

namespace rl {

RL_INTERNAL int set_err(Engine* c, int code, const std::string& msg);
RL_INTERNAL int map_err(Engine* c, uint32_t e);
RL_INTERNAL hipError_t after_batches(Engine* c, hipStream_t st);
RL_INTERNAL TableDev table_view(Engine* c);
RL_INTERNAL Params params(Engine* c, int isolate = 0);
RL_INTERNAL hipError_t log_ctr_get(Engine* c, std::vector<unsigned long long>& ctr, unsigned long long* lost,
                                   unsigned long long* refused = nullptr);

template <typename T>
hipError_t dalloc(T** p, size_t count) {
  return hipMalloc((void**)p, std::max<size_t>(count, 1) * sizeof(T));
}

}  // namespace rl

#define HIPCHK(c, expr)                                                                        \
  do {                                                                                         \
    hipError_t _e = (expr);                                                                    \
    if (_e != hipSuccess)                                                                      \
      return set_err((c), RL_E_HIP, std::string("gpu: ") + #expr + ": " + hipGetErrorString(_e)); \
  } while (0)

// Every entry point but the packed request one and eng_batch_progress starts
// by completing the pending packed request batches (eng_requests_advance).
#define RQ_SETTLE(c)                                               \
  do {                                                             \
    if ((c)->rq_n) {                                               \
      const int _rc = rl::eng_requests_advance((c), (c)->rq_n);    \
      if (_rc) return _rc;                                         \
    }                                                              \
  } while (0)
