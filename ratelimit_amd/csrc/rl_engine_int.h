// rl_engine_int.h — the file-local helpers of rl_engine.hip (where they are
// defined and described) that rl_maint.hip and rl_requests.hip need too.
// Hidden symbols.
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
// (the batch path, which every request batch ends in)
RL_INTERNAL uint32_t enqueue(Engine* c, const BatchDev& b, const OutDev& o, int restore, hipStream_t st, bool pipelined);
RL_INTERNAL BatchDev dev_view(const Engine* c, const rl_batch* in, uint32_t stem_cap);
RL_INTERNAL int collect(Engine* c, hipStream_t st = nullptr);
RL_INTERNAL int grow(Engine* c, uint8_t** p, size_t* cap, size_t need, size_t pad);
RL_INTERNAL rl_batch staged_batch(uint32_t n, uint32_t n_requests, uint32_t n_rules, const uint8_t* stem,
                                  const uint32_t* off, const int64_t* now, const uint32_t* req, const uint8_t* unit,
                                  const uint8_t* flags, const uint32_t* limit, const uint32_t* hits,
                                  const uint32_t* rule);
// (rl_requests.hip's, for eng_destroy)
RL_INTERNAL void free_request_slots(Engine* c);

template <typename T>
hipError_t dalloc(T** p, size_t count) {
  return hipMalloc((void**)p, std::max<size_t>(count, 1) * sizeof(T));
}

// Device arrays into the caller's host arrays by a kernel's stores on `st`,
// ToHost's capacity at a time (the pipelined calls: a DMA copy back would
// queue behind the next batch's input copy). A null array or no bytes: skipped.
struct RL_INTERNAL ToHostList {
  ToHost th{};
  hipStream_t st;
  hipError_t e = hipSuccess;
  explicit ToHostList(hipStream_t s) : st(s) {}
  void flush() {
    if (th.n && e == hipSuccess) e = copy_to_host(th, st);
    th.n = 0;
  }
  void operator()(void* dst, const void* src, uint64_t bytes) {
    if (!dst || !bytes) return;
    if (th.n == TO_HOST_MAX) flush();
    th.dst[th.n] = (uint8_t*)dst;
    th.src[th.n] = (const uint8_t*)src;
    th.bytes[th.n++] = bytes;
  }
};

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
