// rl_log_geom.h — how a requested rl_config.history_entries becomes the
// history log's geometry. Plain C++ (no HIP): rl_create (eng_create),
// rl_resize_history and a stand-alone host test (tests/c_abi/log_geom_run.cpp)
// share it. The partition count and a partition's largest size are arguments
// (LOG_PARTS and LOG_PART_MAX of rl_device.h in the library).
#pragma once

#include <stdint.h>

namespace rl {

// Entries per partition for a request of history_entries (> 0) on a ctx whose
// batches hold up to max_batch descriptors: a power of two, at least
// max(history_entries / parts, max_batch / 16, 1024) and at most part_max. A
// batch's appends are spread over the partitions by workgroup and wave, but a
// skewed one (a hot key replayed serially, the exact path's 8 workgroups) can
// send more than that to one partition: log_append then refuses the excess
// (rl_table_info.history_refused; those windows' later lookups are RL_E_TIME)
// rather than wrap onto entries of the same batch.
inline uint64_t log_part_cap(uint64_t history_entries, uint32_t max_batch, uint32_t parts, uint64_t part_max) {
  uint64_t want = history_entries / parts;
  if (want < max_batch / 16u) want = max_batch / 16u;
  if (want < 1024) want = 1024;
  uint64_t cap = 1;
  while (cap * 2 <= want && cap * 2 <= part_max) cap *= 2;
  if (cap < want && cap < part_max) cap *= 2;
  return cap;
}

// A request the rule can serve: more than parts x part_max entries cannot be
// addressed (an entry pointer is partition << LOG_POS_BITS | position).
inline bool log_entries_fit(uint64_t history_entries, uint32_t parts, uint64_t part_max) {
  return history_entries <= (uint64_t)parts * part_max;
}

}  // namespace rl
