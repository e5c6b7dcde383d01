// rl_shard_split.h — a CSR stem list split by owning shard on the host, for a
// ctx of several shards (rl_api.hip: rl_restore, rl_import, rl_lookup,
// rl_forget). Plain C++, also built by tests/c_abi/maint_host_run.cpp.
#pragma once

#include <stdint.h>

#include <vector>

namespace rlsplit {

// One shard's part: its entries' indices, in the caller's order, and their stems as a list of their own.
struct Sub {
  std::vector<uint32_t> idx;
  std::vector<uint8_t> stems;
  std::vector<uint32_t> off{0};  // [idx.size() + 1], from 0 to stems.size()
};

// owner(stem, len) -> the entry's shard, below n_shards. False when an entry's
// offsets decrease; nothing of that entry or a later one is read.
template <typename F>
inline bool split(uint32_t n, const uint8_t* stem_bytes, const uint32_t* stem_off, uint32_t n_shards, F owner,
                  std::vector<Sub>* out) {
  out->assign(n_shards, Sub{});
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t a = stem_off[i], b = stem_off[i + 1];
    if (b < a) return false;
    Sub& s = (*out)[owner(stem_bytes + a, b - a)];
    s.idx.push_back(i);
    s.stems.insert(s.stems.end(), stem_bytes + a, stem_bytes + b);
    s.off.push_back((uint32_t)s.stems.size());
  }
  return true;
}

// col[idx[0]], col[idx[1]], ...; a null (optional) column reads as zeros
template <typename T>
inline std::vector<T> take(const T* col, const std::vector<uint32_t>& idx) {
  std::vector<T> v(idx.size(), T());
  if (col)
    for (size_t x = 0; x < idx.size(); x++) v[x] = col[idx[x]];
  return v;
}

// the reverse: out[idx[x]] = sub[x] (sub: idx.size() elements)
template <typename T>
inline void put(T* out, const std::vector<uint32_t>& idx, const T* sub) {
  for (size_t x = 0; x < idx.size(); x++) out[idx[x]] = sub[x];
}

}  // namespace rlsplit
