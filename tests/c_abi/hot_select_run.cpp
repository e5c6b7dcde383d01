// hot_select_run.cpp — rl_hot_select.h compiled for the host (test program,
// tests/test_hot_cpu.py): the match predicate, the answer's order and the
// shard merge against plain restatements, on random record sets whose counts
// sit on the radix select's digit boundaries.
//
//   g++ -std=c++17 -Wall -Wextra -I ratelimit_amd/csrc hot_select_run.cpp
//
// Prints "ok <sets checked>" and exits 0, or the first difference and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <tuple>
#include <vector>

#include "rl_hot_select.h"

namespace {

struct Row {
  std::string stem;
  uint32_t unit, ws, count, expire, lc;
};

const uint32_t EDGE[] = {0u, 1u, 2u, 255u, 256u, 65535u, 65536u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFFu};
const uint32_t DIV[] = {0, 1, 60, 3600, 86400};

[[noreturn]] void die(const char* what, int set) {
  printf("FAIL set %d: %s\n", set, what);
  exit(1);
}

// the predicate, restated from the header comment of rl_hot_keys
bool want_match(const Row& r, int64_t now, uint32_t min_count, uint32_t mask, bool blocked) {
  if (mask != 0 && ((mask >> r.unit) & 1u) == 0) return false;
  const int64_t ws = now - now % (int64_t)DIV[r.unit];
  if ((int64_t)r.ws != ws) return false;
  if (now > (int64_t)r.expire) return false;
  if (r.count < min_count) return false;
  if (blocked && !(now < (int64_t)r.lc)) return false;
  return true;
}

std::tuple<uint64_t, std::string, uint32_t> sort_key(const Row& r) {
  return std::make_tuple((uint64_t)0xFFFFFFFFu - r.count, r.stem, r.unit);  // (std::string compares like memcmp, shorter first)
}

rlhot::Rec rec_of(const Row& r) {
  return rlhot::Rec{r.count, r.ws, r.expire, r.lc, r.unit, (uint32_t)r.stem.size(), (const uint8_t*)r.stem.data()};
}

bool same(const rlhot::Rec& a, const Row& r) {
  return a.count == r.count && a.ws == r.ws && a.expire == r.expire && a.lc == r.lc && a.unit == r.unit &&
         a.len == r.stem.size() && std::string((const char*)a.stem, a.len) == r.stem;
}

}  // namespace

int main() {
  std::mt19937_64 rng(20240607);
  auto pick = [&](uint32_t n) { return (uint32_t)(rng() % n); };
  int sets = 0;
  for (int set = 0; set < 400; set++, sets++) {
    // sizes: empty sets, one record, a few, hundreds; every 7th set has every record tied
    const uint32_t n = set % 10 == 0 ? 0u : set % 10 == 1 ? 1u : set % 3 ? pick(40) : pick(700);
    const bool all_tied = set % 7 == 3;
    const uint32_t tied_count = EDGE[pick(10)];
    const int64_t now = 1700000000 + (int64_t)pick(200000);
    std::vector<Row> rows(n);
    for (uint32_t i = 0; i < n; i++) {
      Row& r = rows[i];
      const uint32_t L = 1 + pick(pick(4) ? 6 : 70);
      for (uint32_t b = 0; b < L; b++) r.stem.push_back((char)(pick(3) ? 'a' + pick(3) : pick(256)));
      r.unit = 1 + pick(4);
      const uint32_t cur = (uint32_t)(now - now % DIV[r.unit]);
      r.ws = pick(5) ? cur : pick(2) ? cur - DIV[r.unit] : cur + DIV[r.unit];
      r.count = all_tied ? tied_count : pick(3) ? EDGE[pick(10)] : pick(2) ? (uint32_t)rng() : pick(300);
      r.expire = pick(6) ? (uint32_t)now + pick(100) : (uint32_t)now - 1 - pick(3);
      r.lc = pick(2) ? 0u : pick(2) ? (uint32_t)now + 1 + pick(50) : (uint32_t)now - pick(2);
    }
    const uint32_t masks[] = {0u, 1u << 1, 1u << 2, (1u << 3) | (1u << 4), 0x1Eu};
    const uint32_t mask = masks[pick(5)];
    const uint32_t min_count = pick(3) ? EDGE[pick(10)] : 0u;
    const bool blocked = pick(3) == 0;
    // the predicate
    const rlhot::Query q{(uint32_t)now, min_count, mask, blocked ? rlhot::BLOCKED : 0u};
    std::vector<Row> hit;
    for (const Row& r : rows) {
      const bool w = want_match(r, now, min_count, mask, blocked);
      if (rlhot::match(q, r.unit, r.ws, r.count, r.expire, r.lc) != w) die("match differs from the restated predicate", set);
      if (w) hit.push_back(r);
    }
    if (rlhot::match(q, 2, rlhot::WS_NONE, 5, 0xFFFFFFFFu, 0xFFFFFFFFu)) die("a slot without a record matched", set);
    if (rlhot::match(rlhot::Query{(uint32_t)now, 0, 0, 0}, 0, (uint32_t)now, 5, 0xFFFFFFFFu, 0) ||
        rlhot::match(rlhot::Query{(uint32_t)now, 0, 0, 0}, 5, (uint32_t)now, 5, 0xFFFFFFFFu, 0))
      die("a unit outside 1..4 matched", set);
    // the order: against a plain sort by (count descending, stem, unit)
    std::vector<Row> want = hit;
    std::sort(want.begin(), want.end(), [](const Row& a, const Row& b) { return sort_key(a) < sort_key(b); });
    const uint32_t ks[] = {0u, 1u, (uint32_t)hit.size() / 2, (uint32_t)hit.size(), (uint32_t)hit.size() + 1, 100000u};
    for (uint32_t k : ks) {
      std::vector<rlhot::Rec> got;
      for (const Row& r : hit) got.push_back(rec_of(r));
      std::shuffle(got.begin(), got.end(), rng);
      rlhot::order_top(got, k);
      const size_t m = std::min<size_t>(k, hit.size());
      if (got.size() != m) die("order_top: size", set);
      for (size_t i = 0; i < m; i++) {
        // equal sort keys (same stem, unit and count) may swap: compare keys, then the multiset below
        const Row g{std::string((const char*)got[i].stem, got[i].len), got[i].unit, 0, got[i].count, 0, 0};
        if (sort_key(g) != sort_key(want[i])) die("order_top differs from the plain sort", set);
      }
      uint32_t thr = 7;
      uint64_t above = 7;
      rlhot::summarize(got, &thr, &above);
      uint64_t wa = 0;
      for (size_t i = 0; i < m; i++) wa += want[i].count > want[m ? m - 1 : 0].count;
      if (thr != (m ? want[m - 1].count : 0u) || above != wa) die("summarize", set);
      // the merge: 2 or 3 shards, each answering its own top k
      for (uint32_t shards = 2; shards <= 3; shards++)
        for (int tie_mode = 0; tie_mode < 2; tie_mode++) {
          std::vector<std::vector<Row>> own(shards);
          for (const Row& r : hit) own[pick(shards)].push_back(r);
          std::vector<std::vector<rlhot::Rec>> part(shards);
          for (uint32_t s = 0; s < shards; s++) {
            // tie_mode 0: a shard breaks ties as the answer's order does; 1: the other way round
            std::sort(own[s].begin(), own[s].end(), [&](const Row& a, const Row& b) {
              if (a.count != b.count) return a.count > b.count;
              return tie_mode ? sort_key(b) < sort_key(a) : sort_key(a) < sort_key(b);
            });
            for (size_t i = 0; i < own[s].size() && i < k; i++) part[s].push_back(rec_of(own[s][i]));
            std::shuffle(part[s].begin(), part[s].end(), rng);
          }
          const std::vector<rlhot::Rec> mg = rlhot::merge(part, k);
          if (mg.size() != m) die("merge: size", set);
          for (size_t i = 0; i < m; i++) {
            if (mg[i].count != want[i].count) die("merge: the counts are not the top k of the union", set);
            if (i && rlhot::before(mg[i], mg[i - 1])) die("merge: out of order", set);
            if (tie_mode == 0 && !same(mg[i], want[i]) && sort_key(Row{std::string((const char*)mg[i].stem, mg[i].len),
                                                                       mg[i].unit, 0, mg[i].count, 0, 0}) !=
                                                              sort_key(want[i]))
              die("merge differs from the plain sort", set);
          }
          // every record above the threshold is present
          const uint32_t t = m ? mg[m - 1].count : 0u;
          size_t n_above = 0, g_above = 0;
          for (const Row& r : hit) n_above += m && r.count > t;
          for (const rlhot::Rec& r : mg) g_above += r.count > t;
          if (n_above != g_above) die("merge: a record above the threshold is missing", set);
        }
    }
  }
  printf("ok %d\n", sets);
  return 0;
}
